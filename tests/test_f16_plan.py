"""The plan of the f16 correlation (locomouse_cpp_amd/csrc/lm_corr_f16.h: the
chunk count of a detector width, the LDS window, the host's layout of the B
fragments) on the host, without a GPU: a stand-alone program
(tests/cpp/f16_plan_check.cpp) checks the chunk count of every width 1..130,
every LDS address k_corr_f16 forms for every chunk count 2..10 (inside the
window, aligned), the 160 KiB acceptance cap, and emulates one workgroup in
integers -- f16_bfrag_weight's fragments and the A fragments at the kernel's
addresses, combined by the MFMA's lane maps and the kernel's tile-0 / tile-1
pairing -- against the direct sums, for three widths of every class and
detector heights 1, 2, 3, 4, 5 and 7.  Once more under the sanitizers."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "f16_plan_check.cpp")
INC = "-I" + os.path.join(ROOT, "locomouse_cpp_amd", "csrc")
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
LINE = re.compile(r"nch(?P<nch>( \d+:\d+)+), kh(?P<kh>( \d+:\d+)+), (?P<workgroups>\d+) workgroups, (?P<sums>\d+) sums, "
                  r"(?P<checks>\d+) checks, (?P<failures>\d+) failures")


def _build(exe, flags):
    # (the header must also be clean under the warnings the host library is built with)
    subprocess.check_call(["g++", *flags, "-std=c++17", "-Wall", "-Wextra", "-Werror", INC, SRC, "-o", exe])
    return exe


def _counts(text):
    return {int(k): int(v) for k, v in (p.split(":") for p in text.split())}


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    m = LINE.search(r.stdout)
    assert m, r.stdout[-2000:]
    assert int(m["failures"]) == 0
    nch, kh = _counts(m["nch"]), _counts(m["kh"])
    # every class and every height was emulated: class 2 holds the single width 1, the others three widths
    assert sorted(nch) == list(range(2, 11)) and sorted(kh) == [1, 2, 3, 4, 5, 7]
    assert nch[2] == 6 and all(nch[n] == 18 for n in range(3, 11))
    assert all(v == 25 for v in kh.values())
    assert int(m["workgroups"]) == 150 and int(m["sums"]) == 150 * 128 * 64
    assert int(m["checks"]) > 100000


def test_f16_plan_and_fragment_layout(tmp_path):
    _run(_build(str(tmp_path / "f16_plan_check"), ["-O2"]))


def test_f16_plan_is_clean_under_the_sanitizers(tmp_path):
    """The same program built with -fsanitize=address,undefined; nothing is
    loaded into Python."""
    _run(_build(str(tmp_path / "f16_plan_check_san"), SAN))
