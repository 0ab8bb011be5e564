"""The ring correlation's wave directory (locomouse_cpp_amd/csrc/lm_corr_dir.h:
what k_corr_dir writes per launch group and corr_locate_rw looks its wave up
in) on the host, without a GPU: a stand-alone program
(tests/cpp/corr_dir_check.cpp) locates every wave of a grid twice, by the walk
over the group's detectors that the kernels used before and by the directory
record, for counter sets that are all zero, hold a single entry, hold exact
multiples of 8 and one more, fill the grid, mix listed and unlisted detectors
in groups of 1 to 6, and a few hundred seeded random ones; both must agree on
(detector, segment, place, valid sub-tiles) below the total and find nothing
at or past it.  Once more under the sanitizers."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "corr_dir_check.cpp")
INC = "-I" + os.path.join(ROOT, "locomouse_cpp_amd", "csrc")
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
LINE = re.compile(
    r"(?P<groups>\d+) groups, (?P<waves>\d+) waves, (?P<empty>\d+) empty, (?P<full>\d+) full, (?P<mixed>\d+) mixed, "
    r"n (?P<n1>\d+) (?P<n2>\d+) (?P<n3>\d+) (?P<n4>\d+) (?P<n5>\d+) (?P<n6>\d+), (?P<past>\d+) past, "
    r"(?P<checks>\d+) checks, (?P<failures>\d+) failures")


def _build(exe, flags):
    # (the header must also be clean under the warnings the host library is built with)
    subprocess.check_call(["g++", *flags, "-std=c++17", "-Wall", "-Wextra", "-Werror", INC, SRC, "-o", exe])
    return exe


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    m = LINE.search(r.stdout)
    assert m, r.stdout[-2000:]
    n = {k: int(v) for k, v in m.groupdict().items()}
    assert n["failures"] == 0
    assert n["groups"] > 700 and n["checks"] > 2 * n["waves"]
    # every kind of set was reached: empty groups, groups whose lists fill the grid, listed and unlisted detectors
    # in one group, every group size, and waves past the total
    assert n["empty"] >= 6 and n["full"] >= 48 and n["mixed"] > 50 and n["past"] > 0
    assert all(n[f"n{k}"] > 50 for k in range(1, 7))


def test_directory_lookup_matches_the_walk(tmp_path):
    _run(_build(str(tmp_path / "corr_dir_check"), ["-O2"]))


def test_directory_lookup_is_clean_under_the_sanitizers(tmp_path):
    """The same program built with -fsanitize=address,undefined; nothing is
    loaded into Python."""
    _run(_build(str(tmp_path / "corr_dir_check_san"), SAN))
