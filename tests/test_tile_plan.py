"""The host's plan of the tile-bound pre-pass (locomouse_cpp_amd/csrc/
lm_tile_plan.h: the LmConst::tbw_* / tb_* / tbr_* fields that k_tile_bound and
k_tile_bound_ref trust without a check) on the host, without a GPU: a
stand-alone program (tests/cpp/tile_plan_check.cpp) fills the plan's inputs by
hand for a list of geometries, runs the plan and walks every view and band as
the kernel does: the LDS regions in order, disjoint, aligned and inside 64 KB;
every window's blocks and every band's rows inside the tables; the window
tables, entries and work list large enough; the pair table's read-ahead inside
its spare space; the reciprocals exact; the constants disjoint and aligned;
k_tile_bound_ref's regions inside 144 KB; the switches, the order in which
detectors lose their bound and the row-loop flag.  Once more under the
sanitizers."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "tile_plan_check.cpp")
INC = "-I" + os.path.join(ROOT, "locomouse_cpp_amd", "csrc")
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
LINE = re.compile(
    r"(?P<geoms>\d+) geometries, (?P<views>\d+) views, (?P<bands>\d+) bands, (?P<lost>\d+) lost, (?P<rowloop>\d+) rowloop, "
    r"(?P<generic>\d+) generic, (?P<unrefined>\d+) unrefined, (?P<residues>\d+) residues, "
    r"rem (?P<rem1>\d+) (?P<rem2>\d+) (?P<rem3>\d+), lastcol (?P<col1>\d+) (?P<col2>\d+), tall (?P<tall>\d+), "
    r"onerow (?P<onerow>\d+), low (?P<low>\d+), w9 (?P<w9>\d+) w70 (?P<w70>\d+), oddblk (?P<oddblk>\d+), keep101 (?P<keep101>\d+) "
    r"keep001 (?P<keep001>\d+), off (?P<off>\d+), nobound (?P<nobound>\d+), (?P<checks>\d+) checks, (?P<failures>\d+) failures")


def _build(exe, flags):
    # (the header must also be clean under the warnings the host library is built with)
    subprocess.check_call(["g++", *flags, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", INC, SRC, "-o", exe])
    return exe


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    m = LINE.search(r.stdout)
    assert m, r.stdout[-2000:]
    n = {k: int(v) for k, v in m.groupdict().items()}
    assert n["failures"] == 0
    assert n["views"] == 2 * n["geoms"] and n["bands"] > n["views"] and n["checks"] > 100 * n["views"]
    # every branch was reached: detectors that lost their bound, in both stages of the order (the snout alone, then
    # the paw too); views on the row loop (C3), on the generic loop (C5: two chunks per weight row) and unrefined
    assert n["lost"] > 0 and n["keep101"] > 0 and n["keep001"] > 0
    assert n["rowloop"] > 0 and n["generic"] > 0 and n["unrefined"] > 0
    # every in_x mod 8; last tile rows of 1, 2 and 3 output rows; last tile columns of one and two blocks
    assert n["residues"] == 8
    assert n["rem1"] > 0 and n["rem2"] > 0 and n["rem3"] > 0
    assert n["col1"] > 0 and n["col2"] > 0
    # windows that start in an odd block (the tables start at the even block before)
    assert n["oddblk"] > 0
    # a detector taller than a band, a one-row detector, widths 9 and 70, a box lower than a band's tile rows
    assert n["tall"] > 0 and n["onerow"] > 0 and n["w9"] > 0 and n["w70"] > 0 and n["low"] > 0
    # plans with a switch off, detectors with delta >= 0
    assert n["off"] > 0 and n["nobound"] > 0


def test_tile_plan_holds_what_the_kernel_relies_on(tmp_path):
    _run(_build(str(tmp_path / "tile_plan_check"), ["-O2"]))


def test_tile_plan_is_clean_under_the_sanitizers(tmp_path):
    """The same program built with -fsanitize=address,undefined; nothing is
    loaded into Python."""
    _run(_build(str(tmp_path / "tile_plan_check_san"), SAN))
