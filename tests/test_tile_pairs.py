"""The paired block ranges of the refinement (locomouse_cpp_amd/csrc/
lm_tail_bound.h: lm_tbr_pair_word, lm_tbr_pair_range, lm_tbr_quad_*: the pair
table k_tile_bound reads one entry of per term) on the host, without a GPU: a
stand-alone program (tests/cpp/tile_pair_check.cpp) builds a band's tables
from random block ranges and checks that every term read through the new
accessors has exactly the M, m that lm_tbr_block_skip takes, and that
lm_tbr_sum_negative through them returns lm_tbr_block_skip's value: detectors
9 to 70 wide at every in_x mod 8, windows that end on a block boundary, one
column and seven columns past it, a narrower detector whose window ends in an
earlier block than the table, 1 to 4 rows; once more under the sanitizers."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "tile_pair_check.cpp")
INC = "-I" + os.path.join(ROOT, "locomouse_cpp_amd", "csrc")
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
LINE = re.compile(r"(\d+) geometries, (\d+) blocks, (\d+) proven, (\d+) terms, (\d+) clipped, (\d+) earlier, (\d+) failures")


def _build(exe, flags):
    subprocess.check_call(["g++", *flags, "-std=c++17", "-ffp-contract=off", INC, SRC, "-o", exe])
    return exe


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    m = LINE.search(r.stdout)
    assert m, r.stdout[-2000:]
    geoms, blocks, proven, terms, clipped, earlier, failures = map(int, m.groups())
    assert failures == 0
    # two detectors x 62 widths x 8 residues x 3 window ends x 4 row counts
    assert geoms == 2 * 62 * 8 * 3 * 4
    # both outcomes of the sum, terms at the window's last block, and some of those with a block of the table beyond it
    assert 0 < proven < blocks
    assert 0 < earlier < clipped < terms


def test_pair_table_yields_the_terms_of_the_block_rule(tmp_path):
    _run(_build(str(tmp_path / "tile_pair_check"), ["-O2"]))


def test_pair_table_is_clean_under_the_sanitizers(tmp_path):
    """The same program built with -fsanitize=address,undefined; nothing is
    loaded into Python."""
    _run(_build(str(tmp_path / "tile_pair_check_san"), SAN))
