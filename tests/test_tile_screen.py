"""The fp32 screen in front of the refinement's block sum (locomouse_cpp_amd/
csrc/lm_tail_bound.h: lm_tbs_*, which k_tile_bound<true> runs first in step 4b)
on the host, without a GPU: a stand-alone program (tests/cpp/
tile_screen_check.cpp) compares the screen's three-way decision with the sign
of lm_tbr_sum's double, which stays the definition.  A decided item must agree
with it, every |U_d| >= 2 E must be decided, and the constants must be rounded
the way the header's proof assumes, with a margin no smaller than the proof's.
Synthetic sums (kh 1 to 40, 1 to 4 tap groups at every in_x mod 8, biases that
put U_d at zero, a few ulps to either side, at -+E/2 and beyond -+2 E),
adversarial weights, the views of frames 0-99 of the default C3 scene, and
planted errors in a copy of the header, which must each be caught.  Once more
under the sanitizers; nothing is loaded into Python."""
import os
import re
import subprocess

import pytest

from locomouse_cpp_amd import synthetic as S
from test_tile_refine import DETS
from test_tile_sum_rows import write_views

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "tile_screen_check.cpp")
CSRC = os.path.join(ROOT, "locomouse_cpp_amd", "csrc")
HEADER = os.path.join(CSRC, "lm_tail_bound.h")
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
SUMS = re.compile(r"(\d+) cases, (\d+) sums, (\d+) negative, (\d+) positive, (\d+) undecided, (\d+) disagreements, "
                  r"(\d+) undecided beyond 2E, (\d+) const_fails")
SET = re.compile(r"set (.+): screened (\d) sums (\d+) undecided (\d+) disagreements (\d+) const_fails (\d+)")
VIEW = re.compile(r"det (\d): screened (\d) items (\d+) negative (\d+) undecided (\d+) disagreements (\d+) const_fails (\d+)")

# (name, the header's text, its replacement): each must make the checker fail
PLANTED = (
    ("the margin halved", "R.E = R.on ? lm_tbs_up(E) : 0.f;", "R.E = R.on ? lm_tbs_up(0.5 * E) : 0.f;"),
    ("the margin zero", "R.E = R.on ? lm_tbs_up(E) : 0.f;", "R.E = 0.f;"),
    ("Pf rounded down", "const float pf = lm_tbs_up(p),", "const float pf = lm_tbs_down(p),"),
    ("Nf rounded up", "nf = lm_tbs_down(n);", "nf = lm_tbs_up(n);"),
    ("the bias rounded down", "R.bf = lm_tbs_up(bias);", "R.bf = lm_tbs_down(bias);"),
)


def _build(exe, flags, inc=CSRC):
    subprocess.check_call(["g++", *flags, "-std=c++17", "-ffp-contract=off", "-I" + inc, SRC, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("tile_screen") / "tile_screen_check"), ["-O2"])


@pytest.fixture(scope="module")
def checker_san(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("tile_screen_san") / "tile_screen_check_san"), SAN)


def _run(exe, *args, fails=False):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert (r.returncode == 1) if fails else (r.returncode == 0), r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def _sums(exe):
    m = SUMS.search(_run(exe, "sums"))
    assert m
    cases, sums, neg, pos, und, dis, beyond, cfail = map(int, m.groups())
    assert dis == 0 and beyond == 0 and cfail == 0
    # kh 1 .. 40 x 1 .. 4 groups x 8 residues; five range sets of twelve biases each (the all-zero ranges put the
    # biases "a few ulps from zero" below FLT_MIN, where the gate refuses them)
    assert cases == 40 * 4 * 8 and cases * 5 * 10 < sums <= cases * 5 * 12
    assert neg > 0 and pos > 0 and und > 0, (neg, pos, und)


def _adversarial(exe):
    rows = {m[0]: tuple(map(int, m[1:])) for m in SET.findall(_run(exe, "adversarial"))}
    assert len(rows) == 10, rows
    for name, (on, sums, und, dis, cfail) in rows.items():
        assert dis == 0 and cfail == 0, (name, rows[name])
        assert (sums > 0) == bool(on), (name, rows[name])
    # the gate: a constant below FLT_MIN and sums the floats cannot hold switch the screen off; the others pass it
    off = {n for n, r in rows.items() if not r[0]}
    assert off == {"weights below FLT_MIN", "sums beyond the floats"}, off


def _views(exe, path):
    rows = [tuple(map(int, m)) for m in VIEW.findall(_run(exe, "views", path))]
    assert len(rows) == len(DETS), rows
    for _, on, items, neg, und, dis, cfail in rows:
        assert on == 1 and dis == 0 and cfail == 0, rows
    return rows


def test_decided_sums_agree_with_the_double_sum(checker):
    _sums(checker)


def test_adversarial_weights(checker):
    _adversarial(checker)


def test_views_of_the_synthetic_frames(checker, tmp_path):
    """Frames 0-99 of the default C3 scene: no decided item disagrees with the
    double sum, and fewer than 1 % of the items are undecided (measured: 85 of
    205,990 items, 0.041 %; per detector 38, 33, 0, 3, 2, 9)."""
    cfg = S.SyntheticConfig()
    rows = _views(checker, write_views(cfg, cfg.frames(0, 100), tmp_path / "views100.bin"))
    for d, _, items, neg, und, _, _ in rows:
        print(f"det {d}: {und} of {items} items undecided ({100.0 * und / items:.4f} %), {neg} negative")
        assert 0 < neg < items, rows
    items, und = sum(r[2] for r in rows), sum(r[4] for r in rows)
    print(f"all: {und} of {items} items undecided ({100.0 * und / items:.4f} %)")
    assert und < 0.01 * items, (und, items)


@pytest.mark.parametrize("name,old,new", PLANTED, ids=[p[0].replace(" ", "_") for p in PLANTED])
def test_planted_errors_are_caught(name, old, new, tmp_path):
    with open(HEADER) as fh:
        text = fh.read()
    assert text.count(old) == 1, (name, old)
    with open(tmp_path / "lm_tail_bound.h", "w") as fh:
        fh.write(text.replace(old, new))
    exe = _build(str(tmp_path / "tile_screen_check_planted"), ["-O2"], inc=str(tmp_path))
    m = SUMS.search(_run(exe, "sums", fails=True))
    assert m
    dis, beyond, cfail = map(int, m.groups()[5:])
    assert dis + beyond + cfail > 0, (name, m.groups())


def test_clean_under_the_sanitizers(checker_san, tmp_path):
    """The same program built with -fsanitize=address,undefined: both synthetic
    modes and the views of frame 0; nothing is loaded into Python."""
    _sums(checker_san)
    _adversarial(checker_san)
    cfg = S.SyntheticConfig()
    _views(checker_san, write_views(cfg, cfg.frames(0, 1), tmp_path / "views1.bin"))
