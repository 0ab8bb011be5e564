"""The narrow class of ring work items (locomouse_cpp_amd/csrc/lm_corr_narrow.h)
on the host, without a GPU: a stand-alone program
(tests/cpp/narrow_class_check.cpp) checks the classification of every block
mask, the items' geometry and owned columns, the narrow wave directory, and --
on synthetic detectors and on the oracle's own windows of synthetic C3 frames
0-8 -- that the mask is lm_tbr_block_skip's block by block; once more under the
sanitizers; and that three errors planted in a copy of the header are each
caught.  The crops run prints the per-detector table of kept tiles by unproven
blocks, so the counts behind the class are on record."""
import os
import re
import subprocess

import pytest

from test_tile_refine import DETS, crops  # noqa: F401  (the fixture that records the six detectors' views)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "narrow_class_check.cpp")
CSRC = os.path.join(ROOT, "locomouse_cpp_amd", "csrc")
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
ROW = re.compile(r"det (\d): kept (\d+) blocks (\d+) unproven (\d+) by-count (\d+) (\d+) (\d+) (\d+) (\d+) span2 (\d+) "
                 r"untried (\d+) macs (\d+) narrow-macs (\d+) failures (\d+)")


def _build(exe, flags, inc=CSRC):
    subprocess.check_call(["g++", *flags, "-std=c++17", "-ffp-contract=off", "-I" + inc, "-I" + CSRC, SRC, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("narrow") / "narrow_class_check"), ["-O2"])


@pytest.fixture(scope="module")
def checker_san(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("narrow_san") / "narrow_class_check_san"), SAN)


def _run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=900)
    print(r.stdout[-4000:])
    return r


def _masks(exe):
    r = _run(exe, "masks")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    m = re.search(r"masks (\d+) narrow (\d+) wide (\d+) grids (\d+) waves (\d+) failures 0", r.stdout)
    assert m, r.stdout
    masks, narrow, wide, grids, waves = map(int, m.groups())
    # 2 tiles x 8 widths of the last block x (2^nb - 1 masks of nb = 1 .. 5 blocks) x tried / untried
    assert masks == 2 * 8 * (1 + 3 + 7 + 15 + 31) * 2 and narrow + wide == masks
    # tried masks of one block or two adjacent ones: nb + (nb - 1) per nb
    assert narrow == 2 * 8 * sum(nb + nb - 1 for nb in range(1, 6))
    assert grids == 400 and waves > 10000


def _synth(exe):
    r = _run(exe, "synth")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    m = re.search(r"synth (\d+) cases tiles (\d+) kept (\d+) narrow (\d+) failures 0", r.stdout)
    assert m, r.stdout
    cases, tiles, kept, narrow = map(int, m.groups())
    assert cases >= 300 and 0 < narrow < kept < tiles  # no side is vacuous


def _crops(exe, path):
    r = _run(exe, "crops", path)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rows = [tuple(map(int, m)) for m in ROW.findall(r.stdout)]
    assert len(rows) == len(DETS), r.stdout
    return rows


def test_every_mask_and_the_directory(checker):
    _masks(checker)


def test_mask_is_block_skip_on_synthetic_detectors(checker):
    _synth(checker)


def test_mask_and_counts_on_the_synthetic_frames(checker, crops):  # noqa: F811
    """Frames 0-8: the mask equals the refinement block by block and the tile
    rule as a whole, every narrow item owns its unproven blocks inside its
    tile, and the table's columns are consistent; every detector has narrow
    tiles, each at half the multiply-adds of a whole tile."""
    for (_, name, _, _), row in zip(DETS, _crops(checker, crops[9])):
        _, kept, blocks, unproven, c1, c2, c3, c4, c5, span2, untried, macs, nmacs, fails = row
        assert fails == 0
        assert c1 + c2 + c3 + c4 + c5 == kept and c1 + 2 * c2 + 3 * c3 + 4 * c4 + 5 * c5 == unproven
        assert 0 < unproven < blocks <= 5 * kept
        assert span2 <= c1 + c2 and untried <= kept - span2  # narrow needs at most two blocks, and a tried tile
        assert span2 > 0 and nmacs == macs - (macs // kept // 2) * span2 < macs, (name, span2, kept)


def test_clean_under_the_sanitizers(checker_san, crops):  # noqa: F811
    """The same program built with -fsanitize=address,undefined; nothing is
    loaded into Python."""
    _masks(checker_san)
    _synth(checker_san)
    _crops(checker_san, crops[1])


PLANTS = {
    "an origin not clamped to the tile": ("return o < LM_FW - LM_NW_FW ? o : LM_FW - LM_NW_FW;", "return o;"),
    "a span of three blocks treated as narrow": ("if (last - first + 1 > LM_NW_SPAN) return c;",
                                                 "if (last - first + 1 > LM_NW_SPAN + 1) return c;"),
    "ownership one block too wide": ("LM_NW_BLK * (first + count);", "LM_NW_BLK * (first + count + 1);"),
}


@pytest.mark.parametrize("plant", sorted(PLANTS))
def test_planted_errors_are_caught(tmp_path, plant):
    old, new = PLANTS[plant]
    inc = tmp_path / "inc"
    inc.mkdir()
    with open(os.path.join(CSRC, "lm_corr_narrow.h")) as fh:
        text = fh.read()
    assert text.count(old) == 1, old
    (inc / "lm_corr_narrow.h").write_text(text.replace(old, new))
    exe = _build(str(tmp_path / "planted"), ["-O2"], inc=str(inc))
    r = _run(exe, "masks")
    assert r.returncode == 1 and "FAIL" in r.stdout, (plant, r.stdout[-1000:])
