"""The refinement's loop for detectors of one chunk per row (k_tile_bound<true>
step 4b: lm_tbr_sum_rows_n where every refined detector's weight rows are one
chunk of constants; k_tile_bound<false>, the generic loop alone, elsewhere) at
the smallest inputs that take each path.  The method is
test_gpu_tile_refine_dense.py's: one batch with the refinement on, with it off
and through k_tile_bound_ref; the results are bit-identical to each other and
to the oracle, the flags and work counters equal the reference kernel's.

Every case also evaluates the per-block rule on its own frames on the host
(tests/cpp/tile_sum_rows_check.cpp `views`, on the views test_tile_sum_rows.py
writes) and asserts that the class of tile it is there for occurs -- kept by
an end block, kept by a middle block only, proven (every block summed, none
unproven) -- so a scene that stops producing its case fails instead of passing
vacuously; and that the host's counts are the kernel's: per detector, the
tiles the tile bound fails are the tiles listed with the refinement off, the
kept ones the tiles listed with it on.  (The classes come from the order "end
blocks first", which the kernel ran in two rounds while it was measured; it
sums all blocks of a tile at once now, DESIGN.md section 12, and the cases are
kept as they cover the kept, the proven and the short-column tiles.)"""
import subprocess

import numpy as np
import pytest

import edge_scenes as E
from locomouse_cpp_amd import synthetic as S
from test_gpu_tile_refine_dense import _three
from test_tile_refine import DETS
from test_tile_sum_rows import VIEW, _build, write_views

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("tile_rounds") / "tile_sum_rows_check"), ["-O2"])


def _host(checker, cfg, frames, tmp_path):
    """Per detector (DETS' order) the host's count of tiles the tile bound
    fails, and of those: kept by an end block, kept by a middle block only,
    proven, in a last tile column of fewer than five blocks."""
    flip = bool(cfg.setup.flip)  # (the pipeline mirrors the frame before anything else; so does the background)
    path = write_views(cfg, frames, tmp_path / "views.bin", flip=flip)
    r = subprocess.run([checker, "views", str(path)], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rows = [tuple(map(int, m)) for m in VIEW.findall(r.stdout)]
    assert len(rows) == len(DETS), r.stdout
    return [{"refined": refined, "end": ends, "middle": kept - ends, "proven": refined - kept, "short": short}
            for _, refined, kept, ends, _, _, _, short, failures in rows if failures == 0]


def _run(checker, cfg, frames, monkeypatch, tmp_path, label):
    """The three modes on the GPU, the rule on the host, and the host's counts
    against the kernel's work counters (point detectors 0, 1, 3, 4 of DETS,
    tail detectors 2 and 5)."""
    host = _host(checker, cfg, frames, tmp_path)
    assert len(host) == len(DETS)
    (pw, tw, pw0, tw0), out = _three(cfg, frames, monkeypatch, label)
    kept = [h["end"] + h["middle"] for h in host]
    refined = [h["refined"] for h in host]
    assert tuple(pw["listed"]) == tuple(kept[d] for d in (0, 1, 3, 4)), (label, pw, host)
    assert tuple(tw["listed"]) == tuple(kept[d] for d in (2, 5)), (label, tw, host)
    assert tuple(pw0["listed"]) == tuple(refined[d] for d in (0, 1, 3, 4)), (label, pw0, host)
    assert tuple(tw0["listed"]) == tuple(refined[d] for d in (2, 5)), (label, tw0, host)
    return host


def _total(host, key, dets=range(6)):
    return sum(host[d][key] for d in dets)


@pytest.mark.parametrize("flip", [False, True])
def test_default_scene(flip, checker, monkeypatch, tmp_path):
    """Frames 20-23: every detector has tiles kept by an end block and proven
    ones, the point detectors also tiles kept by a middle block only."""
    cfg = S.SyntheticConfig(flip=flip)
    host = _run(checker, cfg, cfg.frames(20, 4), monkeypatch, tmp_path, f"rounds, default scene, flip {flip}: ")
    for d in range(6):
        assert host[d]["end"] > 0 and host[d]["proven"] > 0, (d, host)
    for d in (0, 1, 3, 4):
        assert host[d]["middle"] > 0, (d, host)


def test_every_tile_kept_by_an_end_block(checker, monkeypatch, tmp_path):
    """The period-2 checkerboard: every tile fails at an end block; no entry
    drops out of any band."""
    cfg = S.SyntheticConfig()
    host = _run(checker, cfg, E.checker_frames(cfg, 2, period=2), monkeypatch, tmp_path, "rounds, checker 2: ")
    for d in range(6):
        assert host[d]["end"] == host[d]["refined"] > 0 and host[d]["middle"] == host[d]["proven"] == 0, (d, host)


def test_nearly_empty_bands(checker, monkeypatch, tmp_path):
    """Blank frames with one bright 12 x 12 patch inside each box: most bands
    have no item, the others a few tiles kept by an end block."""
    cfg = S.SyntheticConfig()
    p = cfg.params
    frames = np.stack([E.blank(cfg)] * 3)
    bot, side = p.bounding_box_bottom, p.bounding_box_side
    for k, f in enumerate(frames):
        f[bot.y + 2:bot.y + 14, bot.x + 2 + k:bot.x + 14 + k] = 255
        f[side.y + side.height - 14:side.y + side.height - 2, side.x + side.width - 14 - k:side.x + side.width - 2 - k] = 255
    host = _run(checker, cfg, frames, monkeypatch, tmp_path, "rounds, patches: ")
    assert 0 < _total(host, "end") and _total(host, "refined") <= 20 * len(frames), host


def test_every_refined_tile_proven(checker, monkeypatch, tmp_path):
    """A faint 30 x 30 square (50 above the background, under a bright patch
    outside the boxes that fixes the frame's maximum) inside the bottom box:
    the tile bound fails 12 tiles per frame of paw_bottom and of snout_bottom
    and every block of them is proven, so their bands have items and no mark,
    and the final compaction empties their segments."""
    cfg = S.SyntheticConfig()
    p = cfg.params
    bot = p.bounding_box_bottom
    frames = np.stack([E.blank(cfg)] * 2)
    b = cfg.background.astype(np.int32)
    for k, f in enumerate(frames):
        f[8:40, 8:40] = 255
        y, x = bot.y + 50, bot.x + 150 + 3 * k
        f[y:y + 30, x:x + 30] = np.minimum(b[y:y + 30, x:x + 30] + 50, 255)
    host = _run(checker, cfg, frames, monkeypatch, tmp_path, "rounds, faint square: ")
    for d in (0, 1):
        assert host[d]["proven"] == host[d]["refined"] > 0, (d, host)
    assert _total(host, "end") == _total(host, "middle") == 0, host


@pytest.mark.parametrize("width", [368, 376])
def test_last_tile_columns_of_one_and_two_blocks(width, checker, monkeypatch, tmp_path):
    """Boxes 368 wide (a last tile column of one block) and 376 wide (two
    blocks); a 30 x 30 square 60 above the background at the right edge of each
    box puts tiles the tile bound fails into those columns."""
    cfg = S.SyntheticConfig(bounding_boxes={"side": (300, 3, width, 90), "bottom": (300, 106, width, 140)})
    p = cfg.params
    frames = cfg.frames(20, 2)
    b = cfg.background.astype(np.int32)
    for k, f in enumerate(frames):
        for box in (p.bounding_box_bottom, p.bounding_box_side):
            y, x = box.y + box.height // 2 - 15, box.x + box.width - 32 - 3 * k
            f[y:y + 30, x:x + 30] = np.minimum(b[y:y + 30, x:x + 30] + 60, 255)
    host = _run(checker, cfg, frames, monkeypatch, tmp_path, f"rounds, boxes {width} wide: ")
    for d in (0, 1, 3, 4):
        assert host[d]["short"] > 0 and host[d]["end"] > 0 and host[d]["middle"] > 0 and host[d]["proven"] > 0, (d, host)


def test_one_and_two_chunks_in_one_view(checker, monkeypatch, tmp_path):
    """snout_bottom 36 x 36 next to paw_bottom 24 x 24 and tail_bottom: its
    window starts at column 0 of the crop (five tap groups, two chunks per
    row: lm_tbr_sum), theirs at columns 6 and 7 (four groups, one chunk:
    lm_tbr_sum_rows_n), so both loops of k_tile_bound<true> run in one workgroup."""
    w = {"snout_bottom": S.dog_detector(36, 36, 6.0, 85)}
    base = S.SyntheticConfig(weights=w)
    cfg = S.SyntheticConfig(weights=w, biases=E._bias_for_rate(base, ["snout_bottom"]))
    shapes = {n: cfg.weights[n].shape for _, n, v, _ in DETS if v == 0}
    groups = {n: ((max(s[1] // 2 for s in shapes.values()) - kw // 2) % 8 + kw - 1) // 8 + 1 for n, (_, kw) in shapes.items()}
    assert groups["snout_bottom"] == 5 and groups["paw_bottom"] <= 4 and groups["tail_bottom"] <= 4, groups
    host = _run(checker, cfg, cfg.frames(10, 2), monkeypatch, tmp_path, "rounds, 36 wide: ")
    for d in (0, 1, 2):
        assert host[d]["end"] > 0 and host[d]["proven"] > 0, (d, host)
