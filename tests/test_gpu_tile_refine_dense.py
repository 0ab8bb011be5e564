"""The refinement's single pass over a band's three detectors (k_tile_bound
step 4b: the (tile, output block) items of all detectors in wave-sized chunks,
terms read from the windows' pair table, one compaction of the three entry
segments) at the smallest shapes at which it takes another path.  The method
is test_gpu_tile_refine.py's: one batch with the refinement on, with it off
and through k_tile_bound_ref; the results are bit-identical to each other and
to the oracle, the flags and work counters equal the reference kernel's, and
the flags with the refinement are a subset of the flags without it.

Full bands: a checkerboard of period 2 fails both bounds in every tile, so
every entry segment is full, the items are several times the workgroup and
cross every chunk boundary, and nothing drops out.  Full bands with gaps (see
test_full_bands_with_gaps): the same checkerboard in every other stripe of 80
columns of the default scene; every detector lists strictly fewer tiles with
the refinement than without and more than none, so the compaction closes gaps
in all three segments of a band at once.
Nearly empty bands: two 12 x 12 patches on blank frames; most bands have no
item, some one tile of one detector.  The clip: boxes whose snout_bottom
window ends on a block boundary and one column past it while the other
detectors end in earlier blocks, with last tile rows of three rows and of
one."""
import numpy as np
import pytest

import edge_scenes as E
from locomouse_cpp_amd import runtime as rt
from locomouse_cpp_amd import synthetic as S
from test_gpu_parity import _oracle
from test_gpu_tile_bound import _state
from test_gpu_tile_refine import MODES, _check, _fewer

pytestmark = pytest.mark.gpu


def _three(cfg, frames, monkeypatch, label):
    """One batch per mode; the counters with the refinement on and off, and every mode's flags."""
    n = len(frames)
    out = {}
    for mode, refine, ref in MODES:
        monkeypatch.setenv("LM_TILE_REFINE", refine)
        monkeypatch.setenv("LM_TILE_BOUND_REF", ref)
        ctx = rt.Context(cfg, max_batch=n)
        got = ctx.detect(frames, 0)
        out[mode] = (got, _state(ctx, n))
        ctx.close()
    return _check(out, _oracle(cfg, frames).result, label), out


def _full(pw, tw):
    return pw["listed"] == pw["bright"] and min(pw["bright"]) > 0 and tw["listed"] == tw["total"] and min(tw["total"]) > 0


def test_full_bands(monkeypatch):
    """Period 2: every bright point tile and every tail tile is listed, on and off."""
    cfg = S.SyntheticConfig()
    (pw, tw, pw0, tw0), _ = _three(cfg, E.checker_frames(cfg, 2, period=2), monkeypatch, "checker 2: ")
    assert _full(pw, tw) and _full(pw0, tw0), (pw, tw, pw0, tw0)


def test_full_bands_with_gaps(monkeypatch):
    """Every detector lists strictly fewer tiles with the refinement than
    without it, and more than none.  No period of the checkerboard alone does
    that: its 2 % of noise pixels keep every bright point tile listed at every
    period (measured on the GPU, two frames, listed with the refinement on /
    off: periods 2 to 96 point (700, 700, 460, 460) and tail (420, 276) both
    ways; 176 to 4096 the point detectors still all of their 688 - 697 and 446
    - 457 bright tiles both ways, only the tail detectors 418 - 420 and 273 -
    276 of (420, 276)).  The scene is therefore the period-2 checkerboard in
    every other stripe of 80 columns (two tile columns) of the default scene's
    frames 20 and 21: point (596, 594, 376, 376) of (612, 608, 395, 395), tail
    (350, 230) of (420, 242)."""
    cfg = S.SyntheticConfig()
    stripes = (np.arange(cfg.cols)[None, None, :] // 80) % 2 == 0
    frames = np.ascontiguousarray(np.where(stripes, E.checker_frames(cfg, 2, period=2), cfg.frames(20, 2)).astype(np.uint8))
    (pw, tw, pw0, tw0), _ = _three(cfg, frames, monkeypatch, "checker stripes: ")
    assert _fewer(pw, tw, pw0, tw0) and min(pw["listed"]) > 0 and min(tw["listed"]) > 0, (pw, tw, pw0, tw0)


def test_full_bands_one_detector_without_a_bound(monkeypatch):
    """paw_side with bias 0 (no bound): its segment bypasses the pass while
    the other two of its view are full."""
    cfg = S.SyntheticConfig(biases={"paw_side": 0.0})
    (pw, tw, pw0, tw0), _ = _three(cfg, E.checker_frames(cfg, 2, period=2), monkeypatch, "checker 2, bias 0: ")
    assert pw["listed"][2] == pw["bright"][2] == pw0["listed"][2] > 0, (pw, pw0)
    assert _full(pw, tw) and _full(pw0, tw0), (pw, tw, pw0, tw0)


def test_nearly_empty_bands(monkeypatch):
    """Blank frames with one bright 12 x 12 patch inside each box: at least
    one tile is listed and fewer than 2 % of all tiles (of the six detectors'
    grids over the three frames)."""
    cfg = S.SyntheticConfig()
    p = cfg.params
    frames = np.stack([E.blank(cfg)] * 3)
    bot, side = p.bounding_box_bottom, p.bounding_box_side
    for k, f in enumerate(frames):  # (in a corner of its box, where the box cuts the detectors' reach; a pixel further per frame)
        f[bot.y + 2:bot.y + 14, bot.x + 2 + k:bot.x + 14 + k] = 255
        f[side.y + side.height - 14:side.y + side.height - 2, side.x + side.width - 14 - k:side.x + side.width - 2 - k] = 255
    (pw, tw, pw0, tw0), out = _three(cfg, frames, monkeypatch, "patches: ")
    _, _, pt, tt = out["on"][1]
    listed = sum(pw["listed"]) + sum(tw["listed"])
    tiles = sum(x.size for x in pt) + sum(x.size for x in tt)
    assert listed == sum(int((x != 0).sum()) for x in pt + tt), (pw, tw)
    assert 1 <= listed < 0.02 * tiles, (listed, tiles, pw, tw)


def test_clip(monkeypatch):
    """Bottom 395 x 139, side 396 x 89: snout_bottom's window (in_x 0, kw 30)
    ends on a block boundary (395 + 29 = 424), snout_side's one column past
    it, the other detectors of each view in earlier blocks; last tile rows of
    three rows and of one (the level over fewer than four rows)."""
    cfg = S.SyntheticConfig(bounding_boxes={"side": (300, 3, 396, 89), "bottom": (300, 106, 395, 139)})
    (pw, tw, pw0, tw0), _ = _three(cfg, cfg.frames(40, 3), monkeypatch, "clip: ")
    assert _fewer(pw, tw, pw0, tw0), (pw, pw0, tw, tw0)


def test_odd_detectors(monkeypatch):
    """Two to ten tap groups (one to three chunks of constants per row) and a
    halo taller than a band."""
    cfg = E.odd_size_config()
    (pw, tw, pw0, tw0), _ = _three(cfg, cfg.frames(10, 2), monkeypatch, "odd detectors: ")
    assert sum(pw["listed"]) + sum(tw["listed"]) < sum(pw0["listed"]) + sum(tw0["listed"]), (pw, pw0, tw, tw0)


def test_c5(monkeypatch):
    c5 = S.SyntheticConfig(rows=512, cols=1920)
    (pw, tw, pw0, tw0), _ = _three(c5, c5.frames(10, 1), monkeypatch, "C5: ")
    assert sum(pw["listed"]) + sum(tw["listed"]) < sum(pw0["listed"]) + sum(tw0["listed"]), (pw, pw0, tw, tw0)
