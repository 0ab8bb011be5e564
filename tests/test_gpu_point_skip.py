"""GPU parity of the point-tile skip: the point detectors' bright 40 x 4 tiles
that k_tile_bound proves non-positive (csrc/lm_tail_bound.h) are not computed.
The results must not depend on it: LM_CORR_POINTSKIP on and off against the
oracle bit for bit, through the per-width and the merged ring launches, fused
and unfused arithmetic, flipped frames, odd boxes, blank frames, a
non-positive bias, point detectors on k_corr_gen (a non-ring width, one row),
C5, two pipeline lanes and LM_CORR_DARK=0; and the listed tiles must be bright
tiles and cover every bright tile in which the oracle has a positive score."""
import numpy as np
import pytest

import edge_scenes as E
from locomouse_cpp_amd import runtime as rt
from locomouse_cpp_amd import synthetic as S
from locomouse_cpp_amd.results import concat_results
from test_gpu_parity import _oracle, assert_same
from test_gpu_tail_skip import _default_ref, _plan, _positive_tiles
from test_tail_bound import _normalised

pytestmark = pytest.mark.gpu

POINT_DETS = (0, 1, 3, 4)  # lm_debug_scores ids in lm_debug_point_work's order: paw_b, snout_b, paw_s, snout_s


def _bright_map(cfg, frame, view):
    """[tile rows, tile columns] bool: some I_*_MOUSE pixel of the 40 x 4 tile
    is > 25 (identity calibration, provided boxes, no flip; the mouse crop
    starts one pixel right of and below the box corner)."""
    tw, th = rt.Context.dark_tile_shape()
    r = cfg.params.bounding_box_side if view else cfg.params.bounding_box_bottom
    crop = _normalised(cfg, frame)[r.y + 1:r.y + 1 + r.height, r.x + 1:r.x + 1 + r.width] > 25
    pad = np.zeros((-(-r.height // th) * th, -(-r.width // tw) * tw), bool)
    pad[:r.height, :r.width] = crop
    return pad.reshape(pad.shape[0] // th, th, pad.shape[1] // tw, tw).any(axis=(1, 3))


def _check_cover(ctx, cfg, frames, ref):
    """Listed tiles are bright tiles and cover the oracle's positive bright
    tiles; the counters equal the sums of the flags and of the bright tiles."""
    work = ctx.point_work()
    listed, bright = [0] * 4, [0] * 4
    for f, frame in enumerate(frames):
        for k, det in enumerate(POINT_DETS):
            fl = ctx.point_tiles(f, det)
            br = _bright_map(cfg, frame, det >= 3)
            truth = _positive_tiles(ref.scores(f, det)) & br
            assert fl.shape == br.shape == truth.shape
            assert not ((fl != 0) & ~br).any(), (f, det, np.argwhere((fl != 0) & ~br)[:4])
            assert not (truth & (fl == 0)).any(), (f, det, np.argwhere(truth & (fl == 0))[:4])
            listed[k] += int(fl.sum())
            bright[k] += int(br.sum())
    assert work == {"listed": tuple(listed), "bright": tuple(bright)}, (work, listed, bright)
    return work


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("unfused", [False, True])
@pytest.mark.parametrize("plan", [0, 1])
def test_skip_on_and_off_match_the_oracle(plan, unfused, flip, monkeypatch):
    """C3, 4 frames: every result array bit-identical to the oracle's with the
    skip on and off (direct launches with debug maps, and with the skip on
    also through the captured graphs)."""
    cfg, frames, ref = _default_ref(unfused, flip)
    for skip, debug in (("1", 1), ("0", 1), ("1", 0)):
        monkeypatch.setenv("LM_CORR_POINTSKIP", skip)
        ctx = rt.Context(cfg, max_batch=4)
        ctx.set_debug(debug | _plan(plan))
        got = ctx.detect(frames, 0)
        assert_same(got, ref.result, f"pointskip={skip} debug={debug} plan {plan} unfused {unfused} flip {flip}: ")
        work = ctx.point_work()
        ctx.close()
        if skip == "1":
            assert all(0 < a < b for a, b in zip(work["listed"], work["bright"])), work
        else:
            assert work is None


def test_listed_tiles_cover_the_positive_scores():
    cfg, frames, ref = _default_ref(False, False)
    ctx = rt.Context(cfg, max_batch=4)
    ctx.set_debug(1)
    ctx.detect(frames, 0)
    work = _check_cover(ctx, cfg, frames, ref)
    tails = ctx.tail_work()
    ctx.close()
    assert all(0 < a < b for a, b in zip(work["listed"], work["bright"])), work  # the default scene: flat body tiles proven
    assert tails["total"] == (4 * 35 * 6, 4 * 23 * 6) and all(a < b for a, b in zip(tails["listed"], tails["total"])), tails


@pytest.mark.parametrize("plan", [0, 1])
def test_odd_boxes(plan):
    """Boxes with oh % 4 != 0 and ow % 40 != 0 (bottom 397 x 139, side 397 x
    89): partial tiles on both edges."""
    from oracle import oracle as O
    cfg = S.SyntheticConfig(bounding_boxes={"side": (300, 3, 397, 89), "bottom": (300, 106, 397, 139)})
    frames = cfg.frames(40, 3)
    ref = _oracle(cfg, frames, flags=O.KEEP_DEBUG)
    ctx = rt.Context(cfg, max_batch=3)
    ctx.set_debug(1 | _plan(plan))
    assert_same(ctx.detect(frames, 0), ref.result, f"odd boxes plan {plan}: ")
    work = _check_cover(ctx, cfg, frames, ref)
    ctx.close()
    assert all(0 < a < b for a, b in zip(work["listed"], work["bright"])), work


def test_blank_frames():
    """Nothing is bright and nothing is listed."""
    cfg = S.SyntheticConfig()
    frames = np.stack([E.blank(cfg)] * 3)
    ctx = rt.Context(cfg, max_batch=3)
    assert_same(ctx.detect(frames, 0), _oracle(cfg, frames).result, "blank: ")
    work = ctx.point_work()
    ctx.close()
    assert work == {"listed": (0, 0, 0, 0), "bright": (0, 0, 0, 0)}, work


def test_non_positive_bias():
    """paw_side with bias 0 (delta = -bias >= 0): the bound never applies to
    it, every bright tile of it is listed; the other detectors still skip."""
    from oracle import oracle as O
    cfg = S.SyntheticConfig(biases={"paw_side": 0.0})
    frames = cfg.frames(12, 3)
    ref = _oracle(cfg, frames, flags=O.KEEP_DEBUG)
    ctx = rt.Context(cfg, max_batch=3)
    ctx.set_debug(1)
    assert_same(ctx.detect(frames, 0), ref.result, "bias 0: ")
    work = _check_cover(ctx, cfg, frames, ref)
    ctx.close()
    assert work["listed"][2] == work["bright"][2] > 0, work
    assert all(0 < work["listed"][k] < work["bright"][k] for k in (0, 1, 3)), work


def test_point_detectors_on_the_generic_kernel():
    """paw_bottom 24 x 34 (a width without a ring instantiation) and
    snout_side of one row (1 x 26): both run on k_corr_gen, whose workgroups
    return when none of their tiles is listed."""
    from oracle import oracle as O
    w = {"paw_bottom": S.dog_detector(24, 34, 6.0, 81), "snout_side": S.dog_detector(1, 26, 5.0, 82)}
    base = S.SyntheticConfig(weights=w)
    cfg = S.SyntheticConfig(weights=w, biases=E._bias_for_rate(base, ["paw_bottom", "snout_side"]))
    assert cfg.biases["paw_bottom"] > 0 and cfg.biases["snout_side"] > 0
    frames = cfg.frames(10, 3)
    ref = _oracle(cfg, frames, flags=O.KEEP_DEBUG)
    ctx = rt.Context(cfg, max_batch=3)
    ctx.set_debug(1)
    assert_same(ctx.detect(frames, 0), ref.result, "point detectors on k_corr_gen: ")
    work = _check_cover(ctx, cfg, frames, ref)
    ctx.close()
    assert all(0 < a <= b for a, b in zip(work["listed"], work["bright"])), work
    assert work["listed"][0] < work["bright"][0], work


def test_c5():
    """C5 (1920 x 512, point detectors 44 to 60 wide), 2 frames."""
    c5 = S.SyntheticConfig(rows=512, cols=1920)
    frames = c5.frames(10, 2)
    ctx = rt.Context(c5, max_batch=2)
    assert_same(ctx.detect(frames, 0), _oracle(c5, frames).result, "C5: ")
    work = ctx.point_work()
    ctx.close()
    assert all(0 < a < b for a, b in zip(work["listed"], work["bright"])), work


def test_two_lanes_with_different_batch_sizes():
    """Batches of 5, 3, 4, 5 and 2 frames through two pipeline lanes (each
    lane with its own lists, counters and captured graphs per batch shape)."""
    cfg = S.SyntheticConfig()
    sizes = (5, 3, 4, 5, 2)
    frames = cfg.frames(0, sum(sizes))
    ctx = rt.Context(cfg, max_batch=5, lanes=2)
    parts, first = [], 0
    for n in sizes:
        if ctx.pending() == 2:
            parts.append(ctx.collect())
        ctx.submit(frames[first:first + n], first)
        first += n
    while ctx.pending():
        parts.append(ctx.collect())
    ctx.close()
    assert_same(concat_results(parts), _oracle(cfg, frames).result, "two lanes: ")


def test_dark_tiles_off_turns_the_skip_off(monkeypatch):
    """LM_CORR_DARK=0: no bright flags, so no point skip; results equal."""
    cfg, frames, ref = _default_ref(False, False)
    monkeypatch.setenv("LM_CORR_DARK", "0")
    ctx = rt.Context(cfg, max_batch=4)
    assert_same(ctx.detect(frames, 0), ref.result, "LM_CORR_DARK=0: ")
    assert ctx.point_work() is None
    ctx.close()
