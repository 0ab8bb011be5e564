"""GPU parity of the tail-tile skip: the tail detectors' 40 x 4 tiles that
k_tail_bound proves non-positive (csrc/lm_tail_bound.h) are not computed.  The
results must not depend on it: LM_CORR_TAILSKIP on and off against the oracle
bit for bit, through the per-width and the merged ring launches, fused and
unfused arithmetic, flipped frames, odd tail boxes, blank frames, a negative
rho, a non-ring tail width (k_corr_gen), C5, and two pipeline lanes; and the
listed tiles must cover every tile in which the oracle has a positive score."""
import functools

import numpy as np
import pytest

import edge_scenes as E
from locomouse_cpp_amd import abi
from locomouse_cpp_amd import runtime as rt
from locomouse_cpp_amd import synthetic as S
from locomouse_cpp_amd.results import concat_results
from test_gpu_parity import _oracle, assert_same

pytestmark = pytest.mark.gpu


def _plan(plan):
    return abi.LM_DEBUG_PLAN_MERGED if plan else abi.LM_DEBUG_PLAN_PER_WIDTH


def _cfg(unfused=False, flip=False, **kw):
    cfg = S.SyntheticConfig(flip=flip, **kw)
    if unfused:
        cfg.setup.filter_arith = abi.LM_FILTER_UNFUSED
    return cfg


@functools.lru_cache(maxsize=None)
def _default_ref(unfused, flip):
    from oracle import oracle as O
    cfg = _cfg(unfused, flip)
    return cfg, cfg.frames(20, 4), _oracle(cfg, cfg.frames(20, 4), flags=O.KEEP_DEBUG)


def _positive_tiles(scores):
    """[tile rows, tile columns] bool: the 40 x 4 tile holds a positive score."""
    tw, th = rt.Context.dark_tile_shape()
    oh, ow = scores.shape
    pos = np.zeros((-(-oh // th) * th, -(-ow // tw) * tw), bool)
    pos[:oh, :ow] = scores > 0
    return pos.reshape(pos.shape[0] // th, th, pos.shape[1] // tw, tw).any(axis=(1, 3))


def _check_cover(ctx, ref, n, first=0):
    """Listed tiles cover the oracle's positive tiles; the counters agree with the flags."""
    work = ctx.tail_work()
    listed = [0, 0]
    for f in range(n):
        for view, det in ((0, 2), (1, 5)):
            fl = ctx.tail_tiles(f, view)
            truth = _positive_tiles(ref.scores(first + f, det))
            assert fl.shape == truth.shape
            assert not (truth & (fl == 0)).any(), (f, view, np.argwhere(truth & (fl == 0))[:4])
            listed[view] += int(fl.sum())
    assert work["listed"] == tuple(listed), (work, listed)
    assert all(a <= b for a, b in zip(work["listed"], work["total"])), work
    return work


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("unfused", [False, True])
@pytest.mark.parametrize("plan", [0, 1])
def test_skip_on_and_off_match_the_oracle(plan, unfused, flip, monkeypatch):
    """C3, 4 frames: every result array and TAIL_MASK bit-identical to the
    oracle's with the skip on and off (direct launches with debug maps, and
    with the skip on also through the captured graphs)."""
    cfg, frames, ref = _default_ref(unfused, flip)
    g = None
    for skip, debug in (("1", 1), ("0", 1), ("1", 0)):
        monkeypatch.setenv("LM_CORR_TAILSKIP", skip)
        ctx = rt.Context(cfg, max_batch=4)
        ctx.set_debug(debug | _plan(plan))
        got = ctx.detect(frames, 0)
        label = f"tailskip={skip} debug={debug} plan {plan} unfused {unfused} flip {flip}: "
        assert_same(got, ref.result, label)
        if debug:
            g = g or ctx.geometry()
            for f in range(4):
                assert np.array_equal(ctx.debug_tail_mask(f),
                                      ref.tail_mask(f, (g.bb_bottom_mouse.height, g.tail_box_width))), label + str(f)
        if skip == "1":
            work = ctx.tail_work()
            assert all(a < b for a, b in zip(work["listed"], work["total"])), work
            assert flip or min(work["listed"]) > 0, work  # (flipped, the tail box holds no tail)
        else:
            assert ctx.tail_work() is None
        ctx.close()


def test_listed_tiles_cover_the_positive_scores():
    cfg, frames, ref = _default_ref(False, False)
    ctx = rt.Context(cfg, max_batch=4)
    ctx.set_debug(1)
    ctx.detect(frames, 0)
    work = _check_cover(ctx, ref, 4)
    ctx.close()
    assert work["total"] == (4 * 35 * 6, 4 * 23 * 6)
    assert all(a < b for a, b in zip(work["listed"], work["total"])), work  # the default scene: most tiles proven


@pytest.mark.parametrize("plan", [0, 1])
def test_odd_tail_boxes(plan):
    """Boxes with oh % 4 != 0 and ow % 40 != 0 (bottom 397 x 139, side 397 x
    89: tail boxes 238 wide): partial tiles on both edges."""
    from oracle import oracle as O
    cfg = S.SyntheticConfig(bounding_boxes={"side": (300, 3, 397, 89), "bottom": (300, 106, 397, 139)})
    frames = cfg.frames(40, 3)
    ref = _oracle(cfg, frames, flags=O.KEEP_DEBUG)
    ctx = rt.Context(cfg, max_batch=3)
    ctx.set_debug(1 | _plan(plan))
    assert_same(ctx.detect(frames, 0), ref.result, f"odd boxes plan {plan}: ")
    g = ctx.geometry()
    assert g.tail_box_width % 40 and g.bb_bottom_mouse.height % 4 and g.bb_side_mouse.height % 4
    work = _check_cover(ctx, ref, 3)
    ctx.close()
    assert all(0 < a < b for a, b in zip(work["listed"], work["total"])), work


def test_blank_frames_and_negative_rho():
    """Blank frames: every tile proven (nothing listed), tail tracks -1.  A
    negative rho (positive delta): the bound never applies, every tile is
    listed, results equal to the oracle's."""
    cfg = S.SyntheticConfig()
    frames = np.stack([E.blank(cfg)] * 3)
    ref = _oracle(cfg, frames).result
    ctx = rt.Context(cfg, max_batch=3)
    got = ctx.detect(frames, 0)
    assert_same(got, ref, "blank: ")
    assert (got["tail"] == -1).all()
    work = ctx.tail_work()
    ctx.close()
    assert work["listed"] == (0, 0) and min(work["total"]) > 0, work
    dense = E.dense_tail_config()
    frames = dense.frames(0, 3)
    ctx = rt.Context(dense, max_batch=3)
    assert_same(ctx.detect(frames, 0), _oracle(dense, frames).result, "negative rho: ")
    work = ctx.tail_work()
    ctx.close()
    assert work["listed"] == work["total"], work


def test_tail_detectors_of_non_ring_widths():
    """16 x 34 and 9 x 33 tail detectors (no ring instantiation: k_corr_gen,
    whose workgroups return when none of their tail tiles is listed)."""
    from oracle import oracle as O
    w = {"tail_bottom": S.line_detector(16, 34, 1.5, 71), "tail_side": S.line_detector(9, 33, 1.5, 72)}
    cfg = S.SyntheticConfig(weights=w)
    frames = cfg.frames(10, 3)
    ref = _oracle(cfg, frames, flags=O.KEEP_DEBUG)
    assert (ref.result["tail"][:, 0] >= 0).any()
    ctx = rt.Context(cfg, max_batch=3)
    ctx.set_debug(1)
    assert_same(ctx.detect(frames, 0), ref.result, "non-ring tail widths: ")
    work = _check_cover(ctx, ref, 3)
    ctx.close()
    assert all(0 < a < b for a, b in zip(work["listed"], work["total"])), work


def test_c5():
    """C5 (1920 x 512, tail detectors 32 x 52: a ring width), 2 frames."""
    c5 = S.SyntheticConfig(rows=512, cols=1920)
    frames = c5.frames(10, 2)
    ctx = rt.Context(c5, max_batch=2)
    assert_same(ctx.detect(frames, 0), _oracle(c5, frames).result, "C5: ")
    work = ctx.tail_work()
    ctx.close()
    assert all(0 < a < b for a, b in zip(work["listed"], work["total"])), work


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
