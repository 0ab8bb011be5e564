"""k_tile_bound (bands of tile rows, from k_ingest's block ranges) against
k_tile_bound_ref (LM_TILE_BOUND_REF=1: one workgroup per slot and view, from
the crops): the flags of every frame and detector and the work counters must
be equal, and the results of the new path bit-identical to the oracle's.  The
cases are the smallest shapes at which the banded kernel takes another path:
partial tiles on both edges and a short last tile row, fewer tile rows than a
band, a detector taller than a band (halo rows > band rows), three ingest
groups with several slots and bands on one list segment, two lanes, C5, blank
frames, a detector without a bound, each skip alone (null counters), and the
modes without any skip (no block ranges are written)."""
import numpy as np
import pytest

import edge_scenes as E
from locomouse_cpp_amd import abi
from locomouse_cpp_amd import runtime as rt
from locomouse_cpp_amd import synthetic as S
from test_gpu_parity import _oracle, assert_same
from test_gpu_tail_skip import _plan

pytestmark = pytest.mark.gpu

POINT_DETS = (0, 1, 3, 4)


def _state(ctx, n):
    """The flags of the delivered batch's n frames and the work counters."""
    pw, tw = ctx.point_work(), ctx.tail_work()
    pt = [ctx.point_tiles(f, d) for f in range(n) for d in POINT_DETS] if pw is not None else None
    tt = [ctx.tail_tiles(f, v) for f in range(n) for v in (0, 1)] if tw is not None else None
    return pw, tw, pt, tt


def _assert_state_equal(new, ref, label):
    (pw, tw, pt, tt), (rpw, rtw, rpt, rtt) = new, ref
    assert pw == rpw, (label, pw, rpw)
    assert tw == rtw, (label, tw, rtw)
    for name, a, b in (("point", pt, rpt), ("tail", tt, rtt)):
        assert (a is None) == (b is None), label
        for i, (x, y) in enumerate(zip(a or [], b or [])):
            assert x.shape == y.shape and np.array_equal(x, y), (label, name, i, np.argwhere(x != y)[:4])


def _both(cfg, frames, monkeypatch, label, debug=0, oracle=True):
    """One batch through a context of the new path and one of the reference
    kernel: equal flags and counters, equal results; the new path's results
    against the oracle.  Returns the new path's counters."""
    n = len(frames)
    out = {}
    for ref in ("0", "1"):
        monkeypatch.setenv("LM_TILE_BOUND_REF", ref)
        ctx = rt.Context(cfg, max_batch=n)
        if debug:
            ctx.set_debug(debug)
        got = ctx.detect(frames, 0)
        out[ref] = (got, _state(ctx, n))
        ctx.close()
    _assert_state_equal(out["0"][1], out["1"][1], label)
    assert_same(out["0"][0], out["1"][0], label + "new against reference kernel: ")
    if oracle:
        assert_same(out["0"][0], _oracle(cfg, frames).result, label)
    return out["0"][1][0], out["0"][1][1]


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("plan", [0, 1])
def test_default_c3(plan, flip, monkeypatch):
    cfg = S.SyntheticConfig(flip=flip)
    pw, tw = _both(cfg, cfg.frames(20, 4), monkeypatch, f"C3 plan {plan} flip {flip}: ", debug=_plan(plan))
    assert all(0 < a < b for a, b in zip(pw["listed"], pw["bright"])), pw
    assert all(a < b for a, b in zip(tw["listed"], tw["total"])), tw


def test_odd_boxes(monkeypatch):
    """Bottom 397 x 139, side 397 x 89: partial tiles on both edges, a last
    tile row of three (bottom) and one (side) output rows, and tile-row counts
    (35, 23) that are no multiple of the band."""
    cfg = S.SyntheticConfig(bounding_boxes={"side": (300, 3, 397, 89), "bottom": (300, 106, 397, 139)})
    pw, tw = _both(cfg, cfg.frames(40, 3), monkeypatch, "odd boxes: ")
    assert all(0 < a < b for a, b in zip(pw["listed"], pw["bright"])), pw
    assert all(0 < a < b for a, b in zip(tw["listed"], tw["total"])), tw


def test_box_of_fewer_tile_rows_than_a_band(monkeypatch):
    """A 400 x 20 bottom box: five tile rows, one band."""
    cfg = S.SyntheticConfig(bounding_boxes={"side": (300, 3, 400, 90), "bottom": (300, 166, 400, 20)})
    pw, tw = _both(cfg, cfg.frames(20, 3), monkeypatch, "400 x 20 bottom box: ")
    assert min(pw["bright"]) > 0, pw


def test_detector_taller_than_a_band(monkeypatch):
    """snout_bottom 70 x 70: its window's halo (69 rows) exceeds the band's
    output rows; paw_side 13 x 13 and tail_side 9 x 33 next to it."""
    cfg = E.odd_size_config()
    pw, tw = _both(cfg, cfg.frames(10, 3), monkeypatch, "70-row detector: ")
    assert all(0 < a <= b for a, b in zip(pw["listed"], pw["bright"])), pw


def test_seventeen_frames(monkeypatch):
    """Three ingest groups of 8, 8 and 1 slots: several slots and bands append
    to one list segment."""
    cfg = S.SyntheticConfig()
    pw, tw = _both(cfg, cfg.frames(0, 17), monkeypatch, "17 frames: ")
    assert all(0 < a < b for a, b in zip(pw["listed"], pw["bright"])), pw


def test_two_lanes(monkeypatch):
    """Batches of 5, 3 and 4 frames through two pipeline lanes."""
    cfg = S.SyntheticConfig()
    sizes = (5, 3, 4)
    frames = cfg.frames(0, sum(sizes))
    states = {}
    for ref in ("0", "1"):
        monkeypatch.setenv("LM_TILE_BOUND_REF", ref)
        ctx = rt.Context(cfg, max_batch=5, lanes=2)
        parts, st, first, coll = [], [], 0, 0

        def collect():
            nonlocal coll
            parts.append(ctx.collect())
            st.append(_state(ctx, sizes[coll]))
            coll += 1

        for n in sizes:
            if ctx.pending() == 2:
                collect()
            ctx.submit(frames[first:first + n], first)
            first += n
        while ctx.pending():
            collect()
        ctx.close()
        states[ref] = (parts, st)
    from locomouse_cpp_amd.results import concat_results
    for i, (a, b) in enumerate(zip(states["0"][1], states["1"][1])):
        _assert_state_equal(a, b, f"two lanes, batch {i}: ")
    assert_same(concat_results(states["0"][0]), _oracle(cfg, frames).result, "two lanes: ")


def test_c5(monkeypatch):
    c5 = S.SyntheticConfig(rows=512, cols=1920)
    pw, tw = _both(c5, c5.frames(10, 2), monkeypatch, "C5: ")
    assert all(0 < a < b for a, b in zip(pw["listed"], pw["bright"])), pw
    assert all(0 < a < b for a, b in zip(tw["listed"], tw["total"])), tw


def test_blank_frames(monkeypatch):
    """Nothing bright, nothing listed, no stray range."""
    cfg = S.SyntheticConfig()
    pw, tw = _both(cfg, np.stack([E.blank(cfg)] * 3), monkeypatch, "blank: ")
    assert pw == {"listed": (0, 0, 0, 0), "bright": (0, 0, 0, 0)}, pw
    assert tw["listed"] == (0, 0), tw


def test_detector_without_a_bound(monkeypatch):
    """paw_side with bias 0 (tb_skip = 0): every bright tile of it is listed."""
    cfg = S.SyntheticConfig(biases={"paw_side": 0.0})
    pw, tw = _both(cfg, cfg.frames(12, 3), monkeypatch, "bias 0: ")
    assert pw["listed"][2] == pw["bright"][2] > 0, pw
    assert all(0 < pw["listed"][k] < pw["bright"][k] for k in (0, 1, 3)), pw


@pytest.mark.parametrize("off", ["LM_CORR_TAILSKIP", "LM_CORR_POINTSKIP"])
def test_one_skip_alone(off, monkeypatch):
    """The other skip's counters are null; the block ranges are still written."""
    monkeypatch.setenv(off, "0")
    cfg = S.SyntheticConfig()
    pw, tw = _both(cfg, cfg.frames(20, 4), monkeypatch, off + "=0: ")
    if off == "LM_CORR_TAILSKIP":
        assert tw is None and all(0 < a < b for a, b in zip(pw["listed"], pw["bright"])), (pw, tw)
    else:
        assert pw is None and all(0 < a < b for a, b in zip(tw["listed"], tw["total"])), (pw, tw)


def test_no_skip_at_all(monkeypatch):
    """LM_CORR_DARK=0 with LM_CORR_TAILSKIP=0, and the f16 mode: no pre-pass,
    no block ranges (the pointer is null), results equal."""
    cfg = S.SyntheticConfig()
    frames = cfg.frames(20, 4)
    monkeypatch.setenv("LM_CORR_DARK", "0")
    pw, tw = _both(cfg, frames, monkeypatch, "LM_CORR_DARK=0: ")  # (the tail skip stays on)
    assert pw is None and tw is not None
    monkeypatch.setenv("LM_CORR_TAILSKIP", "0")
    pw, tw = _both(cfg, frames, monkeypatch, "LM_CORR_DARK=0 LM_CORR_TAILSKIP=0: ")
    assert pw is None and tw is None
    monkeypatch.delenv("LM_CORR_DARK")
    monkeypatch.delenv("LM_CORR_TAILSKIP")
    f16 = S.SyntheticConfig()
    f16.setup.corr_precision = abi.LM_CORR_F16
    pw, tw = _both(f16, frames, monkeypatch, "f16: ", oracle=False)  # (a non-parity mode: new against reference only)
    assert pw is None and tw is None
