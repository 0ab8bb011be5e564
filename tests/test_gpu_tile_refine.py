"""The refinement of the tile bound on the GPU (LM_TILE_REFINE, default 1: the
tiles the tile bound fails are tried per 8-column output block and group of 8
taps, csrc/lm_tail_bound.h).  Every case runs one batch with the refinement on
and off and once more through k_tile_bound_ref (LM_TILE_BOUND_REF=1) with it
on: the results must be bit-identical to each other and to the oracle, the
flags with the refinement a subset of the flags without it, and the flags and
work counters of k_tile_bound equal to the reference kernel's.  The cases are
the smallest shapes at which the refinement takes another path: a last tile
column of 37 outputs (a block of 5), last tile rows of 3 and 1 rows, detectors
of 9 to 70 taps per row (2 to 10 tap groups; a window starts max kw' / 2 -
kw / 2 columns into its view's crop, whatever the box's origin: in_x mod 8 is
0, 2 and 3 in C3, 4 and 6 in C5, 7 with a 70-wide detector, 1 and 5 with
widths 28 and 20 next to 30), a halo taller than a band, three ingest groups,
two lanes, the unfused arithmetic, a detector without a bound, blank frames
and each skip alone."""
import numpy as np
import pytest

import edge_scenes as E
from locomouse_cpp_amd import abi
from locomouse_cpp_amd import runtime as rt
from locomouse_cpp_amd import synthetic as S
from locomouse_cpp_amd.results import concat_results
from test_gpu_parity import _oracle, assert_same
from test_gpu_tail_skip import _plan
from test_gpu_tile_bound import _assert_state_equal, _state

pytestmark = pytest.mark.gpu

MODES = (("on", "1", "0"), ("off", "0", "0"), ("ref", "1", "1"))  # (name, LM_TILE_REFINE, LM_TILE_BOUND_REF)


def _assert_subset(on, off, label):
    """Every tile flagged with the refinement is flagged without it."""
    for name, a, b in (("point", on[2], off[2]), ("tail", on[3], off[3])):
        assert (a is None) == (b is None), label
        for i, (x, y) in enumerate(zip(a or [], b or [])):
            assert x.shape == y.shape and not ((x != 0) & (y == 0)).any(), (label, name, i, np.argwhere((x != 0) & (y == 0))[:4])


def _check(out, ref_result, label):
    print(label, {m: (out[m][1][0], out[m][1][1]) for m in out})
    assert_same(out["on"][0], out["off"][0], label + "refinement on against off: ")
    assert_same(out["on"][0], out["ref"][0], label + "new against reference kernel: ")
    if ref_result is not None:
        assert_same(out["on"][0], ref_result, label)
    _assert_subset(out["on"][1], out["off"][1], label)
    _assert_state_equal(out["on"][1], out["ref"][1], label)
    (pw, tw, _, _), (pw0, tw0, _, _) = out["on"][1], out["off"][1]
    if pw is not None:
        assert pw["bright"] == pw0["bright"] and all(a <= b for a, b in zip(pw["listed"], pw0["listed"])), (label, pw, pw0)
    if tw is not None:
        assert tw["total"] == tw0["total"] and all(a <= b for a, b in zip(tw["listed"], tw0["listed"])), (label, tw, tw0)
    return pw, tw, pw0, tw0


def _three(cfg, frames, monkeypatch, label, debug=0, oracle=True):
    """One batch per mode; returns the counters with the refinement on and off."""
    n = len(frames)
    out = {}
    for mode, refine, ref in MODES:
        monkeypatch.setenv("LM_TILE_REFINE", refine)
        monkeypatch.setenv("LM_TILE_BOUND_REF", ref)
        ctx = rt.Context(cfg, max_batch=n)
        if debug:
            ctx.set_debug(debug)
        got = ctx.detect(frames, 0)
        out[mode] = (got, _state(ctx, n))
        ctx.close()
    return _check(out, _oracle(cfg, frames).result if oracle else None, label)


def _fewer(pw, tw, pw0, tw0):
    return (all(a < b for a, b in zip(pw["listed"], pw0["listed"])) and
            all(a < b for a, b in zip(tw["listed"], tw0["listed"])))


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("plan", [0, 1])
def test_default_c3(plan, flip, monkeypatch):
    """Every one of the six detectors lists strictly fewer tiles."""
    cfg = S.SyntheticConfig(flip=flip)
    pw, tw, pw0, tw0 = _three(cfg, cfg.frames(20, 4), monkeypatch, f"C3 plan {plan} flip {flip}: ", debug=_plan(plan))
    assert _fewer(pw, tw, pw0, tw0), (pw, pw0, tw, tw0)


def test_odd_boxes(monkeypatch):
    """Bottom 397 x 139, side 397 x 89: a last tile column of 37 outputs (five
    blocks, the last of 5), last tile rows of three rows and of one."""
    cfg = S.SyntheticConfig(bounding_boxes={"side": (300, 3, 397, 89), "bottom": (300, 106, 397, 139)})
    pw, tw, pw0, tw0 = _three(cfg, cfg.frames(40, 3), monkeypatch, "odd boxes: ")
    assert _fewer(pw, tw, pw0, tw0), (pw, pw0, tw, tw0)


@pytest.mark.parametrize("x", [303, 306])
def test_box_origins(x, monkeypatch):
    """Boxes moved by 3 and 6 columns: other pixels under every aligned block."""
    cfg = S.SyntheticConfig(bounding_boxes={"side": (x, 3, 400, 90), "bottom": (x, 106, 400, 140)})
    pw, tw, pw0, tw0 = _three(cfg, cfg.frames(30, 2), monkeypatch, f"box origin {x}: ")
    assert _fewer(pw, tw, pw0, tw0), (pw, pw0, tw, tw0)


def test_odd_detectors(monkeypatch):
    """70 x 70, 13 x 13 and 9 x 33 detectors: ten, two and five tap groups with
    partial first and last ones, and a halo (69 rows) taller than a band."""
    cfg = E.odd_size_config()
    pw, tw, pw0, tw0 = _three(cfg, cfg.frames(10, 3), monkeypatch, "odd detectors: ")
    assert sum(pw["listed"]) + sum(tw["listed"]) < sum(pw0["listed"]) + sum(tw0["listed"]), (pw, pw0, tw, tw0)


def test_other_residues(monkeypatch):
    """paw_bottom 24 x 28 and tail_bottom 16 x 20 next to snout_bottom 30 x 30:
    their windows start 1 and 5 columns into the crop, so the first tap group
    has 7 and 3 taps (both run on k_corr_gen: no ring of these widths)."""
    w = {"paw_bottom": S.dog_detector(24, 28, 6.0, 83), "tail_bottom": S.line_detector(16, 20, 1.5, 84)}
    base = S.SyntheticConfig(weights=w)
    cfg = S.SyntheticConfig(weights=w, biases=E._bias_for_rate(base, ["paw_bottom"]))
    pw, tw, pw0, tw0 = _three(cfg, cfg.frames(10, 2), monkeypatch, "in_x mod 8 of 1 and 5: ")
    assert pw["listed"][0] < pw0["listed"][0] and tw["listed"][0] < tw0["listed"][0], (pw, pw0, tw, tw0)


def test_seventeen_frames(monkeypatch):
    """Three ingest groups of 8, 8 and 1 slots on shared list segments."""
    cfg = S.SyntheticConfig()
    pw, tw, pw0, tw0 = _three(cfg, cfg.frames(0, 17), monkeypatch, "17 frames: ")
    assert _fewer(pw, tw, pw0, tw0), (pw, pw0, tw, tw0)


def test_two_lanes(monkeypatch):
    """Batches of 5, 3 and 4 frames through two pipeline lanes."""
    cfg = S.SyntheticConfig()
    sizes = (5, 3, 4)
    frames = cfg.frames(0, sum(sizes))
    runs = {}
    for mode, refine, ref in MODES:
        monkeypatch.setenv("LM_TILE_REFINE", refine)
        monkeypatch.setenv("LM_TILE_BOUND_REF", ref)
        ctx = rt.Context(cfg, max_batch=5, lanes=2)
        parts, st, first = [], [], 0
        for n in sizes:
            if ctx.pending() == 2:
                parts.append(ctx.collect())
                st.append(_state(ctx, sizes[len(st)]))
            ctx.submit(frames[first:first + n], first)
            first += n
        while ctx.pending():
            parts.append(ctx.collect())
            st.append(_state(ctx, sizes[len(st)]))
        ctx.close()
        runs[mode] = (parts, st)
    oracle = _oracle(cfg, frames).result
    assert_same(concat_results(runs["on"][0]), oracle, "two lanes: ")
    for i in range(len(sizes)):
        out = {m: (runs[m][0][i], runs[m][1][i]) for m in runs}
        pw, tw, pw0, tw0 = _check(out, None, f"two lanes, batch {i}: ")
        assert _fewer(pw, tw, pw0, tw0), (i, pw, pw0, tw, tw0)


def test_c5(monkeypatch):
    c5 = S.SyntheticConfig(rows=512, cols=1920)
    pw, tw, pw0, tw0 = _three(c5, c5.frames(10, 2), monkeypatch, "C5: ")
    assert _fewer(pw, tw, pw0, tw0), (pw, pw0, tw, tw0)


def test_unfused_arithmetic(monkeypatch):
    cfg = S.SyntheticConfig()
    cfg.setup.filter_arith = abi.LM_FILTER_UNFUSED
    pw, tw, pw0, tw0 = _three(cfg, cfg.frames(20, 2), monkeypatch, "unfused: ")
    assert _fewer(pw, tw, pw0, tw0), (pw, pw0, tw, tw0)


def test_detector_without_a_bound(monkeypatch):
    """paw_side with bias 0 (rho <= 0: tb_skip = 0): every bright tile of it
    is listed, the other detectors are refined."""
    cfg = S.SyntheticConfig(biases={"paw_side": 0.0})
    pw, tw, pw0, tw0 = _three(cfg, cfg.frames(12, 3), monkeypatch, "bias 0: ")
    assert pw["listed"][2] == pw["bright"][2] == pw0["listed"][2] > 0, (pw, pw0)
    assert all(0 < pw["listed"][k] < pw0["listed"][k] for k in (0, 1, 3)), (pw, pw0)
    assert all(a < b for a, b in zip(tw["listed"], tw0["listed"])), (tw, tw0)


def test_blank_frames(monkeypatch):
    """Nothing is listed, with or without the refinement."""
    cfg = S.SyntheticConfig()
    pw, tw, pw0, tw0 = _three(cfg, np.stack([E.blank(cfg)] * 3), monkeypatch, "blank: ")
    assert pw == pw0 == {"listed": (0, 0, 0, 0), "bright": (0, 0, 0, 0)}, (pw, pw0)
    assert tw["listed"] == tw0["listed"] == (0, 0), (tw, tw0)


@pytest.mark.parametrize("off", ["LM_CORR_TAILSKIP", "LM_CORR_POINTSKIP"])
def test_one_skip_alone(off, monkeypatch):
    """The refinement is off with the skip it belongs to and on for the other."""
    monkeypatch.setenv(off, "0")
    cfg = S.SyntheticConfig()
    pw, tw, pw0, tw0 = _three(cfg, cfg.frames(20, 4), monkeypatch, off + "=0: ")
    if off == "LM_CORR_TAILSKIP":
        assert tw is None and tw0 is None and all(0 < a < b for a, b in zip(pw["listed"], pw0["listed"])), (pw, pw0, tw)
    else:
        assert pw is None and pw0 is None and all(a < b for a, b in zip(tw["listed"], tw0["listed"])), (tw, tw0, pw)
