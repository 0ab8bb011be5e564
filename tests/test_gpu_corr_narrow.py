"""The narrow class of ring work items on the GPU (LM_CORR_NARROW, default 1;
csrc/lm_corr_narrow.h): a listed tile whose unproven 8-column blocks span at
most two runs as a 20 x 4 item, every other as the whole 40 x 4 tile.  Every
case runs one batch with the class on and off: the results must be
bit-identical to each other and to the oracle, k_tile_bound's existing flags
and counters equal, per detector narrow + wide equal to the listed count, and
the narrow and wide entries together exactly the flagged tiles, each once, a
narrow entry's span inside its tile and never in a short last tile row.  Where
a case passes `host`, every entry's class and span must also equal the host
function's: tests/narrow_harness.py recomputes the block ranges from the
submitted frames and classifies every kept tile with lm_tbr_block_skip and
lm_nw_classify (tests/cpp/narrow_class_check.cpp entries), so the mask bits of
k_tile_bound's step 4b, their move with the entries and the untried bit are
compared entry by entry.  The raw score maps (debug bit 1) are read in both
runs too, but they come from k_corr_dbg, which the class cannot change: the
check on the narrow kernels' arithmetic is the candidates and tail results
against the oracle's.  The cases are the smallest shapes at which the class
takes another path: both correlation plans, a flipped view, two lanes, a frame
whose every kept tile is wide and one whose every kept tile is narrow,
checkerboard stripes over the default scene, ow % 40 and ow % 8 != 0 with
short last tile rows, windows 1 and 5 columns into their crop, ring widths
with and without a narrow kernel, blank frames, frames alternating with blank
ones (list segments with gaps), each skip alone and the switches that turn the
class off."""
import numpy as np
import pytest

import edge_scenes as E
import narrow_harness as H
from locomouse_cpp_amd import abi
from locomouse_cpp_amd import runtime as rt
from locomouse_cpp_amd import synthetic as S
from locomouse_cpp_amd.results import concat_results
from test_gpu_parity import _oracle, assert_same
from test_gpu_tail_skip import _plan
from test_gpu_tile_bound import POINT_DETS, _assert_state_equal, _state

pytestmark = pytest.mark.gpu

TAIL_DETS = (2, 5)
LAST = {}  # the entries and tile-grid widths of the last _pair run with the class on


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("narrow_host")
    return H.build(str(d / "narrow_class_check")), str(d / "views.bin")


def _check_host(cfg, frames, host, nw, ent, label):
    """Every entry against the host function: the narrow entries' (frame, tile)
    -> (first, count) and the wide entries' (frame, tile) are the host's."""
    ref = H.host_entries(host[0], cfg, frames, host[1])
    for d in nw:
        en, ew = ent[d]
        got_n = {(int(s) - 1, int(t)): (int(f), int(c)) for s, t, f, c in en if s >= 1}
        got_w = {(int(s) - 1, int(t)) for s, t, _, _ in ew if s >= 1}
        want_n = {k: v[1:] for k, v in ref[d].items() if v[0]}
        want_w = {k for k, v in ref[d].items() if not v[0]}
        assert got_n == want_n, (label, d, sorted(set(got_n.items()) ^ set(want_n.items()))[:6])
        assert got_w == want_w, (label, d, sorted(got_w ^ want_w)[:6])


def _lists(ctx, n):
    """narrow_work and, per detector, the narrow and wide entries as
    (slot, tile, first, count) rows (frame f of the batch is slot f + 1)."""
    nw = ctx.narrow_work()
    if nw is None:
        return None, None
    ent = {}
    for d in nw:
        ent[d] = [abi.narrow_entry_fields(ctx.narrow_entries(d, narrow)) for narrow in (1, 0)]
    return nw, ent


def _check_lists(ctx, n, state, nw, ent, label):
    pw, tw, pt, tt = state
    geo = ctx.geometry()
    for d, (narrow, wide) in nw.items():
        tail = d in TAIL_DETS
        listed = (tw["listed"][TAIL_DETS.index(d)] if tail else pw["listed"][POINT_DETS.index(d)])
        assert narrow + wide == listed, (label, d, narrow, wide, listed)
        en, ew = ent[d]
        assert len(en) == narrow and len(ew) == wide, (label, d, len(en), narrow, len(ew), wide)
        flags = [tt[2 * f + TAIL_DETS.index(d)] for f in range(n)] if tail else \
                [pt[len(POINT_DETS) * f + POINT_DETS.index(d)] for f in range(n)]
        fty, ftx = flags[0].shape
        s0 = 1  # frame f is slot f + 1; slot 0 is the frame before the batch
        seen = [np.zeros(fty * ftx, np.int32) for _ in range(n)]
        for e in (en, ew):
            for s, t in zip(e[:, 0], e[:, 1]):
                if s - s0 >= 0:  # (a halo slot's tiles are listed too; they have no flags here)
                    seen[s - s0][t] += 1
        for f in range(n):
            assert np.array_equal(seen[f].reshape(fty, ftx), (flags[f] != 0).astype(np.int32)), (label, d, f)
        box = geo.bb_side_mouse if d >= 3 else geo.bb_bottom_mouse
        oh = box.height
        for s, t, first, count in en:
            assert 1 <= count <= 2 and 0 <= first and first + count <= 5, (label, d, first, count)
            assert 4 * (t // ftx) + 4 <= oh, (label, d, "a short last tile row listed narrow", t)


def _pair(cfg, frames, monkeypatch, label, debug=0, lanes=1, oracle=True, expect_narrow=True, host=None):
    """One batch with LM_CORR_NARROW 1 and 0; returns narrow_work of the first."""
    n = len(frames)
    out = {}
    for on in ("1", "0"):
        monkeypatch.setenv("LM_CORR_NARROW", on)
        ctx = rt.Context(cfg, max_batch=n, lanes=lanes)
        ctx.set_debug(debug | 1)
        got = ctx.detect(frames, 0)
        st = _state(ctx, n)
        nw, ent = _lists(ctx, n)
        scores = [ctx.debug_scores(0, d) for d in range(6)]
        if on == "1" and nw is not None:
            _check_lists(ctx, n, st, nw, ent, label)
            LAST["ent"] = ent
            if host is not None:
                _check_host(cfg, frames, host, nw, ent, label)
            LAST["ftx"] = {d: (st[3][TAIL_DETS.index(d)] if d in TAIL_DETS else st[2][POINT_DETS.index(d)]).shape[1] for d in nw}
        ctx.close()
        out[on] = (got, st, nw, scores)
    print(label, out["1"][2])
    assert out["0"][2] is None, label
    assert (out["1"][2] is not None) == expect_narrow, (label, out["1"][2])
    assert_same(out["1"][0], out["0"][0], label + "narrow on against off: ")
    _assert_state_equal(out["1"][1], out["0"][1], label)
    for a, b in zip(out["1"][3], out["0"][3]):
        assert np.array_equal(a, b), label
    if oracle:
        assert_same(out["1"][0], _oracle(cfg, frames).result, label)
    return out["1"][2]


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("plan", [0, 1])
def test_default_c3(plan, flip, monkeypatch, host):
    """Three frames; every detector has narrow and wide tiles, and every entry
    has the host function's class and span (the unflipped view: the harness
    writes the views of the identity calibration)."""
    cfg = S.SyntheticConfig(flip=flip)
    nw = _pair(cfg, cfg.frames(20, 3), monkeypatch, f"C3 plan {plan} flip {flip}: ", debug=_plan(plan),
               host=None if flip else host)
    assert sorted(nw) == [0, 1, 2, 3, 4, 5] and all(a > 0 and b > 0 for a, b in nw.values()), nw


@pytest.mark.parametrize("plan", [0, 1])
def test_odd_boxes(plan, monkeypatch):
    """Bottom 397 x 139, side 397 x 89: a last tile column of 37 outputs (five
    blocks, the last of 5: ow % 40 and ow % 8 != 0) and last tile rows of three
    rows and of one, whose tiles stay wide."""
    cfg = S.SyntheticConfig(bounding_boxes={"side": (300, 3, 397, 89), "bottom": (300, 106, 397, 139)})
    nw = _pair(cfg, cfg.frames(40, 3), monkeypatch, f"odd boxes plan {plan}: ", debug=_plan(plan))
    assert all(a > 0 for a, _ in nw.values()), nw


def test_other_residues(monkeypatch):
    """paw_bottom 24 x 28 and tail_bottom 16 x 20 next to snout_bottom 30 x 30:
    their windows start 1 and 5 columns into the crop (in_x & 3 = 1)."""
    w = {"paw_bottom": S.dog_detector(24, 28, 6.0, 83), "tail_bottom": S.line_detector(16, 20, 1.5, 84)}
    base = S.SyntheticConfig(weights=w)
    cfg = S.SyntheticConfig(weights=w, biases=E._bias_for_rate(base, ["paw_bottom"]))
    nw = _pair(cfg, cfg.frames(10, 2), monkeypatch, "in_x mod 8 of 1 and 5: ")
    assert nw[0][0] > 0 and nw[2][0] > 0, nw


def test_wide_ring_widths(monkeypatch):
    """Ring widths 40 and 36 have narrow kernels, 48 and 64 do not: their
    detectors' tiles are all wide."""
    cfg = E.wide_ring_config()
    nw = _pair(cfg, cfg.frames(10, 2), monkeypatch, "wide rings: ")
    assert nw[2][0] == 0 and nw[3][0] == 0 and nw[1][0] > 0 and nw[5][0] > 0, nw


def test_touching_spans_and_straddling_tail_words(monkeypatch):
    """Twelve frames of the default scene hold the two places where a narrow
    item's ownership decides the result: horizontally adjacent tiles of a point
    detector that are both narrow with touching spans (the left one's ends at
    its last block, the right one's starts at its first: a key computed by both
    items must be listed once -- the oracle's candidate counts say so), and a
    tail item that owns 16 columns starting at 24 (mod 32), across two words of
    the tail bitmap."""
    cfg = S.SyntheticConfig()
    _pair(cfg, cfg.frames(0, 12), monkeypatch, "twelve frames: ")
    ent, ftx = LAST["ent"], LAST["ftx"]
    touching = 0
    for d in POINT_DETS:
        spans = {(int(s), int(t)): (int(f), int(c)) for s, t, f, c in ent[d][0]}
        for (s, t), (f, c) in spans.items():
            right = spans.get((s, t + 1))
            touching += f + c == 5 and (t + 1) % ftx[d] != 0 and right is not None and right[0] == 0
    straddling = sum(int(c) == 2 and (40 * (int(t) % ftx[d]) + 8 * int(f)) % 32 == 24 for d in TAIL_DETS for _, t, f, c in ent[d][0])
    print("touching pairs", touching, "straddling tail items", straddling)
    assert touching > 0 and straddling > 0, (touching, straddling)


@pytest.mark.parametrize("plan", [0, 1])
def test_every_kept_tile_wide(plan, monkeypatch, host):
    """A period-2 checkerboard over the whole image: every tile is kept with
    all five blocks unproven, so every narrow list is empty while the wide
    lists hold every tile (the narrow launches find no wave)."""
    cfg = S.SyntheticConfig()
    nw = _pair(cfg, E.checker_frames(cfg, 2), monkeypatch, f"all wide, plan {plan}: ", debug=_plan(plan), host=host)
    assert sorted(nw) == [0, 1, 2, 3, 4, 5] and all(a == 0 and b > 0 for a, b in nw.values()), nw


@pytest.mark.parametrize("plan", [0, 1])
def test_every_kept_tile_narrow(plan, monkeypatch, host):
    """Single bright pixels on the background, three in the bottom view and two
    in the side view: the few tiles around each are kept with one or two
    unproven blocks, so every wide list is empty and the wide launches find
    no wave."""
    cfg = S.SyntheticConfig()
    fr = np.stack([cfg.background.copy() for _ in range(2)])
    for k in range(2):
        for y, x in ((170 + 7 * k, 420), (180, 583 + k), (200, 652), (50 + 3 * k, 500), (40, 611)):
            fr[k, y, x] = min(int(fr[k, y, x]) + 120, 255)
    nw = _pair(cfg, fr, monkeypatch, f"all narrow, plan {plan}: ", debug=_plan(plan), host=host)
    assert sorted(nw) == [0, 1, 2, 3, 4, 5] and all(a > 0 and b == 0 for a, b in nw.values()), nw


def test_checkerboard_stripes(monkeypatch, host):
    """The period-2 checkerboard in every other stripe of 80 columns (two tile
    columns) of the default scene: full and nearly empty stretches side by side
    in every list segment."""
    cfg = S.SyntheticConfig()
    stripes = (np.arange(cfg.cols)[None, None, :] // 80) % 2 == 0
    fr = np.ascontiguousarray(np.where(stripes, E.checker_frames(cfg, 2, period=2), cfg.frames(20, 2)).astype(np.uint8))
    nw = _pair(cfg, fr, monkeypatch, "checker stripes: ", host=host)
    assert all(b > 0 for _, b in nw.values()), nw


def test_blank_frames(monkeypatch):
    cfg = S.SyntheticConfig()
    nw = _pair(cfg, np.stack([E.blank(cfg)] * 3), monkeypatch, "blank: ")
    assert all(v == (0, 0) for v in nw.values()), nw


def test_segments_with_gaps(monkeypatch):
    """17 frames (three ingest groups on shared list segments), every second
    one blank: segments with few entries and empty ones between them."""
    cfg = S.SyntheticConfig()
    fr = cfg.frames(0, 17)
    for k in range(1, 17, 2):
        fr[k] = E.blank(cfg)
    nw = _pair(cfg, fr, monkeypatch, "gaps: ")
    assert all(a > 0 and b > 0 for a, b in nw.values()), nw


@pytest.mark.parametrize("plan", [0, 1])
def test_two_lanes(plan, monkeypatch):
    """Batches of 4, 2 and 3 frames through two pipeline lanes (the later ones with a halo frame)."""
    cfg = S.SyntheticConfig()
    sizes = (4, 2, 3)
    frames = cfg.frames(0, sum(sizes))
    runs = {}
    for on in ("1", "0"):
        monkeypatch.setenv("LM_CORR_NARROW", on)
        ctx = rt.Context(cfg, max_batch=4, lanes=2)
        ctx.set_debug(_plan(plan))
        parts, first, k = [], 0, 0

        def collect():
            nonlocal k
            parts.append(ctx.collect())
            n = sizes[k]
            st = _state(ctx, n)
            nw, ent = _lists(ctx, n)
            if on == "1":
                assert nw is not None
                _check_lists(ctx, n, st, nw, ent, f"two lanes, batch {k}: ")
            k += 1
        for n in sizes:
            if ctx.pending() == 2:
                collect()
            ctx.submit(frames[first:first + n], first)
            first += n
        while ctx.pending():
            collect()
        ctx.close()
        runs[on] = concat_results(parts)
    assert_same(runs["1"], runs["0"], "two lanes, narrow on against off: ")
    assert_same(runs["1"], _oracle(cfg, frames).result, "two lanes: ")


def test_unfused_arithmetic(monkeypatch):
    cfg = S.SyntheticConfig()
    cfg.setup.filter_arith = abi.LM_FILTER_UNFUSED
    nw = _pair(cfg, cfg.frames(20, 2), monkeypatch, "unfused: ")
    assert all(a > 0 for a, _ in nw.values()), nw


@pytest.mark.parametrize("off", ["LM_CORR_TAILSKIP", "LM_CORR_POINTSKIP"])
def test_one_skip_alone(off, monkeypatch):
    """The class is off for the detectors whose skip is off."""
    monkeypatch.setenv(off, "0")
    cfg = S.SyntheticConfig()
    nw = _pair(cfg, cfg.frames(20, 2), monkeypatch, off + "=0: ")
    assert sorted(nw) == ([0, 1, 3, 4] if off == "LM_CORR_TAILSKIP" else [2, 5]), nw


@pytest.mark.parametrize("env", [("LM_TILE_REFINE", "0"), ("LM_TILE_BOUND_REF", "1"), ("LM_CORR_DARK", "0")])
def test_switches_that_turn_it_off(env, monkeypatch):
    monkeypatch.setenv(*env)
    cfg = S.SyntheticConfig()
    assert _pair(cfg, cfg.frames(20, 2), monkeypatch, f"{env[0]}={env[1]}: ", expect_narrow=False) is None


def test_without_the_directory(monkeypatch):
    """LM_CORR_DIR=0: the narrow waves walk their group's detectors."""
    monkeypatch.setenv("LM_CORR_DIR", "0")
    cfg = S.SyntheticConfig()
    _pair(cfg, cfg.frames(20, 2), monkeypatch, "no directory: ")
