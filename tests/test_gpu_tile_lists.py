"""Step 5w of k_tile_bound<., true> (csrc/lm_kernels.hip): with the narrow class
on, one wave per detector of a view reads the detector's entries and marks
where steps 4 and 4b left them, 64 at a time, counts the kept ones per class by
ballots, takes its list places and writes every kept entry once; a band with
at most 64 entries of the detector keeps them in registers between the two
passes, a longer one reads the LDS again.  k_tile_bound<., false>
(LM_CORR_NARROW=0) keeps the tail it had and is the reference.

Every scene runs one small batch with LM_CORR_NARROW 1 and 0 through
test_gpu_corr_narrow._pair: the results bit-identical between the two runs and
to the oracle, the flag planes and the listed / bright counters equal, narrow +
wide = listed per detector, no (slot, tile) listed twice and the entries
exactly the flagged tiles; the narrow and the wide entries as sets equal to
the host statement's (tests/narrow_harness.py), a narrow one with its first
block and count.

The scenes are chosen for the pass's edges.  The band plan is restated here
from lm_tile_plan.h (lm_tbw_view) on the oracle's geometry, and checked against
the GPU's flag planes; the kept entries per (frame, band, detector) come from
the host statement before anything runs on the GPU.  At the default boxes a
bottom band is 9 tile rows of 10 (point) or 6 (tail) tile columns and a side
band 8 of 10 or 6, so a checkerboard over the left w columns of both boxes
gives counts of 9 x c and 8 x c: the search over w finds 63 (w 280), 72
and, in the side view's bands of 8 x 8, exactly 64 (both at w 320).
All three are asserted before the GPU run, 64 included: the search found it.
A count above 128 needs a band that holds that many
tiles of one detector, which three listed detectors never leave (a band is
about 256 tiles over all of them): with LM_CORR_POINTSKIP=0 the tail detector
is alone, its band is the whole grid (35 x 6 = 210 at the bottom) and the
search finds counts on both sides of 128 there."""
import numpy as np
import pytest

import edge_scenes as E
import narrow_harness as H
from locomouse_cpp_amd import runtime as rt
from locomouse_cpp_amd import synthetic as S
from locomouse_cpp_amd.results import concat_results
from test_gpu_corr_narrow import LAST, TAIL_DETS, _check_lists, _lists, _pair
from test_gpu_corr_narrow import host  # noqa: F401  (the host statement's program, built once)
from test_gpu_parity import _oracle, assert_same
from test_gpu_tail_skip import _plan
from test_gpu_tile_bound import _state
from test_tile_refine import DETS

pytestmark = pytest.mark.gpu

FW, FH, TILES = 40, 4, 256  # LM_FW, LM_FH, LM_TBW_TILES


def _grids(cfg):
    """{detector id: (tile rows, tile columns)} of the listed grids."""
    from oracle import oracle as O
    g, p = O.geometry(cfg), cfg.params
    out = {}
    for d, _, view, kind in DETS:
        box = p.bounding_box_side if view else p.bounding_box_bottom
        out[d] = (-(-box.height // FH), -(-(g.tail_box_width if kind else box.width) // FW))
    return out


def _band_rows(grids, listed):
    """Tile rows per band of the two views (lm_tbw_view) for the listed detectors."""
    br = []
    for v in (0, 1):
        ds = [d for d in (3 * v, 3 * v + 1, 3 * v + 2) if d in listed]
        sum_tx = sum(grids[d][1] for d in ds)
        max_ty = max([grids[d][0] for d in ds] + [1])
        br0 = max(1, TILES // max(1, sum_tx))
        nband = -(-max_ty // br0)
        br.append(-(-max_ty // nband))
    return br


def _band_counts(ref, grids, br, listed):
    """{(frame, detector, band): kept entries} of the host statement `ref`."""
    out = {}
    for d in listed:
        for (f, t) in ref[d]:
            key = (f, d, (t // grids[d][1]) // br[d // 3])
            out[key] = out.get(key, 0) + 1
    return out


def _region_frames(cfg, widths):
    """The period-2 checkerboard over the left w columns of both boxes, the background elsewhere."""
    x0 = cfg.params.bounding_box_bottom.x
    chk = E.checker_frames(cfg, len(widths))
    cols = np.arange(cfg.cols)[None, :]
    return np.stack([np.where((cols >= x0) & (cols < x0 + w), chk[i], E.blank(cfg)).astype(np.uint8)
                     for i, w in enumerate(widths)])


def _pick(counts, wanted):
    """Frames that together hold a (band, detector) count of every wanted kind: {kind: (frame, detector, band, count)}."""
    found = {}
    for name, ok in wanted.items():
        hits = sorted((k for k, n in counts.items() if ok(n)), key=lambda k: (k[0] not in {h[0] for h in found.values()}, k))
        if hits:
            found[name] = hits[0] + (counts[hits[0]],)
    return found


def _check_host_sets(cfg, frames, host, nw, ent, label, all_wide=()):  # noqa: F811
    """The entries against the host statement; a detector in all_wide (no narrow kernel for its ring width:
    LmConst::nw_on 0) has every kept tile of the host's in its wide list."""
    ref = H.host_entries(host[0], cfg, frames, host[1])
    for d in nw:
        en, ew = ent[d]
        got_n = {(int(s) - 1, int(t)): (int(f), int(c)) for s, t, f, c in en if s >= 1}
        got_w = {(int(s) - 1, int(t)) for s, t, _, _ in ew if s >= 1}
        if d in all_wide:
            want_n, want_w = {}, set(ref[d])
        else:
            want_n = {k: v[1:] for k, v in ref[d].items() if v[0]}
            want_w = {k for k, v in ref[d].items() if not v[0]}
        assert got_n == want_n, (label, d, sorted(set(got_n.items()) ^ set(want_n.items()))[:6])
        assert got_w == want_w, (label, d, sorted(got_w ^ want_w)[:6])


def _assert_grids(grids):
    """The restated tile grids are the GPU's (the widths of its flag planes)."""
    for d, tx in LAST["ftx"].items():
        assert grids[d][1] == tx, (d, grids[d], tx)


def test_blank_frames(monkeypatch):
    """No band has an entry: every wave leaves before its first pass."""
    cfg = S.SyntheticConfig()
    nw = _pair(cfg, np.stack([E.blank(cfg)] * 2), monkeypatch, "blank: ")
    assert sorted(nw) == [0, 1, 2, 3, 4, 5] and all(v == (0, 0) for v in nw.values()), nw


@pytest.mark.parametrize("plan", [0, 1])
def test_default_scene(plan, monkeypatch, host):  # noqa: F811
    cfg = S.SyntheticConfig()
    nw = _pair(cfg, cfg.frames(20, 2), monkeypatch, f"default, plan {plan}: ", debug=_plan(plan), host=host)
    assert sorted(nw) == [0, 1, 2, 3, 4, 5] and all(a > 0 and b > 0 for a, b in nw.values()), nw
    _assert_grids(_grids(cfg))


def test_every_kept_tile_wide(monkeypatch, host):  # noqa: F811
    """The checkerboard over the whole image: every band is full (90 and 80
    entries of a point detector: two chunks, read again by the second pass),
    every entry wide."""
    cfg = S.SyntheticConfig()
    nw = _pair(cfg, E.checker_frames(cfg, 2), monkeypatch, "all wide: ", host=host)
    assert all(a == 0 and b > 0 for a, b in nw.values()), nw


def test_every_kept_tile_narrow(monkeypatch, host):  # noqa: F811
    """Single bright pixels: a few entries per band, all narrow, most bands empty."""
    cfg = S.SyntheticConfig()
    fr = np.stack([cfg.background.copy() for _ in range(2)])
    for k in range(2):
        for y, x in ((170 + 7 * k, 420), (180, 583 + k), (200, 652), (50 + 3 * k, 500), (40, 611)):
            fr[k, y, x] = min(int(fr[k, y, x]) + 120, 255)
    nw = _pair(cfg, fr, monkeypatch, "all narrow: ", host=host)
    assert all(a > 0 and b == 0 for a, b in nw.values()), nw


def test_region_scenes(monkeypatch, host):  # noqa: F811
    """Counts of a (band, detector) on both sides of 64, and exactly 64."""
    cfg = S.SyntheticConfig()
    grids, listed = _grids(cfg), range(6)
    br = _band_rows(grids, listed)
    widths = list(range(200, 401, 40))
    cand = _region_frames(cfg, widths)
    counts = _band_counts(H.host_entries(host[0], cfg, cand, host[1]), grids, br, listed)
    found = _pick(counts, {"56 to 63": lambda n: 56 <= n <= 63, "64": lambda n: n == 64, "65 to 128": lambda n: 65 <= n <= 128})
    print("bands", br, "region widths", widths, "found", found)
    assert sorted(found) == ["56 to 63", "64", "65 to 128"], (found, sorted(set(counts.values())))
    frames = cand[sorted({v[0] for v in found.values()})]
    _pair(cfg, frames, monkeypatch, "regions: ", host=host)
    _assert_grids(grids)


def test_region_scenes_tail_alone(monkeypatch, host):  # noqa: F811
    """LM_CORR_POINTSKIP=0: the point detectors' waves leave (not listed), the
    tail detector's band is its whole grid, and the regions give it counts on
    both sides of 128 (two chunks, and three or four)."""
    monkeypatch.setenv("LM_CORR_POINTSKIP", "0")
    cfg = S.SyntheticConfig()
    grids, listed = _grids(cfg), TAIL_DETS
    br = _band_rows(grids, listed)
    widths = list(range(80, 241, 40))
    cand = _region_frames(cfg, widths)
    counts = _band_counts(H.host_entries(host[0], cfg, cand, host[1]), grids, br, listed)
    found = _pick(counts, {"65 to 128": lambda n: 65 <= n <= 128, "129 to 192": lambda n: 129 <= n <= 192, "above 192": lambda n: n > 192})
    print("bands", br, "region widths", widths, "found", found)
    assert sorted(found) == ["129 to 192", "65 to 128", "above 192"], (found, sorted(set(counts.values())))
    frames = cand[sorted({v[0] for v in found.values()})]
    nw = _pair(cfg, frames, monkeypatch, "regions, tail alone: ", host=host)
    assert sorted(nw) == [2, 5], nw


def test_tail_skip_off(monkeypatch, host):  # noqa: F811
    """LM_CORR_TAILSKIP=0: the third wave's detector is not listed."""
    monkeypatch.setenv("LM_CORR_TAILSKIP", "0")
    cfg = S.SyntheticConfig()
    nw = _pair(cfg, cfg.frames(20, 2), monkeypatch, "tail skip off: ", host=host)
    assert sorted(nw) == [0, 1, 3, 4], nw


def test_mixed_classes(monkeypatch, host):  # noqa: F811
    """Ring widths 48 and 64 have no narrow kernel (nw_on 0): tail_bottom and
    paw_side go all wide through the pass that splits their neighbours."""
    cfg = E.wide_ring_config()
    frames = cfg.frames(10, 2)
    nw = _pair(cfg, frames, monkeypatch, "mixed classes: ")
    assert nw[2][0] == 0 and nw[3][0] == 0 and nw[1][0] > 0 and nw[5][0] > 0, nw
    _check_host_sets(cfg, frames, host, nw, LAST["ent"], "mixed classes: ", all_wide=(2, 3))


def test_two_list_segments(monkeypatch, host):  # noqa: F811
    """Ten frames: two slot groups (LM_INGEST_FB = 8 slots each), each on a list segment of its own."""
    cfg = S.SyntheticConfig()
    nw = _pair(cfg, cfg.frames(0, 10), monkeypatch, "two segments: ", host=host)
    assert all(a > 0 and b > 0 for a, b in nw.values()), nw


def test_two_lanes(monkeypatch, host):  # noqa: F811
    """Batches of 3 and 2 frames through two pipeline lanes (the second with a halo frame)."""
    cfg = S.SyntheticConfig()
    sizes = (3, 2)
    frames = cfg.frames(0, sum(sizes))
    runs = {}
    for on in ("1", "0"):
        monkeypatch.setenv("LM_CORR_NARROW", on)
        ctx = rt.Context(cfg, max_batch=3, lanes=2)
        parts, first = [], 0
        for n in sizes:
            ctx.submit(frames[first:first + n], first)
            first += n
        first = 0
        for k, n in enumerate(sizes):
            parts.append(ctx.collect())
            if on == "1":
                st = _state(ctx, n)
                nw, ent = _lists(ctx, n)
                assert nw is not None
                _check_lists(ctx, n, st, nw, ent, f"two lanes, batch {k}: ")
                _check_host_sets(cfg, frames[first:first + n], host, nw, ent, f"two lanes, batch {k}: ")
            first += n
        ctx.close()
        runs[on] = concat_results(parts)
    assert_same(runs["1"], runs["0"], "two lanes, narrow on against off: ")
    assert_same(runs["1"], _oracle(cfg, frames).result, "two lanes: ")
