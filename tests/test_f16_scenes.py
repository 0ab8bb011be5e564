"""The scenes of test_gpu_f16_shapes.py (f16_scenes.py), checked on the CPU
from the oracle alone: conditions on the inputs that keep the GPU comparison
from passing vacuously.  Every detector keeps the bound under which the f16
correlation must be bit-exact; in the sweep and edge cases every list is
long, every full 32 x 32 accumulator tile of a point detector's outputs holds
a candidate, candidates reach the last (partial) column and row block of each
view, and the tail map is about half positive and essentially one component
(so TAIL_MASK shows the map itself); the tall cases have candidates in every
list of every frame."""
import numpy as np
import pytest

import f16_scenes as F
from locomouse_cpp_amd.abi import frame_views


def _lists(sc):
    """[list][frame] -> (x, y) arrays of the compared frames."""
    res = sc.result
    out = [[] for _ in range(4)]
    for f in range(int(res["n_frames"])):
        v = frame_views(res, f)
        for lk in range(4):
            out[lk].append((np.asarray(v["cand"][lk]["x"]), np.asarray(v["cand"][lk]["y"])))
    return out


def _geom(sc):
    from oracle import oracle as O
    g = O.geometry(sc.cfg)
    return {"bottom": (g.bb_bottom_mouse.width, g.bb_bottom_mouse.height),
            "side": (g.bb_side_mouse.width, g.bb_side_mouse.height), "tail_w": g.tail_box_width}


def test_case_table_covers_the_issue():
    cases = F.CASES
    for nch in range(2, 11):
        c = cases[f"nch{nch}"]
        assert c.classes == [nch] and c.boxes == ("A" if nch % 2 else "B")
        lo, hi = F.kw_range(nch)
        assert F.nch_of(lo) == nch == F.nch_of(hi) and F.nch_of(hi + 1) == nch + 1 and (lo == 1 or F.nch_of(lo - 1) == nch - 1)
        assert [c.size(n)[0] for n in ("paw_bottom", "snout_bottom", "tail_bottom", "paw_side", "snout_side", "tail_side")] \
            == [5, 7, 4, 2, 1, 3]
        assert c.size("paw_bottom")[1] == hi == c.size("paw_side")[1] and c.size("snout_bottom")[1] == lo == c.size("snout_side")[1]
    assert cases["mixed"].classes == [3, 4, 6, 7, 9, 10]
    for name in ("moving", "flip", "seam"):
        assert len(cases[name].classes) == 1 and cases[name].classes[0] >= 7
    assert cases["tall64"].size("paw_bottom") == (64, 129) and cases["tall247"].size("paw_bottom") == (247, 129)
    assert cases["tall64"].classes == [10] == cases["tall247"].classes


@pytest.mark.parametrize("name", list(F.CASES))
def test_geometry_and_exactness_bound(name):
    sc = F.scene(name)
    g = _geom(sc)
    box = F.BOXES[sc.case.boxes]
    assert g["bottom"] == box["bottom"][2:] and g["side"] == box["side"][2:] and g["tail_w"] == box["bottom"][2]
    for n, w in sc.cfg.weights.items():
        assert np.array_equal(np.round(w * 4096) / 4096, w) and np.abs(w * 4096).max() <= 4
        if sc.case.kind == "dense" and n == "tail_bottom":
            # only the sign of these scores is observed: no sum reaches the bias
            assert 255.0 * np.abs(w).sum() < 1e5 and sc.cfg.biases[n] == -1e6
            continue
        b = F.exactness_bound(w, sc.cfg.biases[n])
        print(f"{name} {n} {w.shape}: bound {b:.0f}")
        assert b < 2 ** 24, (name, n, b)
        assert sc.cfg.biases[n] * 4096 == round(sc.cfg.biases[n] * 4096)


@pytest.mark.parametrize("name", F.SWEEP)
def test_sweep_scene_is_not_vacuous(name):
    sc = F.scene(name)
    assert all(kh <= 8 for _, (kh, _) in sc.case.sizes)
    g = _geom(sc)
    lists = _lists(sc)
    counts = [sum(len(x) for x, _ in lists[lk]) for lk in range(4)]
    print(f"{name}: candidates per list {counts}")
    assert min(counts) >= 30, counts
    for lk, view in ((0, "bottom"), (1, "bottom"), (2, "side"), (3, "side")):
        ow, oh = g[view]
        xs = np.concatenate([x for x, _ in lists[lk]])
        ys = np.concatenate([y for _, y in lists[lk]])
        # every full 32 x 32 block (an accumulator tile that is not cut by the output's edge)
        hit = np.zeros((oh // 32, ow // 32), bool)
        full = (ys < oh // 32 * 32) & (xs < ow // 32 * 32)
        hit[ys[full] // 32, xs[full] // 32] = True
        assert hit.all(), (name, lk, hit)
    for view, lks in (("bottom", (0, 1)), ("side", (2, 3))):
        ow, oh = g[view]
        xs = np.concatenate([x for lk in lks for x, _ in lists[lk]])
        ys = np.concatenate([y for lk in lks for _, y in lists[lk]])
        print(f"{name} {view}: ow {ow} oh {oh}, max x {xs.max()}, max y {ys.max()}")
        assert xs.max() == ow - 1 or xs.max() >= ow // 32 * 32, (name, view, xs.max())
        assert ys.max() == oh - 1 or ys.max() >= oh // 32 * 32, (name, view, ys.max())
    # tail_bottom: the positive map is about half of the box and TAIL_MASK (its largest component) nearly all of it
    shape = (g["bottom"][1], g["tail_w"])
    for f in range(sc.drop, len(sc.frames)):
        pos = sc.ref.scores(f, 2, shape) > 0
        mask = sc.ref.tail_mask(f, shape) != 0
        share, held = pos.mean(), (mask & pos).sum() / max(pos.sum(), 1)
        print(f"{name} frame {f}: tail_bottom positives {share:.3f} of the map, {held:.3f} of them in TAIL_MASK")
        assert not (mask & ~pos).any()
        assert 0.30 <= share <= 0.70 and held >= 0.90


@pytest.mark.parametrize("name", F.TALL)
def test_tall_scene_is_not_vacuous(name):
    sc = F.scene(name)
    lists = _lists(sc)
    counts = [[len(x) for x, _ in lists[lk]] for lk in range(4)]
    print(f"{name}: candidates per list and frame {counts}")
    assert all(n > 0 for per in counts for n in per), counts


def test_dense_tail_scene():
    sc = F.scene("dense_tail")
    g = _geom(sc)
    shape = (g["bottom"][1], g["tail_w"])
    for f in range(len(sc.frames)):
        assert sc.ref.tail_mask(f, shape).all()
