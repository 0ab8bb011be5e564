"""Cross-validation of the SVM costs, the parts that need no GPU: the
LM_TRAIN_CV parser, the fold assignment and the selection rule of
host/Train.hpp against their restatements (tests/train_cv_harness.py), and
csrc/lm_train_core.h's host statement with a held-out group against the same
statement on the samples that are left, to the bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_cv_harness as CV  # noqa: E402
import train_harness as TH  # noqa: E402


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_structs_mirror_the_header():
    import ctypes as C

    from locomouse_cpp_amd import abi
    for which, T in enumerate((abi.lm_train_problem, abi.lm_train_heldout)):
        out = (C.c_int * 8)()
        n = CV.lib().thc_layout(which, out)
        assert n == len(T._fields_) and out[0] == C.sizeof(T)
        assert [out[1 + k] for k in range(n)] == [getattr(T, name).offset for name, _ in T._fields_]
    assert CV.lib().thc_max_problems() == abi.LM_TRAIN_MAX_PROBLEMS and CV.lib().thc_max_groups() == abi.LM_TRAIN_MAX_GROUPS


# ------------------------------------------------------------------ the knob

@pytest.mark.parametrize("spec,want", [
    ("5:0.01,0.1,1,10,100", (5, [0.01, 0.1, 1.0, 10.0, 100.0])),
    ("2:1", (2, [1.0])),
    ("16:1,2,3,4", (16, [1.0, 2.0, 3.0, 4.0])),
    ("4:" + ",".join(str(k + 1) for k in range(16)), (4, [float(k + 1) for k in range(16)])),
    ("3:1e-2,1E2,.5", (3, [0.01, 100.0, 0.5])),
])
def test_cv_spec_accepted(spec, want):
    assert CV.parse_cv(spec) == want


@pytest.mark.parametrize("spec", [
    "", "5", "5:", ":1", "5:1:2", "1:1", "17:1", "25:1", "0:1", "-3:1", "3.5:1", "x:1", "5:0", "5:-1", "5:inf", "5:nan",
    "5:1,,2", "5:1,", "5:,1", "5:1,1", "5:1,1.0", "5:1,2x", "5: 1",
    "5:" + ",".join(str(k + 1) for k in range(13)),  # 5 x 13 = 65 problems
    "2:" + ",".join(str(k + 1) for k in range(17)),  # 17 scales
    "16:1,2,3,4,5",  # 80 problems
])
def test_cv_spec_refused(spec):
    got = CV.parse_cv(spec)
    assert isinstance(got, str) and got.startswith("LM_TRAIN_CV: "), (spec, got)


def test_fewer_labelled_frames_than_folds_is_refused():
    assert CV.check_cv([3, 3, 7, 9, 9], 3, [1.0]) == ""
    msg = CV.check_cv([3, 3, 7, 9, 9], 4, [1.0])
    assert msg.startswith("LM_TRAIN_CV: ") and "labels_paw_bottom" in msg, msg
    assert CV.check_cv([3], 0, []) == ""  # off
    assert CV.check_cv(list(range(20)), 17, [1.0]).startswith("LM_TRAIN_CV: ")
    assert CV.check_cv(list(range(20)), 5, []).startswith("LM_TRAIN_CV: ")
    assert CV.check_cv(list(range(20)), 5, [1.0, 1.0]).startswith("LM_TRAIN_CV: ")


# ------------------------------------------------------------------ folds

@pytest.mark.parametrize("k", [2, 3, 5, 16])
def test_fold_assignment(k):
    rng = np.random.default_rng(k)
    frames = rng.choice(np.arange(0, 4000, 7), size=37, replace=False)
    sample_frames = rng.choice(frames, size=900)  # labels, initial and mined negatives in any order
    got = CV.folds(sample_frames, k)
    want = CV.ref_folds(sample_frames, k)
    assert np.array_equal(got, want)
    # a frame is never on both sides, and consecutive frames alternate
    order = np.sort(np.unique(sample_frames))
    for r, f in enumerate(order):
        assert set(got[sample_frames == f]) == {r % k}


# -------------------------------------------------------------- selection

def test_selection_rule_random_tables():
    rng = np.random.default_rng(11)
    for trial in range(400):
        n = int(rng.integers(1, 17))
        scales = rng.permutation(np.array(CV.SCALES + (0.03, 0.5, 2.0, 5.0, 50.0, 200.0, 0.2, 20.0)))[:n]
        big = trial % 4 == 0
        n_pos = int(rng.integers(0, 2 ** 22 if big else 6))
        n_neg = int(rng.integers(0, 2 ** 22 if big else 6))
        if trial % 7 == 0:
            n_pos = 0
        if trial % 11 == 0:
            n_neg = 0
        rows = [(n_pos, n_neg, int(rng.integers(0, n_pos + 1)), int(rng.integers(0, n_neg + 1))) for _ in range(n)]
        best, score = CV.select(scales, rows)
        assert best == CV.ref_select(list(scales), rows), (scales, rows)
        for k in range(n):
            assert score[k] == pytest.approx(float(CV.ref_score(rows[k])), rel=1e-15, abs=0)


def test_selection_ties_and_empty_classes():
    # equal scores: the smaller scale, wherever it stands
    assert CV.select([10.0, 0.1, 1.0], [(4, 8, 1, 2)] * 3)[0] == 1
    # 1/3 + 1/6 = 1/2 = 2/4 + 0/6 exactly, although neither side is a binary fraction
    assert CV.select([2.0, 1.0], [(3, 6, 1, 1), (4, 6, 2, 0)])[0] == 1
    assert CV.select([1.0, 2.0], [(3, 6, 1, 1), (4, 6, 2, 0)])[0] == 0
    # a difference of one part in 2^44 decides
    n = 2 ** 22 - 1
    assert CV.select([1.0, 2.0], [(n, n, 1000, 1001), (n, n, 1000, 1000)])[0] == 1
    # no positives: the negatives' term alone; no samples at all: score 0
    best, score = CV.select([1.0, 2.0, 3.0], [(0, 10, 0, 3), (0, 10, 0, 2), (0, 10, 0, 2)])
    assert best == 1 and list(score) == [0.15, 0.1, 0.1]
    best, score = CV.select([5.0, 3.0], [(0, 0, 0, 0), (0, 0, 0, 0)])
    assert best == 1 and list(score) == [0.0, 0.0]
    best, score = CV.select([1.0, 2.0], [(8, 0, 4, 0), (8, 0, 2, 0)])
    assert best == 1 and list(score) == [0.25, 0.125]


# ------------------------------------------- the host statement, held out

@pytest.mark.parametrize("kind", TH.KINDS)
@pytest.mark.parametrize("n,d", [(65, 35), (200, 416)])
def test_held_out_statement_equals_the_subsets(kind, n, d):
    P, y = TH.sample_set(kind, n, d)
    cp, cn = TH.kind_costs(kind)
    group = (np.arange(n) % 5).astype(np.uint8)
    rng = np.random.default_rng(n + d)
    for h in (0, 3, 7, -1):  # 7: a group without samples
        keep = group != h if h >= 0 else np.ones(n, bool)
        for wb in (np.zeros(d + 1), rng.standard_normal(d + 1) * 0.02):
            F, g, z, a, na = CV.host_objective(P, y, group, cp, cn, h, wb)
            F1, g1, z1, a1, na1 = TH.host_objective(P[keep], y[keep], cp, cn, wb)
            assert bits([F]) == bits([F1]) and np.array_equal(bits(g), bits(g1)) and na == na1
            assert np.array_equal(bits(z[keep]), bits(z1)) and np.array_equal(bits(a[keep]), bits(a1))
            assert not a[~keep].any()
            v = rng.standard_normal(d + 1)
            assert np.array_equal(bits(TH.host_hessvec(P, a, v)), bits(TH.host_hessvec(P[keep], a1, v)))
            xd = rng.standard_normal(n)
            for scale in (1.0, 1e-3, 1e3):  # steps that are taken at once, late, and never
                wd, dd, gd = 0.3 * scale, 2.0 * scale, -1.5 * scale
                got = CV.host_linesearch(y, group, z, xd * scale, cp, cn, h, wd, dd, gd)
                want = TH.host_linesearch(y[keep], z1, xd[keep] * scale, cp, cn, wd, dd, gd)
                assert got[0] == want[0] and bits([got[1]]) == bits([want[1]])


@pytest.mark.parametrize("size,n", CV.COMPANY_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_company_sets_leave_few_held_out_signs_open(size, n):
    """The sets of the GPU tests' held-out counts: at the reference solver's
    minimiser at most 2 % of a held-out group's margins are closer to 0 than
    the rounding bound of their evaluation, for every held-out problem."""
    import train_ref as R
    d = size[0] * size[1]
    P, y = TH.sample_set("overlapping", n, d)
    groups = CV.company_groups(n)
    Xt = R.xtilde(P)
    for scale, h in CV.POOL:
        if h < 0:
            continue
        keep = groups != h
        w, b, st = R.solve(P[keep], y[keep], scale, scale, 1e-8, 200)
        wb = np.append(w, b)
        z = (Xt[~keep].astype(np.longdouble) @ wb.astype(np.longdouble)).astype(np.float64)
        bound = 2 * (d + 1) * 2.0 ** -53 * (np.abs(Xt[~keep]) @ np.abs(wb))
        n_open = int((np.abs(z) <= bound).sum())
        assert n_open <= 0.02 * (~keep).sum(), (scale, h, n_open)


def test_problem_block_fits_the_lds():
    for side in range(1, 65):
        for kw in (1, side, 64):
            d = side * kw
            pb = CV.lib().thc_problem_block(d)
            vl = (d + 15) // 16 * 16 + 1
            assert pb in (1, 2, 4) and (pb == 1 or pb * vl * 8 <= 48 * 1024)
            assert pb == 4 or 2 * pb * vl * 8 > 48 * 1024  # the largest that fits
    assert CV.lib().thc_problem_block(24 * 24) == 4 and CV.lib().thc_problem_block(64 * 64) == 1
