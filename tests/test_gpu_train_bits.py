"""The SVM solver's answers, to the bit, against tests/golden/train_bits.json.

lm_train_solve is a one-problem lm_train_solve_many (csrc/lm_train.hip holds
one solver), so the comparisons of the two in tests/test_gpu_train_cv.py guard
lm_train_solve's wrapper and no longer the arithmetic.  The fixture holds what
the tree with two separate solvers returned (tests/golden/make_train_bits.py
names the commit): lm_train_solve at test_gpu_train_cv.py's SINGLE_CASES, the
"costs" kind at 5 x 7 with 300 and 1025 samples, the two unconverged exits of
test_gpu_train.py's test_max_iter_returns_ok_unconverged, lm_train_margins of
the returned model at three of them, and one lm_train_solve_many call of the
2 PB + 1 list per company case with its held-out counts.  Nothing here has a
tolerance.  A fixture entry whose inputs are not this test's fails with a
message that says so."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_train_bits as TB  # noqa: E402
import train_cv_harness as CV  # noqa: E402
import train_harness as TH  # noqa: E402

from locomouse_cpp_amd import runtime  # noqa: E402

FIXTURE = TB.load()


def test_the_fixture_holds_the_cases():
    import test_gpu_train_cv as T
    assert TB.SINGLE_CASES == T.SINGLE_CASES and TB.EPS == T.EPS
    want = {TB.solve_key(s, n, TH.KINDS[i % len(TH.KINDS)], *TH.kind_costs(TH.KINDS[i % len(TH.KINDS)]), TB.EPS, 200)
            for i, (s, n) in enumerate(TB.SINGLE_CASES)}
    want |= {TB.solve_key((5, 7), n, "costs", 10.0, 1.0, TB.EPS, 200) for n in (300, 1025)}
    want |= {TB.solve_key((5, 7), 200, "overlapping", 1.0, 1.0, 1e-12, m) for m in (1, 0)}
    assert set(FIXTURE["solve"]) == want
    with_margins = {(tuple(e["size"]), e["n"], e["kind"]) for e in FIXTURE["solve"].values() if "margins_sha256" in e}
    assert with_margins == {((5, 7), 1025, "constant_column"), ((5, 7), 1025, "costs"), ((24, 24), 1000, "separable")}
    assert set(FIXTURE["solve_many"]) == {TB.many_key(s, n) for s, n in CV.COMPANY_CASES}
    assert len(FIXTURE["produced_by"]["commit"]) == 40 and FIXTURE["produced_by"]["hipcc_version"]


@pytest.mark.gpu
@pytest.mark.parametrize("key", sorted(FIXTURE["solve"]))
def test_solve_returns_the_recorded_bits(key):
    e = FIXTURE["solve"][key]
    kh, kw = e["size"]
    P, y = TH.sample_set(e["kind"], e["n"], kh * kw)
    tr = runtime.Trainer(kh, kw, e["n"])
    h = e["n"] // 2  # in two adds, as test_gpu_train.py stores them
    if h:
        tr.add_patches(P[:h], y[:h])
    tr.add_patches(P[h:], y[h:])
    one = tr.solve(e["c_pos"], e["c_neg"], e["eps"], e["max_iter"])
    z = tr.margins(one[0], one[1]) if "margins_sha256" in e else None
    assert not (msg := TB.mismatch(e, P, y, [one], z=z)), msg
    # and through the other entry point, after which lm_train_solve returns them again
    many = list(zip(*tr.solve_many([(e["c_pos"], e["c_neg"], -1)], e["eps"], e["max_iter"])))
    assert not (msg := TB.mismatch(e, P, y, [many[0][:3]])), msg
    assert not (msg := TB.mismatch(e, P, y, [tr.solve(e["c_pos"], e["c_neg"], e["eps"], e["max_iter"])])), msg
    tr.close()


@pytest.mark.gpu
@pytest.mark.parametrize("key", sorted(FIXTURE["solve_many"]))
def test_the_long_company_list_returns_the_recorded_bits(key):
    e = FIXTURE["solve_many"][key]
    kh, kw = e["size"]
    P, y = TH.sample_set(e["kind"], e["n"], kh * kw)
    groups = CV.company_groups(e["n"])
    tr = runtime.Trainer(kh, kw, e["n"] + 17)
    tr.add_patches(P, y)
    tr.set_groups(groups)
    problems = TB.the_long_list(CV, tr.problem_block())
    assert e["problem_block"] == tr.problem_block() and e["problems"] == [list(p) for p in problems]
    got = list(zip(*tr.solve_many(problems, e["eps"], e["max_iter"])))
    assert not (msg := TB.mismatch(e, P, y, got, groups=groups)), msg
    tr.close()
