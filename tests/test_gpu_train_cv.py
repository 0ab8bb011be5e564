"""Several SVM problems on the same samples in one pass (lm_train_solve_many,
include/locomouse_train.h) and the cross-validation of the costs built on it
(host/Train.hpp, LM_TRAIN_CV).

The batched solver is tested against the single one to the bit: a problem
without a held-out group returns what lm_train_solve returns, and any problem
returns the same alone or in any company and order.  That a held-out problem
minimises the objective of the samples that are left is checked as
tests/test_gpu_train.py checks the single solver, with numpy float64
(tests/train_ref.py) on the subset and the rounding bounds of that evaluation
alone.  The held-out counts are bracketed by the margins whose sign the
rounding bound of their evaluation leaves open."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import media_writers as MW  # noqa: E402
import train_cv_harness as CV  # noqa: E402
import train_harness as TH  # noqa: E402
import train_ref as R  # noqa: E402

from locomouse_cpp_amd import abi, runtime  # noqa: E402
from locomouse_cpp_amd import synthetic as S  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 1e-8
INVALID = abi.LM_ERR_INVALID_ARGUMENT


def ident(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def same(a, b):
    """Two results (W, rho, stats[, heldout]) are bit-identical."""
    return (np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64))
            and np.float64(a[1]).view(np.uint64) == np.float64(b[1]).view(np.uint64) and all(x == y for x, y in zip(a[2:], b[2:])))


def results(out):
    """solve_many's four lists as one (W, rho, stats, heldout) per problem."""
    return list(zip(*out))


def trainer(P, y, kh, kw, groups=None, room=0):
    tr = runtime.Trainer(kh, kw, len(y) + room)
    tr.add_patches(P, y)
    if groups is not None:
        tr.set_groups(groups)
    return tr


def reaches_the_minimiser(P, y, keep, cp, cn, res):
    """Asserts 1 and 2 of test_gpu_train.py's test_solver_reaches_the_minimiser on the samples `keep`."""
    W, rho, st = res[:3]
    Xt = R.xtilde(P[keep])
    wb = np.append(W.reshape(-1) * 255.0, -rho)
    F, g, a, sF, sg = R.objective(Xt, y[keep], cp, cn, wb)
    g0 = float(np.linalg.norm(R.objective(Xt, y[keep], cp, cn, np.zeros(len(wb)))[1]))
    gn, s = float(np.linalg.norm(g)), float(np.linalg.norm(sg))
    print(f"costs ({cp}, {cn}) on {int(np.sum(keep))} samples: |g|={gn:.3e} eps|g0|={EPS * g0:.3e} s={s:.3e} "
          f"dF={st['objective'] - F:.3e} sF={sF:.3e} outer={st['outer_iters']} cg={st['cg_iters']}")
    assert st["converged"] == 1, st
    assert gn <= EPS * g0 + s
    assert abs(st["objective"] - F) <= sF


# ------------------------------------------- 1: equal to the single solver

SINGLE_CASES = [((1, 1), 1), ((5, 7), 65), ((5, 7), 1023), ((5, 7), 1024), ((5, 7), 1025), ((16, 26), 1000),
                ((24, 24), 1000), ((64, 64), 70)]


@pytest.mark.parametrize("size,n,kind", [(s, n, TH.KINDS[i % len(TH.KINDS)]) for i, (s, n) in enumerate(SINGLE_CASES)],
                         ids=ident)
def test_one_problem_equals_the_single_solver(size, n, kind):
    kh, kw = size
    P, y = TH.sample_set(kind, n, kh * kw)
    cp, cn = TH.kind_costs(kind)
    tr = trainer(P, y, kh, kw)
    one = tr.solve(cp, cn, EPS, 200)
    many = results(tr.solve_many([(cp, cn, -1)], EPS, 200))
    assert len(many) == 1 and same(one, many[0][:3]), (one[2], many[0][2])
    assert many[0][3] == {"n_pos": 0, "n_neg": 0, "miss_pos": 0, "miss_neg": 0}
    again = tr.solve(cp, cn, EPS, 200)  # the single solver's arrays are its own
    assert same(one, again)
    tr.close()


def test_costs_kind_with_its_costs():
    P, y = TH.sample_set("costs", 300, 35)
    assert TH.kind_costs("costs") == (10.0, 1.0)
    tr = trainer(P, y, 5, 7)
    assert same(tr.solve(10.0, 1.0, EPS, 200), results(tr.solve_many([(10.0, 1.0, -1)], EPS, 200))[0][:3])
    tr.close()


# ---------------------------------------- 2: independent of the company

@pytest.fixture(scope="module", params=CV.COMPANY_CASES, ids=ident)
def company(request):
    """(P, y, groups, the Trainer, PB, {problem: its result alone})."""
    (kh, kw), n = request.param
    P, y = TH.sample_set("overlapping", n, kh * kw)
    groups = CV.company_groups(n)
    tr = trainer(P, y, kh, kw, groups, room=17)
    alone = {q: results(tr.solve_many([(q[0], q[0], q[1])], EPS, 200))[0] for q in CV.POOL}
    yield P, y, groups, tr, tr.problem_block(), alone
    tr.close()


def test_independent_of_the_company(company):
    P, y, groups, tr, pb, alone = company
    assert pb == CV.lib().thc_problem_block(P.shape[1]) and pb >= 1
    lists = CV.company_lists(pb)
    assert sorted(len(l) for l in lists) == sorted({1, 2, max(pb - 1, 1), pb, pb + 1, 2 * pb + 1})
    assert {q for l in lists for q in l} == set(CV.POOL) and all(len(set(l)) == len(l) - 1 for l in lists if len(l) > 1)
    for lst in lists:
        pr = [(s, s, h) for s, h in lst]
        got = results(tr.solve_many(pr, EPS, 200))
        for q, r in zip(lst, got):
            assert same(alone[q], r), (len(lst), q, alone[q][2:], r[2:])
        back = results(tr.solve_many(pr[::-1], EPS, 200))[::-1]
        twice = results(tr.solve_many(pr, EPS, 200))
        for q, r, b, t in zip(lst, got, back, twice):
            assert same(r, b) and same(r, t), (len(lst), q)
    # without a held-out group it is the single solver's answer, whatever the groups
    for s, h in CV.POOL:
        if h < 0:
            assert same(tr.solve(s, s, EPS, 200), alone[(s, h)][:3])


# ------------------------- 3: the minimiser of the subset's objective

def test_held_out_problem_minimises_the_subsets_objective(company):
    P, y, groups, tr, pb, alone = company
    for (s, h), res in alone.items():
        if h >= 0:
            reaches_the_minimiser(P, y, groups != h, s, s, res)
            assert res[2]["n_active"] <= int(np.sum(groups != h))


# ------------------------------- 4: different lengths side by side

@pytest.fixture(scope="module")
def lengths():
    """One set of three groups: positives far from the negatives (0), positives
    close to them (1) and the negatives (2).  Holding out 1 leaves a separable
    problem, holding out 0 an overlapping one, holding out 2 one class."""
    n, d = 240, 35
    Ps, ys = TH.sample_set("separable", n, d)
    Po, yo = TH.sample_set("overlapping", n, d)
    P = np.vstack([Ps[ys > 0], Po[yo > 0], Po[yo < 0]])
    y = np.concatenate([np.ones(int((ys > 0).sum())), np.ones(int((yo > 0).sum())), -np.ones(int((yo < 0).sum()))]).astype(np.int8)
    groups = np.concatenate([np.zeros(int((ys > 0).sum())), np.ones(int((yo > 0).sum())), 2 * np.ones(int((yo < 0).sum()))]).astype(np.int32)
    problems = [(0.01, 0.01, 1), (100.0, 100.0, 0), (1.0, 1.0, 2)]
    tr = trainer(P, y, 5, 7, groups)
    yield P, y, groups, tr, problems
    tr.close()


def test_different_lengths_side_by_side(lengths):
    P, y, groups, tr, problems = lengths
    got = results(tr.solve_many(problems, EPS, 200))
    for pr, res in zip(problems, got):
        reaches_the_minimiser(P, y, groups != pr[2], pr[0], pr[1], res)
        assert same(results(tr.solve_many([pr], EPS, 200))[0], res)  # its own outer_iters among them
    print("outer iterations:", [r[2]["outer_iters"] for r in got])
    assert got[2][3] == {"n_pos": 0, "n_neg": int((y < 0).sum()), "miss_pos": 0, "miss_neg": got[2][3]["miss_neg"]}


def test_max_iter_per_problem(lengths):
    P, y, groups, tr, problems = lengths
    one = results(tr.solve_many(problems, 1e-12, 1))
    for pr, res in zip(problems, one):
        st = res[2]
        if not st["converged"]:
            assert st["outer_iters"] == 1 and st["grad_norm"] < st["grad_norm0"], st
        assert same(results(tr.solve_many([pr], 1e-12, 1))[0], res)
    assert any(not r[2]["converged"] for r in one)
    zero = results(tr.solve_many(problems, 1e-12, 0))
    for W, rho, st, ho in zero:
        assert not W.any() and rho == 0 and st["outer_iters"] == 0 and st["cg_iters"] == 0 and st["converged"] == 0
        assert st["grad_norm"] == st["grad_norm0"] > 0


# --------------------------------------------------- 5: held-out counts

def test_held_out_counts(company):
    P, y, groups, tr, pb, alone = company
    d = P.shape[1]
    Xt = R.xtilde(P)
    checked = 0
    for (s, h), (W, rho, st, ho) in alone.items():
        if h < 0:
            assert ho == {"n_pos": 0, "n_neg": 0, "miss_pos": 0, "miss_neg": 0}
            continue
        out = groups == h
        assert ho["n_pos"] == int((y[out] > 0).sum()) and ho["n_neg"] == int((y[out] < 0).sum())
        wb = np.append(W.reshape(-1) * 255.0, -rho)
        z = (Xt[out].astype(np.longdouble) @ wb.astype(np.longdouble)).astype(np.float64)
        bound = 2 * (d + 1) * 2.0 ** -53 * (np.abs(Xt[out]) @ np.abs(wb))
        pos, neg, is_open = y[out] > 0, y[out] < 0, np.abs(z) <= bound
        sure_pos, sure_neg = int((pos & (z < -bound)).sum()), int((neg & (z > bound)).sum())
        print(f"scale {s} held out {h}: {ho}, certain {sure_pos} / {sure_neg}, open {int(is_open.sum())}")
        assert sure_pos <= ho["miss_pos"] <= sure_pos + int((pos & is_open).sum())
        assert sure_neg <= ho["miss_neg"] <= sure_neg + int((neg & is_open).sum())
        checked += 1
    assert checked == sum(1 for _, h in CV.POOL if h >= 0)
    # a group without samples: counts 0, and the problem is the one without a held-out group
    empty = results(tr.solve_many([(1.0, 1.0, 200)], EPS, 200))[0]
    assert empty[3] == {"n_pos": 0, "n_neg": 0, "miss_pos": 0, "miss_neg": 0} and same(empty[:3], alone[(1.0, -1)][:3])


# ------------------------------------------------------------ 6: refusals

def _code(fn, *args):
    with pytest.raises(runtime.LMError) as e:
        fn(*args)
    return e.value.code


def _raw_solve_many(tr, pr, n, eps=1e-6, max_iter=100, null=None):
    """lm_train_solve_many with raw arguments: `null` names a pointer to pass as NULL."""
    import ctypes as C
    W = np.zeros((max(n, 1), tr.kh, tr.kw))
    rho = np.zeros(max(n, 1))
    args = {"ctx": tr._h, "problems": C.addressof(pr), "W": W.ctypes.data, "rho": rho.ctypes.data}
    if null:
        args[null] = None
    return runtime.lib().lm_train_solve_many(args["ctx"], args["problems"], n, eps, max_iter, args["W"], args["rho"], None,
                                             None)


def test_refusals_change_nothing():
    P, y = TH.sample_set("overlapping", 40, 35)
    groups = CV.company_groups(40)
    tr = runtime.Trainer(5, 7, 64)
    good = [(1.0, 1.0, -1), (10.0, 1.0, -1)]
    assert _code(tr.solve_many, good) == INVALID  # an empty context
    assert _code(tr.set_groups, []) == INVALID
    tr.add_patches(P, y)
    before = tr.patches()
    want_plain = results(tr.solve_many(good, EPS, 200))
    assert _code(tr.solve_many, [(1.0, 1.0, 0)]) == INVALID  # held_out without groups
    assert _code(tr.set_groups, groups[:39]) == INVALID and _code(tr.set_groups, np.append(groups, 0)) == INVALID
    for bad in (-1, 256, 1 << 20):
        g = groups.copy()
        g[7] = bad
        assert _code(tr.set_groups, g) == INVALID
    assert _code(tr.solve_many, [(1.0, 1.0, 0)]) == INVALID  # the refused calls set no groups
    tr.set_groups(groups)
    held = [(1.0, 1.0, 0), (3.0, 0.5, 4), (1.0, 1.0, -1)]
    want_held = results(tr.solve_many(held, EPS, 200))

    def unchanged():
        assert tr.samples() == (int((y > 0).sum()), int((y < 0).sum()))
        after = tr.patches()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        for w, r in zip(want_held, results(tr.solve_many(held, EPS, 200))):  # the groups are still set
            assert same(w, r)
        for w, r in zip(want_plain, results(tr.solve_many(good, EPS, 200))):
            assert same(w, r)

    assert _code(tr.solve_many, []) == INVALID
    assert _code(tr.solve_many, [(1.0, 1.0, -1)] * (abi.LM_TRAIN_MAX_PROBLEMS + 1)) == INVALID
    for cp, cn in ((0.0, 1.0), (-1.0, 1.0), (1.0, 0.0), (np.inf, 1.0), (1.0, np.nan), (1.0, -np.inf)):
        assert _code(tr.solve_many, good + [(cp, cn, 0)]) == INVALID
    for h in (-2, 256, 1 << 30):
        assert _code(tr.solve_many, good + [(1.0, 1.0, h)]) == INVALID
    for eps in (0.0, -1e-6, np.nan, np.inf):
        assert _code(tr.solve_many, good, eps) == INVALID
    assert _code(tr.solve_many, good, 1e-6, -1) == INVALID
    pr = (abi.lm_train_problem * 2)(abi.lm_train_problem(1.0, 1.0, -1, 0), abi.lm_train_problem(1.0, 1.0, 0, 1))
    assert _raw_solve_many(tr, pr, 2) == INVALID  # reserved != 0
    pr[1].reserved = 0
    assert _raw_solve_many(tr, pr, 2) == abi.LM_OK
    for null in ("ctx", "problems", "W", "rho"):
        assert _raw_solve_many(tr, pr, 2, null=null) == INVALID
    assert runtime.lib().lm_train_set_groups(tr._h, None, 40) == INVALID
    assert runtime.lib().lm_train_set_groups(None, groups.ctypes.data, 40) == INVALID
    assert _raw_solve_many(tr, pr, 0) == INVALID and _raw_solve_many(tr, pr, -1) == INVALID
    unchanged()
    # a held-out group that holds every stored sample
    tr.set_groups(np.full(40, 9))
    assert _code(tr.solve_many, [(1.0, 1.0, 9)]) == INVALID
    assert same(results(tr.solve_many([(1.0, 1.0, 8)], EPS, 200))[0][:3], want_plain[0][:3])  # an empty group is fine
    tr.set_groups(groups)
    unchanged()
    # one class left is allowed
    tr.set_groups((y < 0).astype(np.int32))
    one_class = results(tr.solve_many([(1.0, 1.0, 1)], EPS, 200))[0]
    assert one_class[2]["converged"] == 1 and one_class[3]["n_pos"] == 0 and one_class[3]["n_neg"] == int((y < 0).sum())
    # the groups are forgotten by add_patches and by reset
    tr.set_groups(groups)
    tr.add_patches(P[:2], y[:2])
    assert _code(tr.solve_many, [(1.0, 1.0, 0)]) == INVALID
    assert _code(tr.set_groups, groups) == INVALID  # 42 samples now
    tr.set_groups(CV.company_groups(42))
    assert results(tr.solve_many([(1.0, 1.0, 0)], EPS, 200))[0][2]["converged"] == 1
    tr.reset()
    assert _code(tr.solve_many, good) == INVALID
    tr.add_patches(P, y)
    assert _code(tr.solve_many, [(1.0, 1.0, 0)]) == INVALID
    for w, r in zip(want_plain, results(tr.solve_many(good, EPS, 200))):
        assert same(w, r)
    tr.close()


# --------------------------------------------------------- 7: the program

def paw_centres(cfg, f):
    """Image (x, y) of the four bottom-view paws of synthetic frame f (synth_frame's px, py)."""
    sc = S.scene(cfg.rows, cfg.cols)
    s = sc["scale"]
    cx = sc["cx0"] + s * S.tri(f, 50, 40)
    pts = []
    for k in range(4):
        px = cx + (-110, -40, 40, 110)[k] * s + s * S.tri(f + 5 * k, 20, 30)
        py = sc["bottom_cy"] + (58 if (k & 1) else -58) * s
        pts.append((cfg.cols - 1 - px if cfg.setup.flip else px, py))
    return pts


def run_train(args, env=None):
    e = {k: v for k, v in os.environ.items() if not k.startswith("LM_")}
    e.update(env or {})
    p = subprocess.run([runtime.TRAIN_CLI_PATH, *map(str, args)], capture_output=True, text=True, env=e, timeout=300)
    return p.returncode, p.stdout


@pytest.fixture(scope="module")
def program_inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("train_cv_cli")
    cfg = S.SyntheticConfig()
    paths = MW.write_inputs(str(d), cfg, 24)
    labels = [(f, x, y) for f in range(24) for x, y in paw_centres(cfg, f)]
    with open(d / "labels.yml", "w") as fh:
        fh.write("%YAML:1.0\n---\n" + MW.yaml_matrix("labels_paw_bottom", np.array(labels, np.int32), "i"))
    args = [paths["config"], paths["video"], paths["background"], paths["calibration"], "R", str(d / "labels.yml"),
            paths["model"]]
    return cfg, d, args, labels


ROW = re.compile(r" scale (\S+): missed (\d+)/(\d+) positives, (\d+)/(\d+) negatives, score (\S+);")


def test_program_chooses_the_costs_by_cross_validation(program_inputs):
    cfg, d, args, labels = program_inputs
    scales, folds = [0.01, 1.0, 100.0], 3
    out = str(d / "model_cv.yml")
    rc, text = run_train(args + [out, "paw_bottom"],
                         {"LM_TRAIN": "10:1:1e-6:0:60", "LM_TRAIN_CV": "3:0.01,1,100", "LM_TIMING": "1"})
    print(text)
    assert rc == 0, text
    assert "paw_bottom: 96 positives, 1440 initial negatives, mined none" in text and " cv_ms " in text
    line = [l for l in text.splitlines() if l.startswith("paw_bottom cv: ")]
    assert len(line) == 1 and line[0].startswith("paw_bottom cv: 3 folds;"), text
    printed = [(float(m[0]), int(m[2]), int(m[4]), int(m[1]), int(m[3]), float(m[5])) for m in ROW.findall(line[0])]
    chosen = float(re.search(r"; chosen scale (\S+)$", line[0]).group(1))
    # the same samples in the same order, through the Trainer
    vb = cfg.setup.view_box_bottom
    neg = [q for f in range(24) for q in R.initial_negatives(0, f, labels, (vb.x, vb.y, vb.width, vb.height), cfg.rows,
                                                             cfg.cols, 6, 60)]
    pts = [(f, x, y, 1) for f, x, y in labels] + [(f, x, y, -1) for f, x, y in neg]
    ctx = runtime.Context(cfg, max_batch=24)
    tr = runtime.Trainer(24, 24, len(pts))
    tr.gather(ctx, cfg.frames(0, 24), pts)
    fold = CV.ref_folds([p[0] for p in pts], folds)
    assert np.array_equal(fold, CV.folds([p[0] for p in pts], folds))
    tr.set_groups(fold)
    held = tr.solve_many([(10.0 * s, 1.0 * s, f) for f in range(folds) for s in scales], 1e-6, 200)[3]
    tr.close()
    ctx.close()
    rows = CV.pooled(held, len(scales))
    assert all(tuple(r[:2]) == (96, 1440) for r in rows)  # every sample is held out exactly once
    best = CV.ref_select(scales, rows)
    assert [p[:5] for p in printed] == [(s, *map(int, r)) for s, r in zip(scales, rows)], (printed, rows)
    for p, r in zip(printed, rows):
        assert p[5] == pytest.approx(float(CV.ref_score(r)), rel=1e-5, abs=1e-12)  # (printed with six digits)
    assert chosen == scales[best]
    # the detector is the one LM_TRAIN with the chosen costs gives, to the bit; the other five are untouched
    plain = str(d / "model_plain.yml")
    rc, text2 = run_train(args + [plain, "paw_bottom"], {"LM_TRAIN": f"{10.0 * chosen!r}:{1.0 * chosen!r}:1e-6:0:60"})
    assert rc == 0 and "paw_bottom cv:" not in text2, text2
    w, b = TH.load_model(out)
    w2, b2 = TH.load_model(plain)
    assert np.array_equal(w["paw_bottom"].view(np.uint64), w2["paw_bottom"].view(np.uint64))
    assert b["paw_bottom"] == b2["paw_bottom"]
    for name in cfg.weights:
        if name != "paw_bottom":
            assert np.array_equal(w[name].view(np.uint64), cfg.weights[name].view(np.uint64)) and b[name] == cfg.biases[name]


@pytest.mark.parametrize("spec", ["25:1", "3:"])
def test_program_refuses_a_malformed_knob(program_inputs, spec):
    cfg, d, args, labels = program_inputs
    rc, text = run_train(args + [str(d / "model_bad.yml"), "paw_bottom"], {"LM_TRAIN_CV": spec})
    assert rc == 1 and text.startswith("Invalid inputs: LM_TRAIN_CV:"), text
