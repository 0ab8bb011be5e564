"""Detector training on the GPU (include/locomouse_train.h, csrc/lm_train.hip).

The gather is compared byte for byte with cuts from the oracle's I_PAD, and
its anchor is pinned through the oracle's score maps.  The solver is tested
against the definition alone: F is 1-strongly convex, so a point's distance
from the minimiser is at most |grad F| there, and numpy float64
(tests/train_ref.py) recomputes F and grad F at the returned point; the only
tolerances are the fp64 rounding bounds of those evaluations, computed from
the data.

Solver cases: every (kh, kw) x N of the table below with the data kinds
taken in turn, every data kind at every (kh, kw) with N = 65 and at 24 x 24
with N = 1000, N = 4096 at 24 x 24, and N one below, at and one above the
sample block of the X^T u kernel."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edge_scenes as E  # noqa: E402
import media_writers as MW  # noqa: E402
import train_harness as TH  # noqa: E402
import train_ref as R  # noqa: E402

from locomouse_cpp_amd import abi, runtime  # noqa: E402
from locomouse_cpp_amd import synthetic as S  # noqa: E402
from oracle import oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 1e-8
INVALID = abi.LM_ERR_INVALID_ARGUMENT


# ------------------------------------------------------------------ gather

def ipad_cut(ipad, g, x, y, kh, kw):
    """The kh x kw taps of image point (x, y) in I_PAD, zero outside it."""
    out = np.zeros((kh, kw), np.uint8)
    r0, c0 = g.pad_pre_rows + y - kh // 2, g.pad_pre_cols + x - kw // 2
    for i in range(kh):
        r = r0 + i
        if 0 <= r < ipad.shape[0]:
            lo, hi = max(c0, 0), min(c0 + kw, ipad.shape[1])
            if lo < hi:
                out[i, lo - c0:hi - c0] = ipad[r, lo:hi]
    return out


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


def gather_points(cfg):
    """(frame, x, y, label): paws of frames 0 and 2, the view boundary, the
    image corners and edges (taps outside the image), the mouse's body."""
    pts = [(f, x, y, 1) for f in (0, 2) for x, y in paw_centres(cfg, f)]
    b = cfg.setup.view_box_bottom.y
    pts += [(0, 500, b - 1, -1), (0, 500, b, -1), (2, 0, b, -1), (2, cfg.cols - 1, b - 1, -1)]
    pts += [(0, 0, 0, -1), (0, cfg.cols - 1, 0, -1), (2, 0, cfg.rows - 1, -1), (2, cfg.cols - 1, cfg.rows - 1, -1),
            (1, 3, 5, -1), (1, cfg.cols - 4, cfg.rows - 2, -1)]
    pts += [(1, 520, 176, -1), (2, 400, 48, 1)]
    return np.array(pts, np.int32)


@pytest.fixture(scope="module", params=[{}, {"flip": True}, {"method": 1}], ids=["default", "flipped", "method1"])
def scene(request):
    cfg = S.SyntheticConfig(**request.param)
    frames = cfg.frames(0, 3)
    run = O.OracleRun(cfg, frames, flags=O.KEEP_DEBUG)
    g = O.geometry(cfg)
    ipads = [run.ipad(f, (g.ipad_rows, g.ipad_cols)) for f in range(3)]
    ctx = runtime.Context(cfg, max_batch=4)
    yield cfg, frames, run, g, ipads, ctx
    ctx.close()


@pytest.mark.parametrize("size", [(24, 24), (16, 26), (5, 7), (1, 1), (64, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_gather_equals_the_oracles_ipad(scene, size):
    cfg, frames, run, g, ipads, ctx = scene
    kh, kw = size
    pts = gather_points(cfg)
    tr = runtime.Trainer(kh, kw, 2 * len(pts))
    tr.gather(ctx, frames, pts)
    assert tr.samples() == (int((pts[:, 3] > 0).sum()), int((pts[:, 3] < 0).sum()))
    got, lab = tr.patches()
    assert np.array_equal(lab, pts[:, 3])
    for k, (f, x, y, _) in enumerate(pts):
        assert np.array_equal(got[k], ipad_cut(ipads[f], g, x, y, kh, kw)), (k, f, x, y)
    # frames in device memory (an unaligned base: they are staged), appended to the same context
    import torch
    d = torch.zeros(frames.size + 1, dtype=torch.uint8, device="cuda")
    d[1:] = torch.from_numpy(frames.reshape(-1)).cuda()
    torch.cuda.synchronize()
    tr.gather_device(ctx, d.data_ptr() + 1, frames.shape[1] * frames.shape[2], 3, pts)
    again, _ = tr.patches(len(pts), len(pts))
    assert np.array_equal(again, got)
    tr.close()


def test_gathered_patch_scores_like_the_detector(scene):
    """The fp32 fused chain over a gathered patch equals the oracle's score at
    that point, bit for bit: the anchor is kh/2, kw/2 and the taps are in
    filter2D's order."""
    cfg, frames, run, g, ipads, ctx = scene
    p = cfg.params
    names = ("paw_bottom", "snout_bottom", "tail_bottom", "paw_side", "snout_side", "tail_side")
    for det in (0, 2, 3):
        W, rho = cfg.weights[names[det]], cfg.biases[names[det]]
        # image coordinates of output (0, 0): the crop origin of the provided box
        # (cropBoundingBox) plus the unpadding, as tests/test_oracle.py places the maps
        if det < 3:
            box = p.bounding_box_bottom
            x0 = box.x + box.width + g.pad_pre_cols - (g.bb_bottom_mouse_pad.width - g.spost_b_w) + 1 + g.spre_b_w
            y0 = box.y + box.height + g.pad_pre_rows - (g.bb_bottom_mouse_pad.height - g.spost_b_h) + 1 + g.spre_b_h
        else:
            box = p.bounding_box_side
            x0 = g.pad_pre_cols + box.x + box.width - (g.bb_side_mouse_pad.width - g.spost_t_w) + 1 + g.spre_t_w
            y0 = g.pad_pre_rows + box.y + box.height - (g.bb_side_mouse_pad.height - g.spost_t_h) + 1 + g.spre_t_h
        x0, y0 = x0 - g.pad_pre_cols, y0 - g.pad_pre_rows
        pts = []
        for f in (0, 2):
            sc = run.scores(f, det)
            assert sc is not None
            oh, ow = sc.shape
            cells = [(0, 0), (oh - 1, ow - 1), (oh // 2, ow // 3), (7, ow - 2)]
            if det == 0:
                cells += [(y - y0, x - x0) for x, y in paw_centres(cfg, f) if 0 <= y - y0 < oh and 0 <= x - x0 < ow]
                assert len(cells) > 4
            pts += [(f, x0 + ox, y0 + oy, 1, float(sc[oy, ox])) for oy, ox in cells]
        tr = runtime.Trainer(W.shape[0], W.shape[1], len(pts))
        tr.gather(ctx, frames, np.array([q[:4] for q in pts], np.int32))
        got, _ = tr.patches()
        for k, q in enumerate(pts):
            want = np.float32(q[4])
            assert TH.fused_score(got[k], W, rho).view(np.uint32) == want.view(np.uint32), (det, q)
        tr.close()


# ------------------------------------------------------------------ solver

SIZES = ((1, 1), (5, 7), (16, 26), (24, 24), (30, 30))
NS = (1, 2, 63, 64, 65, 1000)
XT_BLOCK = 1024


def solver_cases():
    cases = []
    for si, size in enumerate(SIZES):
        for ni, n in enumerate(NS):
            cases.append((size, n, TH.KINDS[(si + ni) % len(TH.KINDS)]))
    cases.append(((64, 64), 70, "overlapping"))
    for size in SIZES + ((64, 64),):
        for kind in TH.KINDS:
            if (size, 65, kind) not in cases:
                cases.append((size, 65 if size != (64, 64) else 70, kind))
    for kind in TH.KINDS:
        if ((24, 24), 1000, kind) not in cases:
            cases.append(((24, 24), 1000, kind))
    cases.append(((24, 24), 4096, "overlapping"))
    for n in (XT_BLOCK - 1, XT_BLOCK, XT_BLOCK + 1):
        cases.append(((5, 7), n, "costs"))
    return list(dict.fromkeys(cases))


def solve_on_gpu(P, y, kh, kw, cp, cn, max_samples):
    tr = runtime.Trainer(kh, kw, max_samples)
    h = len(y) // 2  # in two adds
    if h:
        tr.add_patches(P[:h], y[:h])
    tr.add_patches(P[h:], y[h:])
    W, rho, st = tr.solve(cp, cn, EPS, 200)
    return tr, W, rho, st


@pytest.mark.parametrize("size,n,kind", solver_cases(), ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_solver_reaches_the_minimiser(size, n, kind):
    from scipy.optimize import minimize
    kh, kw = size
    d = kh * kw
    P, y = TH.sample_set(kind, n, d)
    cp, cn = TH.kind_costs(kind)
    tr, W, rho, st = solve_on_gpu(P, y, kh, kw, cp, cn, n)
    assert TH.lib().th_xt_block() == XT_BLOCK
    Xt = R.xtilde(P)
    wb = np.append(W.reshape(-1) * 255.0, -rho)
    F, g, a, sF, sg = R.objective(Xt, y, cp, cn, wb)
    g0 = float(np.linalg.norm(R.objective(Xt, y, cp, cn, np.zeros(d + 1))[1]))
    gn, s = float(np.linalg.norm(g)), float(np.linalg.norm(sg))
    print(f"{kh}x{kw} N={n} {kind}: |g|={gn:.3e} eps|g0|={EPS * g0:.3e} s={s:.3e} F={F!r} dF={st['objective'] - F:.3e} "
          f"sF={sF:.3e} outer={st['outer_iters']} cg={st['cg_iters']} active={st['n_active']}")
    assert st["converged"] == 1, st
    assert gn <= EPS * g0 + s  # 1
    assert abs(st["objective"] - F) <= sF  # 2
    assert abs(st["grad_norm0"] - g0) <= (n + d + 2) * 2.0 ** -52 * 2 * float(np.linalg.norm(np.abs(Xt).T @ R.costs(y, cp, cn)))
    # 3: the margins of the returned model, and of another
    Xl, wl = Xt.astype(np.longdouble), wb.astype(np.longdouble)
    bound = 2 * (d + 1) * 2.0 ** -53 * (np.abs(Xt) @ np.abs(wb))
    z = tr.margins(W, rho)
    assert np.all(np.abs(z - (Xl @ wl).astype(np.float64)) <= bound)
    # 4: bit-identical again, and in a context with room for more samples
    W2, rho2, st2 = tr.solve(cp, cn, EPS, 200)
    assert np.array_equal(W2.view(np.uint64), W.view(np.uint64)) and rho2 == rho and st2 == st
    tr.close()
    tr3, W3, rho3, st3 = solve_on_gpu(P, y, kh, kw, cp, cn, 3 * n + 1000)
    assert np.array_equal(W3.view(np.uint64), W.view(np.uint64)) and rho3 == rho and st3 == st
    tr3.close()
    # 5: an independent minimiser lands within the two gradient norms of it
    res = minimize(lambda v: R.objective(Xt, y, cp, cn, v)[:2], np.zeros(d + 1), jac=True, method="L-BFGS-B",
                   options={"ftol": 0.0, "gtol": 0.0, "maxiter": 4000 if n * d <= 100000 else 1200, "maxfun": 100000,
                            "maxcor": 30})
    gs = float(np.linalg.norm(R.objective(Xt, y, cp, cn, res.x)[1]))
    assert np.linalg.norm(res.x - wb) <= gs + gn, (gs, gn)


def test_max_iter_returns_ok_unconverged():
    P, y = TH.sample_set("overlapping", 200, 35)
    tr = runtime.Trainer(5, 7, 200)
    tr.add_patches(P, y)
    W, rho, st = tr.solve(1.0, 1.0, 1e-12, 1)
    assert st["converged"] == 0 and st["outer_iters"] == 1 and st["grad_norm"] < st["grad_norm0"]
    wb = np.append(W.reshape(-1) * 255.0, -rho)
    F, g, a, sF, sg = R.objective(R.xtilde(P), y, 1.0, 1.0, wb)
    assert abs(st["objective"] - F) <= sF and abs(st["grad_norm"] - np.linalg.norm(g)) <= np.linalg.norm(sg)
    W0, rho0, st0 = tr.solve(1.0, 1.0, 1e-12, 0)
    assert not W0.any() and rho0 == 0 and st0["outer_iters"] == 0 and st0["grad_norm"] == st0["grad_norm0"]
    tr.close()


# ---------------------------------------------------------------- refusals

def _code(fn, *args):
    with pytest.raises(runtime.LMError) as e:
        fn(*args)
    return e.value.code


def test_refusals_add_nothing():
    P, y = TH.sample_set("overlapping", 10, 35)
    tr = runtime.Trainer(5, 7, 12)
    assert _code(tr.solve) == INVALID  # empty
    assert _code(tr.margins, np.zeros((5, 7)), 0.0) == INVALID
    tr.add_patches(P, y)
    before = tr.patches()
    assert _code(tr.add_patches, P[:3], y[:3]) == INVALID  # 10 + 3 > 12
    for bad in (0, 2, -2, 127):
        lab = np.array(y[:2])
        lab[1] = bad
        assert _code(tr.add_patches, P[:2], lab) == INVALID
    for cp, cn, eps in ((0.0, 1.0, 1e-6), (-1.0, 1.0, 1e-6), (1.0, 0.0, 1e-6), (np.inf, 1.0, 1e-6), (1.0, np.nan, 1e-6),
                        (1.0, 1.0, 0.0), (1.0, 1.0, -1e-6), (1.0, 1.0, np.nan), (1.0, 1.0, np.inf)):
        assert _code(tr.solve, cp, cn, eps) == INVALID
    assert tr.samples() == (int((y > 0).sum()), int((y < 0).sum()))
    after = tr.patches()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    tr.add_patches(P[:2], y[:2])  # exactly full is fine
    assert sum(tr.samples()) == 12
    tr.reset()
    assert tr.samples() == (0, 0) and _code(tr.solve) == INVALID
    tr.close()


def test_gather_refusals_add_nothing():
    cfg = S.SyntheticConfig()
    frames = cfg.frames(0, 2)
    ctx = runtime.Context(cfg, max_batch=2)
    tr = runtime.Trainer(24, 24, 6)
    good = [(0, 500, 150, 1), (1, 10, 10, -1)]
    tr.gather(ctx, frames, good)
    for bad in ((2, 500, 150, 1), (-1, 500, 150, 1), (0, cfg.cols, 150, 1), (0, -1, 150, 1), (0, 500, cfg.rows, 1),
                (0, 500, -1, -1), (0, 500, 150, 0), (0, 500, 150, 2)):
        assert _code(tr.gather, ctx, frames, good + [bad]) == INVALID
    assert _code(tr.gather, ctx, frames, good * 3) == INVALID  # 2 + 6 > 6
    assert tr.samples() == (1, 1)
    gctx = runtime.Context(E.gray_lut_config(), max_batch=2)  # transform_gray_values on
    assert _code(tr.gather, gctx, frames, good) == INVALID
    assert tr.samples() == (1, 1)
    gctx.close()
    ctx.close()
    tr.close()


# -------------------------------------------------------------- end to end

def paw_hits(res, cfg, first, n):
    """(frame, paw) pairs of frames first .. first + n - 1 with a paw_bottom
    candidate within 3 pixels of the paw's centre, and the candidates per frame."""
    box = cfg.params.bounding_box_bottom
    x0, y0 = box.x + 1, box.y + 1  # corner - width + 1
    hits = total = 0
    for f in range(n):
        lo, hi = int(res["cand_offset"][4 * f]), int(res["cand_offset"][4 * f + 1])
        cx, cy = res["cand"]["x"][lo:hi] + x0, res["cand"]["y"][lo:hi] + y0
        total += hi - lo
        for px, py in paw_centres(cfg, first + f):
            hits += bool(np.any((cx - px) ** 2 + (cy - py) ** 2 <= 9))
    return hits, total / n


def training_points(cfg, n_frames, neg_per_frame=60, r_neg=6, seed=5):
    rng = np.random.default_rng(seed)
    vb = cfg.setup.view_box_bottom
    pts = []
    for f in range(n_frames):
        paws = paw_centres(cfg, f)
        pts += [(f, x, y, 1) for x, y in paws]
        k = 0
        while k < neg_per_frame:
            x, y = int(rng.integers(vb.x, vb.x + vb.width)), int(rng.integers(vb.y, vb.y + vb.height))
            if all(max(abs(x - px), abs(y - py)) >= r_neg for px, py in paws):
                pts.append((f, x, y, -1))
                k += 1
    return np.array(pts, np.int32)


@pytest.fixture(scope="module")
def trained():
    cfg = S.SyntheticConfig()
    frames = cfg.frames(0, 24)
    ctx = runtime.Context(cfg, max_batch=24)
    pts = training_points(cfg, 24)
    tr = runtime.Trainer(24, 24, len(pts))
    tr.gather(ctx, frames, pts)
    W, rho, st = tr.solve(10.0, 1.0, 1e-6, 200)
    tr.close()
    ctx.close()
    assert st["converged"] == 1, st
    return W, rho, st


def test_trained_paw_detector_finds_the_paws(trained):
    W, rho, st = trained
    base = S.SyntheticConfig()
    cfg = S.SyntheticConfig(weights={"paw_bottom": W}, biases={"paw_bottom": rho})
    frames = base.frames(24, 12)
    ref_hand = O.OracleRun(base, frames).result
    ref = O.OracleRun(cfg, frames).result
    ctx = runtime.Context(cfg, max_batch=12)
    got = ctx.detect(frames, 0)
    ctx.close()
    for k in ("cand_offset", "cand", "p22d", "side_y", "side_s", "unary", "pw_jc", "pw_ir", "pw_pr", "tail"):
        x, y = got[k], ref[k]
        assert x.shape == y.shape and (all(np.array_equal(x[n], y[n]) for n in x.dtype.names) if x.dtype.names
                                       else np.array_equal(x, y)), k
    hand, hand_per = paw_hits(ref_hand, base, 24, 12)
    mine, mine_per = paw_hits(got, cfg, 24, 12)
    print(f"hand-made {hand}/48 ({hand_per:.1f} candidates per frame), trained {mine}/48 ({mine_per:.1f}); solver {st}")
    assert mine >= hand


# ------------------------------------------------------------- the program

def run_train(args, env=None):
    import subprocess
    e = {k: v for k, v in os.environ.items() if not k.startswith("LM_")}
    e.update(env or {})
    p = subprocess.run([runtime.TRAIN_CLI_PATH, *map(str, args)], capture_output=True, text=True, env=e, timeout=300)
    return p.returncode, p.stdout


@pytest.fixture(scope="module")
def program_inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("train_cli")
    cfg = S.SyntheticConfig()
    paths = MW.write_inputs(str(d), cfg, 24)
    labels = [(f, x, y) for f in range(24) for x, y in paw_centres(cfg, f)]
    with open(d / "labels.yml", "w") as fh:
        fh.write("%YAML:1.0\n---\n" + MW.yaml_matrix("labels_paw_bottom", np.array(labels, np.int32), "i"))
    args = [paths["config"], paths["video"], paths["background"], paths["calibration"], "R", str(d / "labels.yml"),
            paths["model"]]
    return cfg, d, args, labels


def test_program_trains_the_trainers_detector(program_inputs):
    """LocoMouseTrain without mining rounds writes, to the bit, the detector the
    Trainer gives on the same samples in the same order, and leaves the other
    five as model_in.yml has them."""
    cfg, d, args, labels = program_inputs
    out = str(d / "model_out.yml")
    rc, text = run_train(args + [out, "paw_bottom"], {"LM_TRAIN": "10:1:1e-6:0:60", "LM_TIMING": "1"})
    print(text)
    assert rc == 0, text
    assert "paw_bottom: 96 positives, 1440 initial negatives, mined none" in text and " converged" in text
    assert "LM_TIMING gather_ms " in text and " solve_ms " in text and " mining_ms " in text
    w, b = TH.load_model(out)
    for name in cfg.weights:
        if name != "paw_bottom":
            assert np.array_equal(w[name].view(np.uint64), cfg.weights[name].view(np.uint64)) and b[name] == cfg.biases[name]
    vb = cfg.setup.view_box_bottom
    neg = [q for f in range(24) for q in R.initial_negatives(0, f, labels, (vb.x, vb.y, vb.width, vb.height), cfg.rows,
                                                             cfg.cols, 6, 60)]
    pts = [(f, x, y, 1) for f, x, y in labels] + [(f, x, y, -1) for f, x, y in neg]
    ctx = runtime.Context(cfg, max_batch=24)
    tr = runtime.Trainer(24, 24, len(pts))
    tr.gather(ctx, cfg.frames(0, 24), pts)
    W, rho, st = tr.solve(10.0, 1.0, 1e-6, 200)
    tr.close()
    ctx.close()
    assert np.array_equal(w["paw_bottom"].view(np.uint64), W.view(np.uint64)) and b["paw_bottom"] == rho


def test_program_mines_hard_negatives(program_inputs):
    """Mining, from the worst start: without initial negatives the first
    detector is trained on the paws alone (one class), so it fires all over the
    box, and the candidates away from the labels become the negatives of the
    next solve."""
    import re
    cfg, d, args, labels = program_inputs
    out = str(d / "model_mined.yml")
    rc, text = run_train(args + [out], {"LM_TRAIN": "10:1:1e-6:2:0"})  # every feature labels.yml has: paw_bottom
    print(text)
    assert rc == 0, text
    m = re.search(r"paw_bottom: 96 positives, 0 initial negatives, mined((?: \d+)+);", text)
    assert m and " converged" in text and "NOT converged" not in text, text
    mined = list(map(int, m.group(1).split()))
    assert 1 <= len(mined) <= 2 and mined[0] > 0 and all(k > 0 for k in mined[:-1])
    w, b = TH.load_model(out)
    for name in cfg.weights:
        if name != "paw_bottom":
            assert np.array_equal(w[name].view(np.uint64), cfg.weights[name].view(np.uint64)) and b[name] == cfg.biases[name]
    # the mined negatives count: the paws alone would give a detector that is positive on every labelled patch
    # and almost everywhere else; this one is negative on the body between the paws
    trained = S.SyntheticConfig(weights={"paw_bottom": w["paw_bottom"]}, biases={"paw_bottom": b["paw_bottom"]})
    frames = cfg.frames(24, 12)
    mine, per = paw_hits(O.OracleRun(trained, frames).result, trained, 24, 12)
    print(f"trained from the paws and mined negatives alone: {mine}/48 paws, {per:.1f} candidates per frame")
    run = O.OracleRun(trained, frames[:1], flags=O.KEEP_DEBUG)
    sc = run.scores(0, 0)
    assert (sc > 0).mean() < 0.5
