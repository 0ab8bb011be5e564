#!/usr/bin/env python3
"""Rate of the detector training (lm_train_*) on one GPU.

A 65,536 x 576 (24 x 24) and a 65,536 x 900 (30 x 30) sample set are
gathered from 256 synthetic frames resident in HBM (lm_synth_frames_device,
lm_train_gather_device): the four bottom-view paws of every frame as
positives, 252 points of a fixed sequence in the bottom view box as
negatives.  Both matrices fit the 256 MB last-level cache.  Per set: the wall
time of lm_train_solve (C+ = 10, C- = 1, eps = 1e-6; the best and the mean of
--steps solves after --warmup), its outer and CG iteration counts, the time
per pass over the matrix (the solve's time over its passes: 3 per outer
iteration and 2 per CG step, everything else included) against the matrix
bytes, lm_train_margins (one pass, with its copies), and the same solve by the
numpy restatement (tests/train_ref.py) on the host's threads.

--work: the share of the bright point-detector tiles the tile bound lists for
computing (lm_debug_point_work) on a 64-frame C3 batch, with the hand-made
paw_bottom detector and with one trained here on frames 0-23 (the end-to-end
test's samples).

Writes profiles/train/rate.json (or --out) and prints the same JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def paw_centres(S, cfg, f):
    sc = S.scene(cfg.rows, cfg.cols)
    cx = sc["cx0"] + S.tri(f, 50, 40)
    return [(cx + (-110, -40, 40, 110)[k] + S.tri(f + 5 * k, 20, 30), sc["bottom_cy"] + (58 if k & 1 else -58))
            for k in range(4)]


def points_of(S, cfg, n_frames, per_frame, r_neg):
    import numpy as np
    import train_ref as R
    vb = cfg.setup.view_box_bottom
    pts = []
    for f in range(n_frames):
        lab = [(f, x, y) for x, y in paw_centres(S, cfg, f)]
        neg = R.initial_negatives(0, f, lab, (vb.x, vb.y, vb.width, vb.height), cfg.rows, cfg.cols, r_neg, per_frame - 4)
        pts += [(f, x, y, 1) for _, x, y in lab] + [(f, x, y, -1) for _, x, y in neg]
    return np.array(pts, np.int32)


def measure_set(args, kh, kw):
    import numpy as np
    import torch
    import train_ref as R

    from locomouse_cpp_amd import runtime
    from locomouse_cpp_amd import synthetic as S
    cfg = S.SyntheticConfig()
    n_frames, per_frame, chunk = args.frames, args.samples // args.frames, 64
    pitch = cfg.rows * cfg.cols
    d = torch.empty(n_frames * pitch, dtype=torch.uint8, device="cuda:0")
    runtime.synth_frames_device(d.data_ptr(), cfg.rows, cfg.cols, 0, n_frames, pitch)
    torch.cuda.synchronize()
    ctx = runtime.Context(cfg, max_batch=chunk)
    pts = points_of(S, cfg, n_frames, per_frame, max(kh, kw) // 4)
    tr = runtime.Trainer(kh, kw, len(pts))
    t0 = time.perf_counter()
    for f0 in range(0, n_frames, chunk):
        sel = pts[(pts[:, 0] >= f0) & (pts[:, 0] < f0 + chunk)].copy()
        sel[:, 0] -= f0
        tr.gather_device(ctx, d.data_ptr() + f0 * pitch, pitch, min(chunk, n_frames - f0), sel)
    gather_s = time.perf_counter() - t0
    n, D = len(pts), kh * kw
    Dp = (D + 15) // 16 * 16
    times, st = [], None
    for i in range(args.warmup + args.steps):
        t0 = time.perf_counter()
        W, rho, st = tr.solve(10.0, 1.0, 1e-6, 200)
        if i >= args.warmup:
            times.append(time.perf_counter() - t0)
    passes = 3 * st["outer_iters"] + 2 * st["cg_iters"] + 2
    mt = []
    for i in range(3):
        t0 = time.perf_counter()
        z = tr.margins(W, rho)
        mt.append(time.perf_counter() - t0)
    P, y = tr.patches()
    P = P.reshape(n, D)
    tr.close()
    ctx.close()
    # the check the timing rests on: numpy's gradient at the returned point
    Xt = R.xtilde(P)
    wb = np.append(W.reshape(-1) * 255.0, -rho)
    F, g, a, sF, sg = R.objective(Xt, y, 10.0, 1.0, wb)
    ok = bool(np.linalg.norm(g) <= 1e-6 * st["grad_norm0"] + np.linalg.norm(sg) and abs(F - st["objective"]) <= sF
              and np.allclose(z, Xt @ wb, rtol=0, atol=1e-9))
    out = {
        "kh": kh, "kw": kw, "samples": n, "positives": int((y > 0).sum()), "matrix_bytes": n * Dp,
        "gather_s": gather_s, "solve_ms": {"best": 1e3 * min(times), "mean": 1e3 * sum(times) / len(times)},
        "outer_iters": st["outer_iters"], "cg_iters": st["cg_iters"], "n_active": st["n_active"],
        "objective": st["objective"], "grad_norm": st["grad_norm"], "grad_norm0": st["grad_norm0"],
        "matrix_passes": passes, "ms_per_pass": 1e3 * min(times) / passes,
        "matrix_GB_per_s": n * Dp / (min(times) / passes) / 1e9,
        "margins_ms": 1e3 * min(mt), "numpy_gradient_check": ok,
    }
    if not args.no_numpy:
        t0 = time.perf_counter()
        w_np, b_np, st_np = R.solve(P, y, 10.0, 1.0, 1e-6, 200)
        out["numpy_solve_s"] = time.perf_counter() - t0
        out["numpy_threads"] = int(os.environ.get("OMP_NUM_THREADS", "0")) or None
        out["numpy_outer_iters"], out["numpy_cg_iters"] = st_np["outer_iters"], st_np["cg_iters"]
        out["numpy_distance"] = float(np.linalg.norm(np.append(w_np, b_np) - wb))
    return out


def measure_work():
    import numpy as np

    from locomouse_cpp_amd import runtime
    from locomouse_cpp_amd import synthetic as S
    base = S.SyntheticConfig()
    frames = base.frames(0, 24)
    rng = np.random.default_rng(5)
    vb = base.setup.view_box_bottom
    pts = []
    for f in range(24):
        paws = paw_centres(S, base, f)
        pts += [(f, x, y, 1) for x, y in paws]
        k = 0
        while k < 60:
            x, y = int(rng.integers(vb.x, vb.x + vb.width)), int(rng.integers(vb.y, vb.y + vb.height))
            if all(max(abs(x - px), abs(y - py)) >= 6 for px, py in paws):
                pts.append((f, x, y, -1))
                k += 1
    ctx = runtime.Context(base, max_batch=24)
    tr = runtime.Trainer(24, 24, len(pts))
    tr.gather(ctx, frames, pts)
    W, rho, st = tr.solve(10.0, 1.0, 1e-6, 200)
    tr.close()
    ctx.close()
    out = {}
    batch = base.frames(0, 64)
    for name, cfg in (("hand_made", base),
                      ("trained_paw_bottom", S.SyntheticConfig(weights={"paw_bottom": W}, biases={"paw_bottom": rho}))):
        c = runtime.Context(cfg, max_batch=64)
        c.detect(batch, 0)
        w = c.point_work()
        c.close()
        out[name] = None if w is None else {
            "listed": list(w["listed"]), "bright": list(w["bright"]),
            "share": [l / b if b else None for l, b in zip(w["listed"], w["bright"])],
            "order": ["paw_bottom", "snout_bottom", "paw_side", "snout_side"]}
    out["solver"] = st
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=65536)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sizes", default="24x24,30x30")
    ap.add_argument("--no-numpy", action="store_true", help="skip the numpy restatement's solve")
    ap.add_argument("--work", action="store_true", help="also the listed-tile share of a trained detector")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train", "rate.json"))
    args = ap.parse_args()
    line = {"metric": "detector training, lm_train_solve wall time", "unit": "ms", "higher_is_better": False,
            "data": "gathered synthetic patches (lm_synth.h scene), C+ 10, C- 1, eps 1e-6", "sets": []}
    for size in args.sizes.split(","):
        kh, kw = map(int, size.split("x"))
        line["sets"].append(measure_set(args, kh, kw))
    line["value"] = line["sets"][0]["solve_ms"]["best"]
    if args.work:
        line["point_work_64_frames"] = measure_work()
    if not all(s["numpy_gradient_check"] for s in line["sets"]):
        raise SystemExit("numpy's gradient at the returned point is not small: " + json.dumps(line))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(line, fh, indent=1)
        fh.write("\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
