#!/usr/bin/env python3
"""Rate of the SVM solver with many problems in one call (lm_train_solve_many)
against the same problems as one-problem calls in turn (lm_train_solve, which
is that: there is one solver) on one GPU: the comparison that justifies
batching.

The sample sets are those of scripts/train_rate.py, gathered the same way: the
65,536 x 576 (24 x 24) and 65,536 x 900 (30 x 30) sets from 256 synthetic
frames, and the 1,536 x 576 set of the end-to-end test's size from 24 frames.
Per set, for 1, PB (lm_train_problem_block), 8 and 40 problems without a
held-out group, with the costs (10, 1) times scales spread geometrically over
0.01 .. 100 (one problem: scale 1):

  many_ms   the wall time of one lm_train_solve_many call;
  single_ms the same problems as one-problem calls in turn: the sum of the
            wall times of lm_train_solve over them, in the same process;

each the best of --steps after --warmup.  The two return the same bits, which
is checked here.  Then a real cross-validation call: 5 folds by frame x the 8
scales 0.01, 0.1, 0.3, 1, 3, 10, 30, 100, with its pooled table.

Writes profiles/traincv/rate.json (or --out) and prints the same JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def best_of(fn, warmup, steps):
    times, out = [], None
    for i in range(warmup + steps):
        t0 = time.perf_counter()
        out = fn()
        if i >= warmup:
            times.append(time.perf_counter() - t0)
    return 1e3 * min(times), out


def measure_set(args, kh, kw, n_frames, samples):
    import numpy as np
    import torch
    import train_cv_harness as CV
    import train_rate as TR

    from locomouse_cpp_amd import runtime
    from locomouse_cpp_amd import synthetic as S
    cfg = S.SyntheticConfig()
    per_frame, chunk = samples // n_frames, 64
    pitch = cfg.rows * cfg.cols
    d = torch.empty(n_frames * pitch, dtype=torch.uint8, device="cuda:0")
    runtime.synth_frames_device(d.data_ptr(), cfg.rows, cfg.cols, 0, n_frames, pitch)
    torch.cuda.synchronize()
    ctx = runtime.Context(cfg, max_batch=chunk)
    pts = TR.points_of(S, cfg, n_frames, per_frame, max(kh, kw) // 4)
    tr = runtime.Trainer(kh, kw, len(pts))
    for f0 in range(0, n_frames, chunk):
        sel = pts[(pts[:, 0] >= f0) & (pts[:, 0] < f0 + chunk)].copy()
        sel[:, 0] -= f0
        tr.gather_device(ctx, d.data_ptr() + f0 * pitch, pitch, min(chunk, n_frames - f0), sel)
    pb = tr.problem_block()
    out = {"kh": kh, "kw": kw, "samples": len(pts), "problem_block": pb, "calls": []}
    for n in sorted({1, pb, 8, 40}):
        scales = [1.0] if n == 1 else [float(s) for s in np.geomspace(0.01, 100.0, n)]
        problems = [(10.0 * s, 1.0 * s, -1) for s in scales]
        many_ms, many = best_of(lambda: tr.solve_many(problems, 1e-6, 200), args.warmup, args.steps)
        single_ms, single = best_of(lambda: [tr.solve(cp, cn, 1e-6, 200) for cp, cn, _ in problems], args.warmup, args.steps)
        same = all(np.array_equal(many[0][q].view(np.uint64), single[q][0].view(np.uint64)) and many[1][q] == single[q][1]
                   and many[2][q] == single[q][2] for q in range(n))
        out["calls"].append({
            "problems": n, "many_ms": many_ms, "single_ms": single_ms, "single_over_many": single_ms / many_ms,
            "bit_identical": bool(same), "outer_iters": [s["outer_iters"] for s in many[2]],
            "cg_iters": [s["cg_iters"] for s in many[2]], "converged": [s["converged"] for s in many[2]]})
        print(f"{kh}x{kw} N={len(pts)} problems={n}: many {many_ms:.1f} ms, single {single_ms:.1f} ms", file=sys.stderr,
              flush=True)
    # a real cross-validation: 5 folds by frame x 8 scales
    folds = 5
    tr.set_groups(CV.ref_folds(pts[:, 0], folds))
    problems = [(10.0 * s, 1.0 * s, f) for f in range(folds) for s in CV.SCALES]
    cv_ms, cv = best_of(lambda: tr.solve_many(problems, 1e-6, 200), args.warmup, args.steps)
    rows = CV.pooled(cv[3], len(CV.SCALES))
    out["cross_validation"] = {
        "folds": folds, "scales": list(CV.SCALES), "many_ms": cv_ms,
        "rows_n_pos_n_neg_miss_pos_miss_neg": rows.tolist(), "score": [float(CV.ref_score(r)) for r in rows],
        "chosen_scale": CV.SCALES[CV.ref_select(CV.SCALES, rows)], "outer_iters": [s["outer_iters"] for s in cv[2]],
        "cg_iters": [s["cg_iters"] for s in cv[2]], "converged": [s["converged"] for s in cv[2]]}
    tr.close()
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sets", default="24x24:256:65536,30x30:256:65536,24x24:24:1536", help="khxkw:frames:samples,...")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "traincv", "rate.json"))
    args = ap.parse_args()
    line = {"metric": "lm_train_solve_many against lm_train_solve in turn, wall time", "unit": "ms",
            "higher_is_better": False,
            "data": "gathered synthetic patches (lm_synth.h scene), costs (10, 1) x scale, eps 1e-6", "sets": []}
    for spec in args.sets.split(","):
        size, frames, samples = spec.split(":")
        kh, kw = map(int, size.split("x"))
        line["sets"].append(measure_set(args, kh, kw, int(frames), int(samples)))
    line["value"] = line["sets"][0]["calls"][-1]["many_ms"]
    if not all(c["bit_identical"] for s in line["sets"] for c in s["calls"]):
        raise SystemExit("a call of many problems and its problems in turn differ: " + json.dumps(line))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(line, fh, indent=1)
        fh.write("\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
