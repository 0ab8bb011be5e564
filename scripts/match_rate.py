#!/usr/bin/env python3
"""What a matched context (include/locomouse_match.h) costs on one GPU, on the
C3 workload of bench.py (1024x256 synthetic frames resident in HBM, 448-frame
batches).  Two modes, one process each:

  --what spans  one context with LM_GRAPH=0, so that every kernel of the chain
                before the correlation has its own HIP events (a captured chain
                times k_corr only): k_minmax + k_lut, k_match and k_ingest per
                batch over --steps batches after --warmup, for a plain and a
                matched context, each with the provided box and with a box that
                moves per frame (the whole-video bounding-box workload: k_match
                then gathers pixel by pixel), and for a matched context whose
                reference CDF is all zeros (every table entry runs the second
                loop from 0: the worst case of the serial part).
  --what rate   bench.py's own run_stream (8 contexts x 448 frames, captured
                graphs), plain and with runtime.Context creating matched
                contexts, alternating --runs times in this process: the bench
                line with matching on beside the line with it off.

The reference CDF is lm_match_cdf of a synthetic frame's bottom box through a
gamma 0.7 table (a brighter rig).  Writes --out (JSON; rate: one line per run)
and prints the same."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

ROWS, COLS, BATCH = 256, 1024, 448


def reference_cdf(cfg, runtime, np):
    p = cfg.params.bounding_box_bottom
    img = cfg.frames(7, 1)[0][p.y:p.y + p.height, p.x:p.x + p.width]
    gamma = np.floor(255.0 * (np.arange(256) / 255.0) ** 0.7 + 0.5).astype(np.uint8)
    return runtime.match_cdf(np.ascontiguousarray(gamma[img]))


def moving_corners(cfg, np, n, amp=6):
    """Bottom-right corners per frame, a few pixels around the provided boxes (inside the image at C3)."""
    p = cfg.params
    k = np.arange(n)
    dx = (amp * np.sin(k * 0.9)).astype(np.int32)
    dy = (amp // 2 * np.cos(k * 1.3)).astype(np.int32)
    return np.stack([p.bounding_box_bottom.x + p.bounding_box_bottom.width + dx,
                     p.bounding_box_bottom.y + p.bounding_box_bottom.height + dy,
                     p.bounding_box_side.y + p.bounding_box_side.height - dy], 1).astype(np.int32)


def run_spans(a):
    os.environ["LM_GRAPH"] = "0"  # read at the first launch: the chain runs directly, every timed kernel with its events
    import numpy as np
    import torch

    from locomouse_cpp_amd import runtime
    from locomouse_cpp_amd import synthetic as S
    cfg = S.SyntheticConfig(rows=ROWS, cols=COLS)
    B, n_b = BATCH, a.warmup + a.steps
    pitch = ROWS * COLS
    d = torch.empty(n_b * B * pitch, dtype=torch.uint8, device="cuda:0")
    runtime.synth_frames_device(d.data_ptr(), ROWS, COLS, 0, n_b * B, pitch)
    torch.cuda.synchronize()
    ref = reference_cdf(cfg, runtime, np)
    bb = moving_corners(cfg, np, n_b * B)
    cases = [("plain", None, False), ("matched", ref, False), ("plain_moving_box", None, True),
             ("matched_moving_box", ref, True), ("matched_zero_reference", np.zeros(256, np.float32), False)]
    out = {"what": "kernel spans per 448-frame C3 batch, one context, LM_GRAPH=0, microseconds from HIP events",
           "rows": ROWS, "cols": COLS, "batch_frames": B, "steps": a.steps, "warmup": a.warmup,
           "box_bottom": [cfg.params.bounding_box_bottom.width, cfg.params.bounding_box_bottom.height],
           "reference_cdf_last": float(ref[255]), "data": "synthetic (lm_synth.h scene, resident in HBM)", "cases": {}}
    for name, cdf, moving in cases:
        ctx = runtime.Context(cfg, max_batch=B, reference_cdf=cdf)
        ctx.set_debug(2)
        us = {}
        for k in range(n_b):
            ctx.detect_device(d.data_ptr() + k * B * pitch, pitch, B, k * B, bb=bb[k * B:(k + 1) * B] if moving else None)
            if k >= a.warmup:
                for kn, t0, t1 in ctx.kernel_spans():
                    us.setdefault(kn, []).append(1e3 * (t1 - t0))
        ctx.close()
        out["cases"][name] = {kn: {"mean": round(sum(v) / len(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
                              for kn, v in us.items()}
        out["cases"][name]["all_timed_kernels_mean"] = round(sum(sum(v) / len(v) for v in us.values()), 2)
        print(name, json.dumps(out["cases"][name]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


def run_rate(a):
    import functools

    import numpy as np
    import torch

    import bench
    from locomouse_cpp_amd import runtime
    from locomouse_cpp_amd import synthetic as S
    torch.cuda.set_device(0)
    ref = reference_cdf(S.SyntheticConfig(rows=ROWS, cols=COLS), runtime, np)
    plain = runtime.Context
    matched = functools.partial(plain, reference_cdf=ref)
    args = argparse.Namespace(gpus=1, steps=a.steps, warmup=a.warmup, config="c3", precision="fp32", batch=None,
                              resident=6400, streams=None, lanes=None, video_frames=0, host_frames=False,
                              round_robin=False, dump_outputs=None, check=False, check_all_ranks=False, cpu=False,
                              cpu_seconds=0.0, workload="detect")
    bench.resolve_shape(args)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        for run in range(1, a.runs + 1):
            for name, ctor in (("plain", plain), ("matched", matched)):
                runtime.Context = ctor  # run_stream imports the name when it is called
                try:
                    res = bench.run_stream(args, 1, 0, 0)
                finally:
                    runtime.Context = plain
                line = json.dumps({"contexts": name, "run": run, "result": res})
                fh.write(line + "\n")
                fh.flush()
                print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=["spans", "rate"], required=True)
    ap.add_argument("--steps", type=int, default=None, help="timed batches (spans: 10) or bench steps (rate: 40)")
    ap.add_argument("--warmup", type=int, default=None, help="spans: 3, rate: 5")
    ap.add_argument("--runs", type=int, default=3, help="rate: runs of each kind, alternating")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    spans = a.what == "spans"
    a.steps = a.steps if a.steps is not None else (10 if spans else 40)
    a.warmup = a.warmup if a.warmup is not None else (3 if spans else 5)
    a.out = a.out or os.path.join(ROOT, "profiles", "match", "kernel_spans.json" if spans else "bench_matched.jsonl")
    (run_spans if spans else run_rate)(a)


if __name__ == "__main__":
    main()
