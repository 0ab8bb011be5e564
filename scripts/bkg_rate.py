#!/usr/bin/env python3
"""Rate of the background pass (lm_bkg_push_device) on one GPU: synthetic
frames (lm_synth_frames_device) resident in HBM at 1024x256, pushes of 256
frames, 20 timed steps after 5 warm-up, timed with HIP events on the context's
stream.  Writes frames/s, the per-kernel times and the HBM bytes a batch needs
to profiles/r08/bkg/rate.json (or --out) and prints the same JSON line.

The yardstick is the bounding-box pass, the other whole-video pre-pass:
`python bench.py --workload bb --batch 256 --steps 20 --warmup 5` in the same
GPU visit.  --px 1|2|4 (one process each) compares k_bkg_accum's pixels per
thread through the LM_BKG_PX diagnostics switch."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(args):
    import numpy as np
    import torch

    from locomouse_cpp_amd import runtime
    rows, cols, B, nbuf = args.rows, args.cols, args.batch, 4
    pitch = rows * cols
    d = torch.empty(nbuf * B * pitch, dtype=torch.uint8, device="cuda:0")
    runtime.synth_frames_device(d.data_ptr(), rows, cols, 0, nbuf * B, pitch)
    torch.cuda.synchronize()
    est = runtime.BackgroundEstimator(rows, cols, max_batch=B)
    stream = torch.cuda.ExternalStream(est.stream())
    for i in range(args.warmup):
        est.push_device(d.data_ptr() + (i % nbuf) * B * pitch, pitch, B)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    ev[0].record(stream)
    for i in range(args.steps):
        est.push_device(d.data_ptr() + (i % nbuf) * B * pitch, pitch, B)
        ev[i + 1].record(stream)
    stream.synchronize()
    push_ms = [ev[i].elapsed_time(ev[i + 1]) for i in range(args.steps)]
    total_ms = ev[0].elapsed_time(ev[-1])
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    img = est.finish(500)  # k_bkg_select + the D2H copy of the image
    e1.record(stream)
    stream.synchronize()
    samples = est.samples
    # the check the timing rests on: the median of the frames that were pushed
    host = d.view(nbuf * B, rows, cols)[:, :8, :64].cpu().numpy()
    order = [(i % nbuf) * B + k for i in range(args.warmup + args.steps) for k in range(B)]
    want = np.sort(host[order], axis=0)[(500 * (len(order) - 1)) // 1000]
    ok = bool(np.array_equal(img[:8, :64], want))
    est.close()
    npix = rows * cols
    # 64-byte lines of the table one batch's updates fall in: a line holds 32 counters, bins 32 l .. 32 l + 31
    first = d[:B * pitch].view(B, npix) >> 5
    lines = sum(int((first == ln).any(dim=0).sum()) for ln in range(8))
    return {
        "metric": "background pass frames/s (lm_bkg_push_device, per-pixel histograms)",
        "value": args.steps * B / (total_ms * 1e-3), "unit": "frames/s", "higher_is_better": True,
        "rows": rows, "cols": cols, "batch_frames": B, "steps": args.steps, "warmup": args.warmup,
        "pixels_per_thread": int(os.environ.get("LM_BKG_PX", "4")),
        "kernel_ms": {"k_bkg_accum": {"mean": sum(push_ms) / len(push_ms), "min": min(push_ms), "max": max(push_ms)},
                      "k_bkg_select_and_copy": e0.elapsed_time(e1)},
        "hbm_bytes_per_batch": {
            "frames_read": B * npix,
            "histogram_table": 2 * 256 * npix,
            "histogram_lines_per_pixel": lines / npix,
            "histogram_read_and_written": 2 * 64 * lines,
            "total": B * npix + 2 * 64 * lines,
            "note": "from the first batch's values, not from counters: the frames are read once, and a pixel's "
                    "updates read and write back the 64-byte lines (32 counters each) its values fall in, "
                    "once each if they stay in L2 for the launch"},
        "samples": samples, "matches_numpy_on_a_corner": ok,
        "data": "synthetic (lm_synth.h scene, resident in HBM)",
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--cols", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--px", type=int, nargs="*", default=None, help="also measure these pixels-per-thread variants")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08", "bkg", "rate.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(measure(args)))
        return
    line = measure(args)
    if not line["matches_numpy_on_a_corner"]:
        raise SystemExit("the pushed frames' median differs from numpy: " + json.dumps(line))
    if args.px:  # each variant in a fresh process (the switch is read when the context is made)
        line["variants"] = []
        for px in args.px:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--rows", str(args.rows), "--cols", str(args.cols),
                   "--batch", str(args.batch), "--steps", str(args.steps), "--warmup", str(args.warmup)]
            out = subprocess.run(cmd, env=dict(os.environ, LM_BKG_PX=str(px)), capture_output=True, text=True,
                                 timeout=300, check=True).stdout
            v = json.loads(out.strip().splitlines()[-1])
            line["variants"].append({k: v[k] for k in ("pixels_per_thread", "value", "kernel_ms",
                                                       "matches_numpy_on_a_corner")})
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(line, fh, indent=1)
        fh.write("\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
