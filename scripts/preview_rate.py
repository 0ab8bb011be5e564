#!/usr/bin/env python3
"""Rates of the preview's device stages (include/locomouse_encode.h) on one
GPU: synthetic 1024x256 frames (lm_synth_frames_device) resident in HBM,
256-frame calls, 10 timed calls after 3 warm-up.  Two figures in frames/s, from
the context's own HIP events (first kernel to last, lm_enc_last_stats):

  * grey encode (lm_enc_encode_device), and
  * render + 4:2:0 encode with 25 marks per frame (lm_enc_render_encode_device),

with the wall time of the same calls (which adds the copy of the files to the
host) beside them.  The baselines, in the same run on the same frames: the host
encoder (host/JpegEncode.cpp) on the host threads this process may use, and
Pillow (libjpeg-turbo) on one core.  One call's files are checked against the
host encoder's before anything is timed.  Writes profiles/r09/preview/rate.json
(or --out) and prints the same JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def host_threads():
    n = len(os.sched_getaffinity(0))
    omp = os.environ.get("OMP_NUM_THREADS")
    return max(1, min(n, int(omp))) if omp and omp.isdigit() else n


def marks_of(n, per_frame, rows, cols, radius):
    """per_frame marks on every frame, moving with the frame number, some cut by the borders."""
    return [[((37 * k + 5 * f) % cols, (53 * k + 3 * f) % rows, radius if k < 10 else 1, k % 8) for k in range(per_frame)]
            for f in range(n)]


def pillow_rate(EH, frames, quality, n=32):
    """Pillow on this thread, frames/s over n frames, after one untimed encode (the first loads Pillow's plugins)."""
    EH.pillow_encode(frames[0], quality)
    t0 = time.perf_counter()
    for i in range(n):
        EH.pillow_encode(frames[i], quality)
    return n / (time.perf_counter() - t0)


def timed_calls(call, enc, steps, warmup, batch):
    for _ in range(warmup):
        call()
    dev_ms, wall_ms, nbytes = [], [], 0
    for _ in range(steps):
        t0 = time.perf_counter()
        call()
        wall_ms.append(1e3 * (time.perf_counter() - t0))
        st = enc.stats()
        dev_ms.append(st["device_ms"])
        nbytes = st["bytes_out"]
    return {"frames_per_s": steps * batch / (sum(dev_ms) * 1e-3), "frames_per_s_wall": steps * batch / (sum(wall_ms) * 1e-3),
            "device_ms_per_call": {"mean": sum(dev_ms) / steps, "min": min(dev_ms), "max": max(dev_ms)},
            "wall_ms_per_call": {"mean": sum(wall_ms) / steps, "min": min(wall_ms), "max": max(wall_ms)},
            "bytes_per_frame": nbytes / batch}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--cols", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--marks", type=int, default=25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09", "preview", "rate.json"))
    a = ap.parse_args()
    import numpy as np
    import torch

    import enc_harness as EH
    from locomouse_cpp_amd import abi, runtime
    rows, cols, B = a.rows, a.cols, a.batch
    pitch = rows * cols
    d = torch.empty(B * pitch, dtype=torch.uint8, device="cuda:0")
    runtime.synth_frames_device(d.data_ptr(), rows, cols, 0, B, pitch)
    torch.cuda.synchronize()
    raw = d.view(B, rows, cols).cpu().numpy()
    threads = host_threads()
    out = {"what": "preview stages: device JPEG encode and render + encode, frames/s from HIP events",
           "rows": rows, "cols": cols, "batch_frames": B, "steps": a.steps, "warmup": a.warmup, "quality": a.quality,
           "marks_per_frame": a.marks, "host_threads": threads, "data": "synthetic (lm_synth.h scene, resident in HBM)"}

    # grey
    enc = runtime.JpegEncoder(rows, cols, abi.LM_ENC_GRAY8, quality=a.quality, max_batch=B)
    files = enc.encode_device(d.data_ptr(), B)
    ok = all(files[i] == EH.host_encode(raw[i], a.quality) for i in (0, 1, B // 2, B - 1))
    out["grey_encode"] = timed_calls(lambda: enc.encode_device(d.data_ptr(), B, files=False), enc, a.steps, a.warmup, B)
    enc.close()
    EH.host_encode_many(raw[:threads], a.quality, threads)  # untimed: the threads' first allocations
    t0 = time.perf_counter()
    EH.host_encode_many(raw, a.quality, threads)
    out["grey_encode"]["host_encoder_frames_per_s"] = B / (time.perf_counter() - t0)
    out["grey_encode"]["pillow_one_core_frames_per_s"] = pillow_rate(EH, raw, a.quality)

    # render + 4:2:0 encode
    enc = runtime.JpegEncoder(rows, cols, abi.LM_ENC_RGB24, quality=a.quality, max_batch=B)
    cal = np.arange(rows * cols, dtype=np.int32).reshape(rows, cols)
    enc.set_overlay(cal, rows, cols, 0)
    marks = marks_of(B, a.marks, rows, cols, 3)
    arr, off = enc._marks(marks)
    canvases = enc.render_device(d.data_ptr(), pitch, marks)
    files = enc.render_encode_device(d.data_ptr(), pitch, marks)
    ok = ok and all(files[i] == EH.host_encode(canvases[i], a.quality) for i in (0, 1, B // 2, B - 1))
    res = abi.lm_enc_result()

    def call():
        rc = runtime.lib().lm_enc_render_encode_device(enc._h, C.c_void_p(d.data_ptr()), pitch, B, arr, off.ctypes.data,
                                                      C.byref(res))
        assert rc == abi.LM_OK, runtime.lib().lm_last_error()

    out["render_encode_420"] = timed_calls(call, enc, a.steps, a.warmup, B)
    enc.close()
    t0 = time.perf_counter()
    EH.host_encode_many(canvases, a.quality, threads)
    out["render_encode_420"]["host_encoder_frames_per_s"] = B / (time.perf_counter() - t0)
    out["render_encode_420"]["host_encoder_note"] = "the host figure encodes canvases that are already rendered"
    out["render_encode_420"]["pillow_one_core_frames_per_s"] = pillow_rate(EH, canvases, a.quality)
    out["matches_host_encoder"] = bool(ok)
    if not ok:
        raise SystemExit("the device's files differ from the host encoder's: " + json.dumps(out))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
