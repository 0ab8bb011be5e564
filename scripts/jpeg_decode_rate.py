"""Device JPEG decode rate (lm_jpeg_decode_device) on camera-sized frames
(256 x 1024, synthetic scene, quality 92), 256-frame batches, grey and 4:2:0,
at the default subsequence size and at 64 / 128 bytes: median wall time of 5
calls and the last call's statistics, as JSON (profiles/r07/jpeg/decode_rate.json).

    python scripts/jpeg_decode_rate.py [out.json]
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import media_writers as MW
from locomouse_cpp_amd import runtime, synthetic as S

cfg = S.SyntheticConfig()
base = cfg.frames(0, 32)
rows, cols = base.shape[1:]
out = {}
for tag, kw in (("grey_q92", dict(mode="L", quality=92)), ("c420_q92", dict(mode="RGB", quality=92, subsampling=2))):
    js = MW.jpeg_frames(base, **kw) * 8
    for subseq in (0, 64, 128):
        dec = runtime.JpegDecoder(rows, cols, max_batch=256, subseq_bytes=subseq)
        d = torch.empty((256, rows, cols), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ts = []
        for r in range(6):
            t0 = time.perf_counter()
            st = dec.decode_into(js, d.data_ptr())
            ts.append(time.perf_counter() - t0)
        assert (st == 0).all()
        ms = sorted(ts[1:])[len(ts[1:]) // 2] * 1e3
        out[f"{tag}_s{subseq}"] = dict(ms_per_256=round(ms, 2), fps=round(256 / ms * 1e3), bytes=len(js[0]), **dec.stats())
        dec.close()
        print(tag, subseq, out[f"{tag}_s{subseq}"], flush=True)
dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "bench_out", "jpeg_decode_rate.json")
os.makedirs(os.path.dirname(os.path.abspath(dst)), exist_ok=True)
json.dump(out, open(dst, "w"), indent=1)
