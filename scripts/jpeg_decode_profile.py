"""The workload behind profiles/r07/jpeg/kernel_stats_*.csv: four
lm_jpeg_decode_device calls on one 256-frame batch of camera-sized frames
(256 x 1024, synthetic scene, quality 92), grey or 4:2:0 colour, for a kernel
trace.  Each CSV is rocprofv3's <name>_kernel_stats.csv of

    rocprofv3 --kernel-trace --stats -d OUT -o grey --output-format csv -- python scripts/jpeg_decode_profile.py grey
    rocprofv3 --kernel-trace --stats -d OUT -o c420 --output-format csv -- python scripts/jpeg_decode_profile.py c420

(4 calls per kernel: AverageNs is the time per 256-frame batch).
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import media_writers as MW  # noqa: E402
from locomouse_cpp_amd import runtime, synthetic as S  # noqa: E402

kind = sys.argv[1] if len(sys.argv) > 1 else "grey"
cfg = S.SyntheticConfig()
base = cfg.frames(0, 32)
rows, cols = base.shape[1:]
kw = dict(mode="L", quality=92) if kind == "grey" else dict(mode="RGB", quality=92, subsampling=2)
js = MW.jpeg_frames(base, **kw) * 8
dec = runtime.JpegDecoder(rows, cols, max_batch=256)
d = torch.empty((256, rows, cols), dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()
for r in range(4):
    st = dec.decode_into(js, d.data_ptr())
assert (st == 0).all()
print(kind, dec.stats())
dec.close()
