"""Restart-interval MJPEG: the device decoder's interval path against its
subsequence path and the host decoder, and the device encoder with and without
restart markers (profiles/rst/rate.json).

The protocol is DESIGN.md §13's: 256-frame batches of camera-sized frames
(256 x 1024, synthetic scene, quality 92), median wall time of 5
lm_jpeg_decode_device calls.  Streams: grey (written by the device encoder) and
4:2:0 (written by Pillow), at restart intervals of none, one MCU row, 32, 16, 8
and 4 MCUs.  For each: the decode with the interval path on and off in one
process (lm_jpeg_set_interval_path), the host decoder on 16 threads on the
same files, the files' growth against no restarts, and for grey the encode rate
from HIP events.

    python scripts/jpeg_rst_rate.py [out.json]
    python scripts/jpeg_rst_rate.py --only grey:8 [--path off]   # decode calls alone, for a profiler run of its own
    python scripts/jpeg_rst_rate.py --merge-stats grey:8 kernel_stats.csv out.json   # that run's kernel split
"""
import csv
import json
import os
import re
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

N, HOST_THREADS = 256, 16
INTERVALS = (("none", 0), ("row", None), ("32", 32), ("16", 16), ("8", 8), ("4", 4))


def streams(tag, ri):
    """The 256 files of one stream at a restart interval of ri MCUs (0: none), and for grey the encode's HIP time."""
    import media_writers as MW
    from locomouse_cpp_amd import runtime, synthetic as S
    base = S.SyntheticConfig().frames(0, 32)
    rows, cols = base.shape[1:]
    if tag == "grey":
        import torch
        frames = np.ascontiguousarray(np.tile(base, (8, 1, 1)))
        d = torch.from_numpy(frames).cuda()
        torch.cuda.synchronize()
        enc = runtime.JpegEncoder(rows, cols, runtime.JpegEncoder.GRAY8, quality=92, max_batch=N, restart_interval=ri)
        ms = []
        for _ in range(6):
            files = enc.encode_device(d.data_ptr(), N)
            ms.append(enc.stats()["device_ms"])
        enc.close()
        return files, rows, cols, sorted(ms[1:])[2]
    kw = dict(restart_marker_blocks=ri) if ri else {}
    return MW.jpeg_frames(base, mode="RGB", quality=92, subsampling=2, **kw) * 8, rows, cols, None


def decode_calls(dec, js, d, calls=6):
    ts, dev = [], []
    for _ in range(calls):
        t0 = time.perf_counter()
        st = dec.decode_into(js, d.data_ptr())
        ts.append(time.perf_counter() - t0)
        dev.append(dec.stats()["device_ms"])
    assert (st == 0).all()
    return sorted(ts[1:])[len(ts[1:]) // 2] * 1e3, sorted(dev[1:])[len(dev[1:]) // 2]


def interval_of(tag, name, ri, cols):
    return (cols + (7 if tag == "grey" else 15)) // (8 if tag == "grey" else 16) if name == "row" else ri


def measure(only=None, path=None):
    import torch
    import jpeg_harness as JH
    from locomouse_cpp_amd import runtime
    out = {}
    for tag in ("grey", "c420"):
        plain_bytes = None
        for name, ri in INTERVALS:
            if only and only != f"{tag}:{name}":
                continue
            js, rows, cols, enc_ms = streams(tag, interval_of(tag, name, ri, 1024))
            total = sum(map(len, js))
            if name == "none":
                plain_bytes = total
            dec = runtime.JpegDecoder(rows, cols, max_batch=N)
            d = torch.empty((N, rows, cols), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            if only:  # the profiler's run: the decode calls alone
                dec.set_interval_path(path != "off")
                decode_calls(dec, js, d, calls=4)
                dec.close()
                continue
            rec = dict(restart_mcus=interval_of(tag, name, ri, cols), bytes_per_frame=round(total / N))
            if plain_bytes:
                rec["growth_percent"] = round(100.0 * (total - plain_bytes) / plain_bytes, 3)
            for mode in ("on", "off", "on", "off"):  # alternating, the later pair kept
                dec.set_interval_path(mode == "on")
                ms, dev_ms = decode_calls(dec, js, d)
                ist = dec.interval_stats()
                rec[mode] = dict(ms_per_256=round(ms, 3), fps=round(N / ms * 1e3), device_ms=round(dev_ms, 3),
                                 parse_ms=round(ist["parse_ms"], 3), frames_interval=ist["frames_interval"],
                                 intervals=ist["intervals"], longest_interval_bytes=ist["longest_interval_bytes"],
                                 sync_rounds=dec.stats()["sync_rounds"])
            # the marker index's share of the host parse: the same call with the path off builds none
            rec["index_ms_per_256"] = round(rec["on"]["parse_ms"] - rec["off"]["parse_ms"], 3)
            got = d.cpu().numpy()
            with ThreadPoolExecutor(HOST_THREADS) as pool:
                ts = []
                for _ in range(4):
                    t0 = time.perf_counter()
                    host = list(pool.map(lambda j: JH.host_decode(j, rows, cols), js))
                    ts.append(time.perf_counter() - t0)
            assert all(np.array_equal(got[i], host[i]) for i in range(0, N, 17))
            hms = sorted(ts[1:])[1] * 1e3
            rec["host_16_threads"] = dict(ms_per_256=round(hms, 3), fps=round(N / hms * 1e3))
            if enc_ms is not None:
                rec["encode"] = dict(device_ms_per_256=round(enc_ms, 4), fps=round(N / enc_ms * 1e3))
            dec.close()
            out[f"{tag}_{name}"] = rec
            print(tag, name, json.dumps(rec), flush=True)
    return out


def merge_stats(key, stats_csv, dst):
    """The kernels' share of a profiler run (rocprofv3 --kernel-trace --stats: *_kernel_stats.csv) into dst[key]."""
    out = json.load(open(dst)) if os.path.exists(dst) else {}
    rows = list(csv.DictReader(open(stats_csv)))
    split = {re.search(r"k_jpeg_\w+", r["Name"]).group(0): dict(calls=int(r["Calls"]), percent=float(r["Percentage"]),
                                                                avg_us=round(float(r["AverageNs"]) / 1e3, 2))
             for r in rows if "k_jpeg" in r["Name"]}
    out.setdefault("kernel_split", {})[key] = split
    json.dump(out, open(dst, "w"), indent=1)
    print(key, json.dumps(split))


if __name__ == "__main__":
    a = sys.argv[1:]
    if a and a[0] == "--merge-stats":
        merge_stats(a[1], a[2], a[3])
    elif a and a[0] == "--only":
        measure(only=a[1], path=a[3] if len(a) > 3 and a[2] == "--path" else "on")
    else:
        dst = a[0] if a else os.path.join(ROOT, "bench_out", "jpeg_rst_rate.json")
        res = measure()
        res["protocol"] = "256 frames of 256 x 1024 at quality 92 per call; median of 5 calls after one warm-up"
        res["parent_encode_fps"] = 404600
        os.makedirs(os.path.dirname(os.path.abspath(dst)), exist_ok=True)
        json.dump(res, open(dst, "w"), indent=1)
