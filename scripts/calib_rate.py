#!/usr/bin/env python3
"""Rate of the calibration pass (lm_calib_push_device) next to the background
pass (lm_bkg_push_device) on one GPU, in the same run: synthetic frames
(lm_synth_frames_device) resident in HBM at 1024x256, pushes of 256 frames,
timed with HIP events on each context's stream after a warm-up, the two passes
alternating over --rounds rounds.  The program runs both passes back to back,
so the expectation is that the calibration pass, which does less work per
byte, is not the slower one.  Also the wall split of LocoMouseCalibrate
(LM_TIMING) on a marker video of --video-frames frames (0: skip).  Writes
profiles/calib/rate.json (or --out) and prints the same JSON line."""
import argparse
import json
import os
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12  # bytes/s: the float4 copy and the data sheet (MI355X)


def timed_pushes(ctx, stream, d_ptr, pitch, B, nbuf, steps):
    import torch
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record(stream)
    for i in range(steps):
        ctx.push_device(d_ptr + (i % nbuf) * B * pitch, pitch, B)
    ev[1].record(stream)
    stream.synchronize()
    return ev[0].elapsed_time(ev[1])


def measure(args):
    import numpy as np
    import torch

    import calib_harness as CH
    from locomouse_cpp_amd import runtime
    from locomouse_cpp_amd import synthetic as S
    rows, cols, split, B, nbuf = args.rows, args.cols, args.split, args.batch, 4
    pitch = rows * cols
    d = torch.empty(nbuf * B * pitch, dtype=torch.uint8, device="cuda:0")
    runtime.synth_frames_device(d.data_ptr(), rows, cols, 0, nbuf * B, pitch)
    torch.cuda.synchronize()
    bkg_image = S.synth_background(rows, cols)
    cal = runtime.Calibrator(rows, cols, split, max_batch=B)
    cal.set_background(bkg_image)
    est = runtime.BackgroundEstimator(rows, cols, max_batch=B)
    s_cal, s_est = torch.cuda.ExternalStream(cal.stream()), torch.cuda.ExternalStream(est.stream())
    # warm-up: every shape of the timed window, and the record buffer at its final size
    timed_pushes(cal, s_cal, d.data_ptr(), pitch, B, nbuf, args.calib_steps)
    timed_pushes(est, s_est, d.data_ptr(), pitch, B, nbuf, args.warmup)
    # the check the timing rests on: the records of some pushed frames against the restatement
    host = d.view(nbuf * B, rows, cols)[:3].cpu().numpy()
    got = cal.records(0, 3)
    want = CH.ref_records(host, bkg_image, split, CH.DEFAULTS)
    ok = all(np.array_equal(got[n], want[n]) for n in CH.RECORD_DTYPE.names)
    cal_ms, est_ms = [], []
    for _ in range(args.rounds):
        cal.reset()
        est.reset()
        cal_ms.append(timed_pushes(cal, s_cal, d.data_ptr(), pitch, B, nbuf, args.calib_steps))
        est_ms.append(timed_pushes(est, s_est, d.data_ptr(), pitch, B, nbuf, args.bkg_steps))
    cal.close()
    est.close()
    cal_fps = [args.calib_steps * B / (ms * 1e-3) for ms in cal_ms]
    est_fps = [args.bkg_steps * B / (ms * 1e-3) for ms in est_ms]
    best = max(cal_fps)
    return {
        "metric": "calibration pass frames/s (lm_calib_push_device) next to the background pass (lm_bkg_push_device)",
        "value": sorted(cal_fps)[len(cal_fps) // 2], "unit": "frames/s", "higher_is_better": True,
        "rows": rows, "cols": cols, "split_row": split, "batch_frames": B, "rounds": args.rounds,
        "calibration": {"steps": args.calib_steps, "window_ms": cal_ms, "frames_per_s": cal_fps},
        "background": {"steps": args.bkg_steps, "warmup": args.warmup, "window_ms": est_ms, "frames_per_s": est_fps},
        "calibration_over_background": sorted(cal_fps)[len(cal_fps) // 2] / sorted(est_fps)[len(est_fps) // 2],
        "calibration_bytes_per_s": {
            "note": "frame bytes only, rows * cols per frame, over the window's time (the background image is read as "
                    "often but stays in cache; the window's second read of the frame is not counted); median round",
            "value": sorted(cal_fps)[len(cal_fps) // 2] * pitch,
            "share_of_measured_hbm_6.29e12": sorted(cal_fps)[len(cal_fps) // 2] * pitch / HBM_MEASURED,
            "share_of_spec_hbm_8.0e12": sorted(cal_fps)[len(cal_fps) // 2] * pitch / HBM_SPEC,
            "best_round_share_of_measured_hbm": best * pitch / HBM_MEASURED},
        "records_match_the_restatement": bool(ok),
        "data": "synthetic (lm_synth.h scene, resident in HBM)",
    }


def write_long_marker_avi(path, n_frames):
    """The 200-frame marker video of the tests (8-bit AVI) repeated to n_frames: the one written by
    media_writers.write_avi with its frame chunks repeated and the counts and sizes in its headers patched."""
    import calib_harness as CH
    import media_writers as MW
    video = CH.marker_video()
    reps = -(-n_frames // len(video))
    with tempfile.TemporaryDirectory() as tmp:
        short = os.path.join(tmp, "short.avi")
        MW.write_avi(short, video, bits=8)
        data = open(short, "rb").read()
    at = data.index(b"movi") - 8                      # "LIST" size "movi"
    chunks = data[at + 12:]
    head = bytearray(data[:at + 12])
    total = reps * len(video)
    a = head.index(b"avih") + 8
    head[a + 16:a + 20] = struct.pack("<I", total)     # dwTotalFrames
    s = head.index(b"strh") + 8
    head[s + 32:s + 36] = struct.pack("<I", total)     # dwLength
    head[at + 4:at + 8] = struct.pack("<I", 4 + reps * len(chunks))
    head[4:8] = struct.pack("<I", len(head) - 8 + reps * len(chunks))
    with open(path, "wb") as fh:
        fh.write(head)
        for _ in range(reps):
            fh.write(chunks)
    return total


def program_wall_split(n_frames):
    from locomouse_cpp_amd import runtime
    import calib_harness as CH
    with tempfile.TemporaryDirectory() as tmp:
        video, out = os.path.join(tmp, "marker.avi"), os.path.join(tmp, "calibration.yml")
        total = write_long_marker_avi(video, n_frames)
        runs = []
        for _ in range(2):  # the second run reads the file from the page cache
            p = subprocess.run([runtime.CALIB_CLI_PATH, video, out, str(CH.SPLIT)], env=dict(os.environ, LM_TIMING="1"),
                               capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                return {"frames": total, "error": p.stdout[-400:]}
            t = [ln for ln in p.stdout.splitlines() if ln.startswith("LM_TIMING ")][0].split()[1:]
            runs.append({t[i]: float(t[i + 1]) for i in range(0, len(t), 2)})
            runs[-1]["summary"] = p.stdout.splitlines()[0].split(", written to ")[0]
        return {"frames": total, "video_bytes": os.path.getsize(video), "runs": runs,
                "note": "LocoMouseCalibrate's LM_TIMING, milliseconds of wall time: background_ms is estimate_background "
                        "(read, decode, push, median), detect_ms the second read with lm_calib_push and the records' "
                        "read-back, fit_ms the fp64 fit and the map, write_ms the yml"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--cols", type=int, default=1024)
    ap.add_argument("--split", type=int, default=96)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--calib-steps", type=int, default=400)
    ap.add_argument("--bkg-steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--video-frames", type=int, default=10000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "calib", "rate.json"))
    args = ap.parse_args()
    line = measure(args)
    if not line["records_match_the_restatement"]:
        raise SystemExit("the pushed frames' records differ from the restatement: " + json.dumps(line))
    if args.video_frames > 0:
        try:
            line["program_wall_split"] = program_wall_split(args.video_frames)
        except (OSError, subprocess.SubprocessError, MemoryError) as e:
            line["program_wall_split"] = {"error": f"not measured: {e!r}"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(line, fh, indent=1)
        fh.write("\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
