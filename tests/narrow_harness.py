"""The host statement of k_tile_bound's narrow and wide lists for a batch of
frames: the six detectors' views written as tests/test_tile_refine.py's crops
fixture writes them (the detector's window as the runtime's ext crop holds it,
from the normalised frames), classified by tests/cpp/narrow_class_check.cpp in
its `entries` mode."""
import os
import struct
import subprocess

import numpy as np

from test_tail_bound import _normalised
from test_tile_refine import DETS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "narrow_class_check.cpp")
CSRC = os.path.join(ROOT, "locomouse_cpp_amd", "csrc")


def build(exe):
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + CSRC, SRC, "-o", exe])
    return exe


def write_views(cfg, frames, path):
    """The views of every detector for `frames` (identity calibration, fixed
    boxes); the reference scores of the file format are left zero: the narrow
    checker does not read them."""
    from oracle import oracle as O
    g = O.geometry(cfg)
    p = cfg.params
    pad = 96
    norm = [np.pad(_normalised(cfg, fr), pad) for fr in frames]
    blob = [struct.pack("<i", len(DETS))]
    for det, name, view, kind in DETS:
        box = p.bounding_box_side if view else p.bounding_box_bottom
        shapes = [cfg.weights[n].shape for _, n, v, _ in DETS if v == view]
        w = cfg.weights[name].astype(np.float32)
        kh, kw = w.shape
        in_y = max(s[0] // 2 for s in shapes) - kh // 2
        in_x = max(s[1] // 2 for s in shapes) - kw // 2
        oh, ow = box.height, (g.tail_box_width if kind else box.width)
        eh, ew = in_y + oh + kh - 1, -(-(in_x + ow + kw - 1) // 16) * 16
        blob.append(struct.pack("<10if", kh, kw, oh, ow, len(frames), eh, ew, in_y, in_x, kind, np.float32(-cfg.biases[name])))
        blob.append(w.tobytes())
        zero = np.zeros((oh, ow), np.float32).tobytes()
        for f in range(len(frames)):
            y0, x0 = pad + box.y + 1 - kh // 2 - in_y, pad + box.x + 1 - kw // 2 - in_x
            ext = np.ascontiguousarray(norm[f][y0:y0 + eh, x0:x0 + ew])
            assert ext.shape == (eh, ew)
            blob.append(ext.tobytes())
            blob.append(zero)
    with open(path, "wb") as fh:
        fh.write(b"".join(blob))
    return path


def host_entries(exe, cfg, frames, path):
    """{detector id: {(frame, tile): (narrow, first, count)}} of every tile the correlation keeps."""
    write_views(cfg, frames, path)
    r = subprocess.run([exe, "entries", str(path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = {d: {} for d in range(len(DETS))}
    for line in r.stdout.splitlines():
        if line.startswith("e "):
            d, f, t, n, a, c = map(int, line.split()[1:])
            out[d][(f, t)] = (n, a, c)
    return out


def counts(ent):
    return {d: (sum(v[0] for v in e.values()), sum(1 - v[0] for v in e.values())) for d, e in ent.items()}
