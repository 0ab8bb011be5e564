"""The tile bound (locomouse_cpp_amd/csrc/lm_tail_bound.h) applied to the
point detectors, on the host without a GPU: a stand-alone program
(tests/cpp/point_bound_check.cpp) checks on the oracle's own windows of
synthetic C3 frames that no bright 40 x 4 tile the bound marks "skip" holds a
positive score in the fused or the unfused fp32 chain, and that the bound
proves a good share of the bright tiles (non-vacuity); once more under the
sanitizers."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from locomouse_cpp_amd import synthetic as S
from test_tail_bound import _normalised

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "point_bound_check.cpp")
INC = "-I" + os.path.join(ROOT, "locomouse_cpp_amd", "csrc")
# (debug id, name, view) of the four point detectors
DETS = ((0, "paw_bottom", 0), (1, "snout_bottom", 0), (3, "paw_side", 1), (4, "snout_side", 1))
ROW = re.compile(r"det (\d): tiles (\d+) bright (\d+) nokept (\d+) proven (\d+) mismatch (\d+) failures (\d+)")


@pytest.fixture(scope="module")
def crops(tmp_path_factory):
    """Files of the oracle's windows and raw scores of the point detectors:
    synthetic C3 frames 0-8, and frames 0-1 alone (for the sanitizer run)."""
    from oracle import oracle as O
    cfg = S.SyntheticConfig()
    frames = cfg.frames(0, 9)
    ref = O.OracleRun(cfg, frames, flags=O.KEEP_DEBUG)
    p = cfg.params
    pad = 64
    norm = [np.pad(_normalised(cfg, fr), pad) for fr in frames]
    paths = {}
    for nf in (9, 2):
        blob = [struct.pack("<i", len(DETS))]
        for det, name, view in DETS:
            box = p.bounding_box_side if view else p.bounding_box_bottom
            w = cfg.weights[name].astype(np.float32)
            kh, kw = w.shape
            oh, ow = box.height, box.width
            blob.append(struct.pack("<5if", kh, kw, oh, ow, nf, np.float32(-cfg.biases[name])))
            blob.append(w.tobytes())
            for f in range(nf):
                # the mouse crop starts one pixel right of and below the box corner (getBoundingBox :547-557);
                # output (y, x) has its anchor tap (kh / 2, kw / 2) on crop pixel (y, x)
                y0, x0 = pad + box.y + 1 - kh // 2, pad + box.x + 1 - kw // 2
                win = np.ascontiguousarray(norm[f][y0:y0 + oh + kh - 1, x0:x0 + ow + kw - 1])
                assert win.shape == (oh + kh - 1, ow + kw - 1)
                blob.append(win.tobytes())
                blob.append(ref.scores(f, det, (oh, ow)).tobytes())
        paths[nf] = tmp_path_factory.mktemp("point_bound") / f"crops{nf}.bin"
        paths[nf].write_bytes(b"".join(blob))
    return paths


def _run(exe, path):
    r = subprocess.run([exe, "crops", str(path)], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rows = [tuple(map(int, m)) for m in ROW.findall(r.stdout)]
    assert len(rows) == len(DETS), r.stdout
    for _, tiles, bright, nokept, proven, mismatch, failures in rows:
        assert mismatch == 0 and failures == 0, r.stdout
        assert 0 < proven <= nokept <= bright < tiles, r.stdout
    return rows


def test_bound_proves_bright_tiles_of_the_synthetic_frames(crops, tmp_path):
    """Frames 0-8: the checker's fused chain reproduces the oracle's raw point
    scores bit for bit on every bright tile (so the windows are the
    reference's), no proven tile holds a positive score in either chain, and
    at least 40 % of the bright tiles of each point detector are proven (a
    numpy estimate without the rounding term gave 49.7 - 58.0 %)."""
    exe = str(tmp_path / "point_bound_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", INC, SRC, "-o", exe])
    for _, tiles, bright, nokept, proven, _, _ in _run(exe, crops[9]):
        assert proven >= 0.40 * bright, (tiles, bright, nokept, proven)


def test_bound_is_clean_under_the_sanitizers(crops, tmp_path):
    """The same program built with -fsanitize=address,undefined on frames 0-1;
    nothing is loaded into Python."""
    exe = str(tmp_path / "point_bound_check_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", INC, SRC, "-o", exe])
    _run(exe, crops[2])
