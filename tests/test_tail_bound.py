"""The tail detectors' tile bound (locomouse_cpp_amd/csrc/lm_tail_bound.h) on
the host, without a GPU: a stand-alone program (tests/cpp/tail_bound_check.cpp)
checks that a tile the bound marks "skip" never holds a positive score in the
fused or the unfused fp32 chain, on synthetic detectors and images and on the
oracle's own windows of synthetic C3 frames (where the bound must also prove
most tiles: non-vacuity); once more under the sanitizers."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from locomouse_cpp_amd import synthetic as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "tail_bound_check.cpp")
INC = "-I" + os.path.join(ROOT, "locomouse_cpp_amd", "csrc")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tail_bound") / "tail_bound_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", INC, SRC, "-o", exe])
    return exe


def _synth(exe):
    r = subprocess.run([exe, "synth"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    m = re.search(r"(\d+) cases, 0 failures, (\d+) tiles, (\d+) skipped, (\d+) non-positive", r.stdout)
    assert m, r.stdout[-2000:]
    cases, tiles, skipped, nonpos = map(int, m.groups())
    assert cases >= 300
    assert 0 < skipped <= nonpos < tiles  # some tiles proven, some positive: neither side is vacuous


def test_skipped_tiles_hold_no_positive_score(checker):
    _synth(checker)


def _normalised(cfg, frame):
    """readFrame's subtract + NORM_MINMAX (LocoMouse_class.cpp:1304-1310) of
    one frame, identity calibration."""
    d = np.clip(frame.astype(np.int32) - cfg.background.astype(np.int32), 0, 255)
    mn, mx = int(d.min()), int(d.max())
    scale = 255.0 / (mx - mn) if mx - mn > 2.220446049250313e-16 else 0.0
    t = d.astype(np.float32) * np.float32(scale) + np.float32(-mn * scale)
    return np.clip(np.rint(t), 0, 255).astype(np.uint8)


def test_bound_proves_most_tiles_of_the_synthetic_frames(checker, tmp_path):
    """The oracle's windows of synthetic C3 frames 0-8: the checker's fused
    chain reproduces the oracle's tail scores bit for bit (so the windows are
    the reference's), no skipped tile holds a positive score, and at least
    60 % of the 40 x 4 tiles of each tail detector are skipped."""
    from oracle import oracle as O
    cfg = S.SyntheticConfig()
    frames = cfg.frames(0, 9)
    ref = O.OracleRun(cfg, frames, flags=O.KEEP_DEBUG)
    g = O.geometry(cfg)
    p = cfg.params
    pad = 64
    blob = [struct.pack("<i", 2)]
    for det, name, box in ((2, "tail_bottom", p.bounding_box_bottom), (5, "tail_side", p.bounding_box_side)):
        w = cfg.weights[name].astype(np.float32)
        kh, kw = w.shape
        oh, ow = box.height, g.tail_box_width
        blob.append(struct.pack("<5if", kh, kw, oh, ow, len(frames), np.float32(-cfg.biases[name])))
        blob.append(w.tobytes())
        for f, fr in enumerate(frames):
            n = np.pad(_normalised(cfg, fr), pad)
            # the mouse crop starts one pixel right of and below the box corner (getBoundingBox :547-557);
            # output (y, x) has its anchor tap (kh / 2, kw / 2) on crop pixel (y, x)
            y0, x0 = pad + box.y + 1 - kh // 2, pad + box.x + 1 - kw // 2
            win = np.ascontiguousarray(n[y0:y0 + oh + kh - 1, x0:x0 + ow + kw - 1])
            assert win.shape == (oh + kh - 1, ow + kw - 1)
            blob.append(win.tobytes())
            blob.append(ref.scores(f, det, (oh, ow)).tobytes())
    path = tmp_path / "crops.bin"
    path.write_bytes(b"".join(blob))
    r = subprocess.run([checker, "crops", str(path)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rows = re.findall(r"det (\d): tiles (\d+) skipped (\d+) nonpositive (\d+) mismatch 0 failures 0", r.stdout)
    assert len(rows) == 2, r.stdout
    for _, tiles, skipped, nonpos in rows:
        assert int(skipped) >= 0.60 * int(tiles), r.stdout
        assert int(skipped) <= int(nonpos)


def test_bound_is_clean_under_the_sanitizers(tmp_path):
    """The same program built with -fsanitize=address,undefined; nothing is
    loaded into Python."""
    exe = str(tmp_path / "tail_bound_check_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", INC, SRC, "-o", exe])
    _synth(exe)
