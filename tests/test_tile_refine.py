"""The refinement of the tile bound (locomouse_cpp_amd/csrc/lm_tail_bound.h:
the bound per 8-column output block and group of 8 taps, for the tiles the
tile bound fails) on the host, without a GPU: a stand-alone program
(tests/cpp/tile_refine_check.cpp) checks on synthetic detectors and images and
on the oracle's own windows of synthetic C3 frames that no tile the rule skips
holds a positive score in the fused or the unfused fp32 chain, that the
four-row shortcut never changes a flag, and that every detector proves more
tiles than the tile bound alone, at least the floors of the shipped block
height; once more under the sanitizers."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from locomouse_cpp_amd import synthetic as S
from test_tail_bound import _normalised

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "tile_refine_check.cpp")
INC = "-I" + os.path.join(ROOT, "locomouse_cpp_amd", "csrc")
# (debug id, name, view, kind: 0 point / 1 tail) of the six detectors
DETS = ((0, "paw_bottom", 0, 0), (1, "snout_bottom", 0, 0), (2, "tail_bottom", 0, 1),
        (3, "paw_side", 1, 0), (4, "snout_side", 1, 0), (5, "tail_side", 1, 1))
# floors on the proven share of the bright (point) / all (tail) tiles per
# shipped block height: five points under a numpy estimate with the blocks
# aligned to the window (1 row: 70.6, 70.8, 94.0, 77.1, 76.7, 92.5 %; 4 rows:
# 60.5, 63.1, 92.8, 72.2, 71.9, 91.8 %)
FLOORS = {1: {"bottom": 0.65, "side": 0.70, "tail": 0.87}, 4: {"bottom": 0.55, "side": 0.66, "tail": 0.86}}
ROW = re.compile(r"det (\d): tiles (\d+) bright (\d+) nokept (\d+) base (\d+) rh4 (\d+) rh1 (\d+) shipped (\d+) "
                 r"mismatch (\d+) shortcut (\d+) failures (\d+)")
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


def _build(exe, flags):
    subprocess.check_call(["g++", *flags, "-std=c++17", "-ffp-contract=off", INC, SRC, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("tile_refine") / "tile_refine_check"), ["-O2"])


@pytest.fixture(scope="module")
def checker_san(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("tile_refine_san") / "tile_refine_check_san"), SAN)


@pytest.fixture(scope="module")
def crops(tmp_path_factory):
    """Files of the six detectors' views and the oracle's raw scores: synthetic
    C3 frames 0-8, and frame 0 alone (for the sanitizer run).  A view is the
    detector's window as the runtime's ext crop holds it: the three windows of
    a camera view share the box's corner, the crop starts at the leftmost and
    topmost of them, so the window of a kh x kw detector starts at
    (max kh' / 2 - kh / 2, max kw' / 2 - kw / 2) of it, and a row is a multiple
    of 16 bytes."""
    from oracle import oracle as O
    cfg = S.SyntheticConfig()
    frames = cfg.frames(0, 9)
    ref = O.OracleRun(cfg, frames, flags=O.KEEP_DEBUG)
    g = O.geometry(cfg)
    p = cfg.params
    pad = 96
    norm = [np.pad(_normalised(cfg, fr), pad) for fr in frames]
    paths = {}
    for nf in (9, 1):
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
            blob.append(struct.pack("<10if", kh, kw, oh, ow, nf, eh, ew, in_y, in_x, kind, np.float32(-cfg.biases[name])))
            blob.append(w.tobytes())
            for f in range(nf):
                # the mouse crop starts one pixel right of and below the box corner (getBoundingBox :547-557);
                # output (y, x) has its anchor tap (kh / 2, kw / 2) on crop pixel (y, x)
                y0, x0 = pad + box.y + 1 - kh // 2 - in_y, pad + box.x + 1 - kw // 2 - in_x
                ext = np.ascontiguousarray(norm[f][y0:y0 + eh, x0:x0 + ew])
                assert ext.shape == (eh, ew)
                blob.append(ext.tobytes())
                blob.append(ref.scores(f, det, (oh, ow)).tobytes())
        paths[nf] = tmp_path_factory.mktemp("tile_refine_crops") / f"crops{nf}.bin"
        paths[nf].write_bytes(b"".join(blob))
    return paths


def _synth(exe):
    r = subprocess.run([exe, "synth"], capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    m = re.search(r"(\d+) cases, 0 failures, (\d+) tiles, (\d+) base, (\d+) skipped, (\d+) non-positive, 0 shortcut", r.stdout)
    assert m, r.stdout[-2000:]
    cases, tiles, base, skipped, nonpos = map(int, m.groups())
    assert cases >= 300
    # some tiles proven by the refinement alone, some kept, some positive: no side is vacuous
    assert 0 < base < skipped <= nonpos < tiles


def _crops(exe, path):
    r = subprocess.run([exe, "crops", str(path)], capture_output=True, text=True, timeout=900)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    level = int(re.search(r"level (\d)", r.stdout).group(1))
    rows = [tuple(map(int, m)) for m in ROW.findall(r.stdout)]
    assert len(rows) == len(DETS), r.stdout
    for _, tiles, bright, nokept, base, rh4, rh1, shipped, mismatch, shortcut, failures in rows:
        assert mismatch == 0 and shortcut == 0 and failures == 0, r.stdout
        assert 0 < base <= rh4 <= rh1 <= nokept <= bright <= tiles, r.stdout
        assert shipped == (rh1 if level == 1 else rh4), r.stdout
    return level, rows


def test_skipped_tiles_hold_no_positive_score(checker):
    """Synthetic detectors 9 to 70 wide at every in_x mod 8, outputs with
    oh % 4 of 1, 2, 3 and ow no multiple of 8 or 40, steps, blobs and noise."""
    _synth(checker)


def test_refinement_on_the_synthetic_frames(checker, crops):
    """Frames 0-8, all six detectors: the checker's fused chain reproduces the
    oracle's raw scores bit for bit (so the views hold the reference's
    windows), no skipped tile holds a positive score, the shortcut changes no
    flag, every detector proves strictly more tiles than the tile bound alone,
    and at least the floor of the shipped block height."""
    level, rows = _crops(checker, crops[9])
    floors = FLOORS[level]
    for (_, name, view, kind), (_, tiles, bright, nokept, base, rh4, rh1, shipped, _, _, _) in zip(DETS, rows):
        assert shipped > base, (name, base, shipped)
        floor = floors["tail" if kind else "side" if view else "bottom"]
        assert shipped >= floor * bright, (name, level, shipped, bright, shipped / bright, floor)


def test_refinement_is_clean_under_the_sanitizers(checker_san, crops):
    """The same program built with -fsanitize=address,undefined: the synthetic
    cases and frame 0; nothing is loaded into Python."""
    _synth(checker_san)
    _crops(checker_san, crops[1])
