"""The fp32 screen in front of the refinement's block sum on the GPU
(LM_TILE_SCREEN, default 1: k_tile_bound<true> sums a block in fp32 first and in
double only where the fp32 value lies within its margin of zero, csrc/
lm_tail_bound.h: lm_tbs_*).  The method is test_gpu_tile_refine_dense.py's: one
batch with the screen on, with LM_TILE_SCREEN=0 and through k_tile_bound_ref;
the results are bit-identical to each other and to the oracle, the flags and
work counters equal.  The kernel's count of the block sums that took the double
path must equal what the host checker (tests/cpp/tile_screen_check.cpp) finds
undecided on the same views, over the blocks of the tiles a fourth batch with
LM_TILE_REFINE=0 lists (the tiles the tile bound fails)."""
import re
import subprocess

import numpy as np
import pytest

from locomouse_cpp_amd import runtime as rt
from locomouse_cpp_amd import synthetic as S
from test_gpu_parity import _oracle, assert_same
from test_gpu_tile_bound import _assert_state_equal, _state
from test_tile_refine import DETS
from test_tile_screen import VIEW, _build
from test_tile_sum_rows import write_views

pytestmark = pytest.mark.gpu

# (name, LM_TILE_SCREEN, LM_TILE_REFINE, LM_TILE_BOUND_REF)
MODES = (("on", "1", "1", "0"), ("off", "0", "1", "0"), ("ref", "1", "1", "1"), ("norefine", "1", "0", "0"))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("tile_screen_gpu") / "tile_screen_check"), ["-O2"])


def _four(cfg, frames, monkeypatch, label):
    """One batch per mode: (results, state, fallback count) each; the first
    three modes compared with each other and with the oracle."""
    n = len(frames)
    out = {}
    for mode, screen, refine, ref in MODES:
        monkeypatch.setenv("LM_TILE_SCREEN", screen)
        monkeypatch.setenv("LM_TILE_REFINE", refine)
        monkeypatch.setenv("LM_TILE_BOUND_REF", ref)
        ctx = rt.Context(cfg, max_batch=n)
        got = ctx.detect(frames, 0)
        out[mode] = (got, _state(ctx, n), ctx.screen_fallback())
        ctx.close()
    print(label, {m: (out[m][1][0], out[m][1][1], out[m][2]) for m in out})
    assert_same(out["on"][0], out["off"][0], label + "screen on against off: ")
    assert_same(out["on"][0], out["ref"][0], label + "screen on against the reference kernel: ")
    assert_same(out["on"][0], _oracle(cfg, frames).result, label)
    _assert_state_equal(out["on"][1], out["off"][1], label + "screen on against off: ")
    _assert_state_equal(out["on"][1], out["ref"][1], label + "screen on against the reference kernel: ")
    assert out["off"][2] == 0 and out["ref"][2] == 0 and out["norefine"][2] == 0, (label, {m: out[m][2] for m in out})
    return out


def _host_undecided(checker, cfg, frames, state, tmp_path, flip=False):
    """The checker's rows (detector, screened, items, negative, undecided) over
    the blocks of the tiles set in `state`'s flags (a batch with
    LM_TILE_REFINE=0: the tiles the tile bound fails)."""
    n = len(frames)
    _, _, pt, tt = state
    views = write_views(cfg, frames, tmp_path / "views.bin", flip=flip)
    blob = []
    for det, _, view, kind in DETS:
        for f in range(n):
            flags = tt[f * 2 + view] if kind else pt[f * 4 + (0, 1, None, 2, 3)[det]]
            blob.append(np.ascontiguousarray(flags != 0, dtype=np.uint8).tobytes())
    with open(tmp_path / "masks.bin", "wb") as fh:
        fh.write(b"".join(blob))
    r = subprocess.run([checker, "views", str(views), str(tmp_path / "masks.bin")], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rows = [tuple(map(int, m)) for m in VIEW.findall(r.stdout)]
    assert len(rows) == len(DETS) and all(row[5] == 0 and row[6] == 0 for row in rows), rows
    return [row[:5] for row in rows]


@pytest.mark.parametrize("flip", [False, True])
def test_default_c3(flip, checker, monkeypatch, tmp_path):
    """Frames 20-23 of the default scene: some block sums are undecided (6
    without the flip and 4 with it on the host), and the kernel counts as many."""
    cfg = S.SyntheticConfig(flip=flip)
    frames = cfg.frames(20, 4)
    out = _four(cfg, frames, monkeypatch, f"C3 flip {flip}: ")
    rows = _host_undecided(checker, cfg, frames, out["norefine"][1], tmp_path, flip=flip)
    host = sum(r[4] for r in rows)
    assert all(r[1] == 1 and r[2] > 0 for r in rows), rows
    assert host > 0, rows
    assert out["on"][2] == host, (out["on"][2], rows)


def test_short_last_column_and_row(checker, monkeypatch, tmp_path):
    """Bottom 390 x 139, side 390 x 89: a last tile column of 30 outputs (four
    blocks; the lanes of its fifth do nothing) and last tile rows of three
    rows and of one, which are summed in double from the block ranges and are
    not the screen's: the host count leaves them out, and the counts agree."""
    cfg = S.SyntheticConfig(bounding_boxes={"side": (300, 3, 390, 89), "bottom": (300, 106, 390, 139)})
    frames = cfg.frames(40, 3)
    out = _four(cfg, frames, monkeypatch, "short column and row: ")
    rows = _host_undecided(checker, cfg, frames, out["norefine"][1], tmp_path)
    assert all(r[1] == 1 and r[2] > 0 for r in rows), rows
    assert out["on"][2] == sum(r[4] for r in rows), (out["on"][2], rows)
    pw, tw, pw0, tw0 = out["on"][1][0], out["on"][1][1], out["norefine"][1][0], out["norefine"][1][1]
    assert all(a < b for a, b in zip(pw["listed"], pw0["listed"])) and all(a < b for a, b in zip(tw["listed"], tw0["listed"]))


def test_one_detector_without_the_screen(checker, monkeypatch, tmp_path):
    """paw_side with a weight row of zeros but for one tap of 1e-41: that tap
    group's constant is below FLT_MIN, so the gate switches the detector's
    screen off while its bound and its refinement stay (the tap adds at most
    2.6e-39 to a score, below every rounding); the other five are screened.
    Both loops run in one launch."""
    w = S.SyntheticConfig().weights["paw_side"].astype(np.float32).copy()
    w[3, :] = 0.0
    w[3, 0] = np.float32(1e-41)
    cfg = S.SyntheticConfig(weights={"paw_side": w})
    frames = cfg.frames(20, 3)
    out = _four(cfg, frames, monkeypatch, "paw_side unscreened: ")
    rows = _host_undecided(checker, cfg, frames, out["norefine"][1], tmp_path)
    assert [r[1] for r in rows] == [1, 1, 1, 0, 1, 1], rows
    assert out["on"][2] == sum(r[4] for r in rows), (out["on"][2], rows)
    pw, pw0 = out["on"][1][0], out["norefine"][1][0]
    assert 0 < pw["listed"][2] < pw0["listed"][2], (pw, pw0)  # (paw_side is still refined, in double)


def test_c5(monkeypatch):
    """C5's detectors have more than four tap groups: k_tile_bound<false>, the
    generic loop alone, and nothing is counted."""
    c5 = S.SyntheticConfig(rows=512, cols=1920)
    out = _four(c5, c5.frames(10, 2), monkeypatch, "C5: ")
    assert out["on"][2] == 0, out["on"][2]
    tw, tw0 = out["on"][1][1], out["norefine"][1][1]
    assert sum(tw["listed"]) < sum(tw0["listed"]), (tw, tw0)
