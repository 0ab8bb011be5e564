"""The block sum's form for detectors of one chunk per row (locomouse_cpp_amd/
csrc/lm_tail_bound.h: lm_tbr_sum_rows, which k_tile_bound<true> runs in step
4b) on the host, without a GPU: a stand-alone program (tests/cpp/
tile_sum_rows_check.cpp) checks that lm_tbr_sum_rows returns lm_tbr_sum's U
bit for bit (kh 1 to 40, 1 to 4 tap groups at every in_x mod 8, random ranges,
biases that put U at zero and a few ulps to either side).  The program also
holds the order "a tile's end blocks first, the blocks between them only while
it is unmarked", which was measured in the kernel and not kept there (DESIGN.md
section 12): it checks that the order over lm_tbr_block_skip's flags marks a
tile exactly when lm_tbr_tile_skip keeps it, last tile columns of one to five
blocks included, and counts the block sums each order needs on the views of
synthetic C3 frames 0-23.  Once more under the sanitizers."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from locomouse_cpp_amd import synthetic as S
from test_tail_bound import _normalised
from test_tile_refine import DETS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "tile_sum_rows_check.cpp")
INC = "-I" + os.path.join(ROOT, "locomouse_cpp_amd", "csrc")
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
SUMS = re.compile(r"(\d+) cases, (\d+) sums, (\d+) negative, (\d+) zero, (\d+) positive, (\d+) calls differ, (\d+) failures")
ROUNDS = re.compile(r"(\d+) tiles, (\d+) kept by an end, (\d+) kept by a middle block only, (\d+) proven, (\d+) short columns, "
                    r"(\d+) failures")
VIEW = re.compile(r"det (\d): refined (\d+) kept (\d+) ends (\d+) all (\d+) ends_first (\d+) sequential (\d+) short (\d+) failures (\d+)")


def _build(exe, flags):
    subprocess.check_call(["g++", *flags, "-std=c++17", "-ffp-contract=off", INC, SRC, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("tile_sum_rows") / "tile_sum_rows_check"), ["-O2"])


@pytest.fixture(scope="module")
def checker_san(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("tile_sum_rows_san") / "tile_sum_rows_check_san"), SAN)


def write_views(cfg, frames, path, flip=False):
    """The six detectors' views of `frames`, as tests/test_tile_refine.py's
    fixture builds them (without the oracle's scores, which nothing here
    reads): a view is the detector's window as the runtime's ext crop holds it.
    flip: the normalised frame mirrored left to right, as the pipeline does
    with setup.flip."""
    from oracle import oracle as O
    g = O.geometry(cfg)
    p = cfg.params
    pad = 96
    norm = [np.pad(_normalised(cfg, fr)[:, ::-1] if flip else _normalised(cfg, fr), pad) for fr in frames]
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
        for f in range(len(frames)):
            y0, x0 = pad + box.y + 1 - kh // 2 - in_y, pad + box.x + 1 - kw // 2 - in_x
            ext = np.ascontiguousarray(norm[f][y0:y0 + eh, x0:x0 + ew])
            assert ext.shape == (eh, ew)
            blob.append(ext.tobytes())
    with open(path, "wb") as fh:
        fh.write(b"".join(blob))
    return path


def _run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def _sums(exe):
    m = SUMS.search(_run(exe, "sums"))
    assert m
    cases, sums, neg, zero, pos, calls, failures = map(int, m.groups())
    assert failures == 0 and calls == 0
    # kh 1 .. 40 x 1 .. 4 groups x 8 residues (one group at residue a holds at most 8 - a taps: every residue has one)
    assert cases == 40 * 4 * 8 and sums == cases * 4 * 8
    # the sign test on both sides of zero and at it
    assert neg > 0 and pos > 0 and zero > 0, (neg, zero, pos)


def _rounds(exe):
    m = ROUNDS.search(_run(exe, "rounds"))
    assert m
    tiles, ends, middle, proven, short, failures = map(int, m.groups())
    assert failures == 0
    assert ends > 0 and middle > 0 and proven > 0 and short > 0 and ends + middle + proven == tiles, m.groups()


def _views(exe, path, every=True):
    out = _run(exe, "views", path)
    rows = [tuple(map(int, m)) for m in VIEW.findall(out)]
    assert len(rows) == len(DETS), out
    for _, refined, kept, ends, alls, ends_first, sequential, _, failures in rows:
        assert failures == 0, out
        assert (0 < ends or not every) and ends <= kept <= refined and max(sequential, ends_first) <= alls, out
    return rows


def test_row_loop_returns_the_same_sum(checker):
    _sums(checker)


def test_two_rounds_mark_what_the_tile_rule_keeps(checker):
    _rounds(checker)


def test_sums_per_order_on_the_synthetic_frames(checker, tmp_path):
    """Frames 0-23 of the default C3 scene: every order marks the same tiles;
    ends first needs fewer block sums than all blocks of every refined tile
    for every detector (the figures are printed; DESIGN.md section 12 and
    profiles/tileround/README.md quote them)."""
    cfg = S.SyntheticConfig()
    rows = _views(checker, write_views(cfg, cfg.frames(0, 24), tmp_path / "views24.bin"))
    for _, refined, kept, ends, alls, ends_first, sequential, _, _ in rows:
        assert ends_first < alls, rows


def test_clean_under_the_sanitizers(checker_san, tmp_path):
    """The same program built with -fsanitize=address,undefined: both synthetic
    modes and the views of frame 0; nothing is loaded into Python."""
    _sums(checker_san)
    _rounds(checker_san)
    cfg = S.SyntheticConfig()
    _views(checker_san, write_views(cfg, cfg.frames(0, 1), tmp_path / "views1.bin"), every=False)
