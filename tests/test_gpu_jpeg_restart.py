"""Restart intervals in the device JPEG encoder (lm_enc_create_restart,
csrc/lm_jpeg_enc.hip): every file is compared byte for byte with Pillow's
restart_marker_blocks and with the host encoder's, alone and in mixed batches,
and the project's decoders read the files back."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import enc_harness as EH  # noqa: E402
import enc_rst_harness as RH  # noqa: E402
import jpeg_harness as JH  # noqa: E402

from locomouse_cpp_amd import abi, runtime  # noqa: E402

pytestmark = pytest.mark.gpu


def _fmt(tag):
    return abi.LM_ENC_GRAY8 if tag == "grey" else abi.LM_ENC_RGB24


@pytest.mark.parametrize("tag,h,w", RH.SHAPES, ids=[f"{t}_{h}x{w}" for t, h, w in RH.SHAPES])
def test_device_equals_pillow_and_host(tag, h, w):
    """Every case of the CPU test's list (intervals of 1 and 3 MCUs, a row, the MCU count and beyond), one batch per
    quality and interval."""
    pillow = dict(zip((c[0] for c in RH.cases()), RH.pillow_files()))
    groups = {}
    for name, img, q, ri, nm in RH.cases():
        if name.startswith(f"{tag}_{h}x{w}_"):
            groups.setdefault((q, ri), []).append((name, img, nm))
    assert len(groups) >= 12
    for (q, ri), group in groups.items():
        enc = runtime.JpegEncoder(h, w, _fmt(tag), quality=q, max_batch=len(group), restart_interval=ri)
        files = enc.encode(np.stack([img for _, img, _ in group]))
        for (name, img, nm), got in zip(group, files):
            assert got == pillow[name], f"{name}: {len(got)} bytes against Pillow's {len(pillow[name])}"
            assert got == RH.host_encode(img, q, ri), name
            assert len(RH.markers(got)) == nm and RH.dri(got) == ri, name
            assert len(got) <= enc.slot_bytes(h, w, _fmt(tag), ri)
        st = enc.stats()
        assert st["frames"] == len(group) and st["bytes_out"] == sum(map(len, files)) and st["device_ms"] > 0
        enc.close()


def _mixed(tag, h, w):
    """Five frames: noise, flat, edges (8 x 8 squares of 0 and 255), a smooth image, noise again."""
    rng = np.random.default_rng(h * 31 + w)
    y, x = np.mgrid[0:h, 0:w]
    grey = [rng.integers(0, 256, size=(h, w)), np.full((h, w), 200), (((x // 8) + (y // 8)) & 1) * 255,
            128 + 100 * np.sin(x / 9.0) * np.cos(y / 5.0), rng.integers(0, 256, size=(h, w))]
    frames = np.stack(grey).astype(np.uint8)
    if tag == "rgb":
        frames = np.stack([frames, frames[::-1], 255 - frames], axis=3)
    return np.ascontiguousarray(frames)


@pytest.mark.parametrize("tag,h,w,ri", [("grey", 17, 23, 1), ("grey", 24, 40, 2), ("rgb", 37, 53, 1), ("rgb", 37, 53, 5)])
def test_mixed_batch_and_max_batch(tag, h, w, ri):
    """Per-frame independence: noise, flat and edge frames in one batch, at max_batch 1 against 8, in another order,
    and after other calls on the same context."""
    frames = _mixed(tag, h, w)
    want = [RH.pillow_encode(f, 100, ri) for f in frames]
    assert len(want[1]) < len(want[0]) // 2  # a flat frame (a few bytes an interval) next to quality-100 noise
    one = runtime.JpegEncoder(h, w, _fmt(tag), quality=100, max_batch=1, restart_interval=ri)
    eight = runtime.JpegEncoder(h, w, _fmt(tag), quality=100, max_batch=8, restart_interval=ri)
    assert eight.encode(frames) == want
    assert [one.encode(frames[i:i + 1])[0] for i in range(5)] == want
    order = [4, 1, 0, 2]
    assert eight.encode(frames[order]) == [want[i] for i in order]
    assert eight.encode(frames[1:2]) == want[1:2]
    one.close()
    eight.close()


def test_interval_zero_is_the_plain_context():
    h, w = 24, 40
    frames = _mixed("grey", h, w)
    plain = runtime.JpegEncoder(h, w, abi.LM_ENC_GRAY8, quality=90, max_batch=5)
    zero = runtime.JpegEncoder(h, w, abi.LM_ENC_GRAY8, quality=90, max_batch=5, restart_interval=0)
    files = zero.encode(frames)
    assert files == plain.encode(frames) == [EH.pillow_encode(f, 90) for f in frames]
    assert all(RH.dri(j) is None for j in files)
    plain.close()
    zero.close()


@pytest.mark.parametrize("tag,h,w,ris", [("grey", 128, 136, (1, 7, 17)), ("rgb", 112, 128, (1, 5))])
def test_more_blocks_and_bytes_than_one_round(tag, h, w, ris):
    """272 grey blocks (336 colour ones): more than one round of the 256-wide scan, with interval ends on both sides of
    the round's edge; quality-100 noise is several rounds of k_enc_write's 4096 bytes, so markers fall inside a
    thread's 16 bytes, at their start, and across rounds.  The frames come from device memory with a wide pitch."""
    import torch
    frames = _mixed(tag, h, w)[:3]
    n, fb = len(frames), frames[0].size
    pitch = fb + 64
    buf = np.zeros(n * pitch, np.uint8)
    for i in range(n):
        buf[i * pitch:i * pitch + fb] = frames[i].reshape(-1)
    d = torch.from_numpy(buf).cuda()
    torch.cuda.synchronize()
    for ri in ris:
        enc = runtime.JpegEncoder(h, w, _fmt(tag), quality=100, max_batch=n, restart_interval=ri)
        files = enc.encode_device(d.data_ptr(), n, pitch=pitch)
        for i in range(n):
            assert files[i] == RH.pillow_encode(frames[i], 100, ri), (ri, i)
        assert len(files[0]) > 3 * 4096
        assert len(RH.markers(files[0])) == RH.intervals(h, w, EH.GRAY8 if tag == "grey" else EH.RGB24, ri) - 1
        enc.close()


def test_decoders_take_the_encoders_restart_files():
    """JpegDecoder on the device encoder's restart files: LM_JPEG_OK, and the host decoder's pixels."""
    for tag, h, w, ri in (("grey", 24, 40, 1), ("grey", 128, 136, 1), ("rgb", 37, 53, 2), ("grey", 17, 23, 3)):
        frames = _mixed(tag, h, w)[:4]
        for q in (90, 100):
            enc = runtime.JpegEncoder(h, w, _fmt(tag), quality=q, max_batch=4, restart_interval=ri)
            files = enc.encode(frames)
            enc.close()
            for j in files:
                assert runtime.jpeg_probe(j)["status"] == abi.LM_JPEG_OK
            dec = runtime.JpegDecoder(h, w, max_batch=4)
            out, status = dec.decode(files)
            assert (status == abi.LM_JPEG_OK).all(), (tag, h, w, q, status)
            got = out.cpu().numpy()
            dec.close()
            for i, j in enumerate(files):
                assert np.array_equal(got[i], JH.host_decode(j, h, w)), (tag, h, w, q, ri, i)


# ---- the decoder's interval path (k_jpeg_scan_rst) against the subsequence path and the host decoder
import functools  # noqa: E402

import jpeg_rst_harness as JR  # noqa: E402
import media_writers as MW  # noqa: E402

H, W = 128, 136


@functools.lru_cache(maxsize=None)
def _batch():
    """[(name, jpeg, lanes, handed over)] of 128 x 136 frames: with and without DRI, another interval in every frame,
    two Huffman table sets next to each other in one workgroup's lanes, the 272-interval frame, and damaged ones."""
    f = JH.frames(6, H, W, 2026)

    def enc(i, **kw):
        return MW.jpeg_frames(f[i:i + 1], **kw)[0]

    g1 = enc(0, mode="L", quality=90, restart_marker_blocks=1)                      # 272 intervals
    g7 = enc(1, mode="L", quality=75, restart_marker_blocks=7)                      # 39
    c3 = enc(2, mode="RGB", quality=85, subsampling=2, restart_marker_blocks=3)     # 72 MCUs: 24
    o17 = enc(3, mode="RGB", quality=85, subsampling=0, restart_marker_blocks=17, optimize=True)  # 272 MCUs: 16
    row = enc(4, mode="RGB", quality=60, subsampling=1, restart_marker_rows=1)      # 16 rows of 9 MCUs
    whole = enc(5, mode="L", quality=90, restart_marker_blocks=272)                 # DRI, one interval: no lane
    out = [("grey_ri1", g1, 272, 0), ("plain_grey", enc(1, mode="L", quality=90), 0, 0), ("grey_ri7", g7, 39, 0),
           ("optimized_444_ri17", o17, 16, 0), ("420_ri3", c3, 24, 0), ("plain_420", enc(2, mode="RGB", quality=85, subsampling=2), 0, 0),
           ("422_rows", row, 16, 0), ("one_interval", whole, 0, 0),
           ("dri_without_markers", JH.with_dri(enc(0, mode="L", quality=90), 5), 0, 1),
           ("without_last", JH.without_last_rst(g7), 0, 1), ("without_middle", JR.without_marker(c3, 11), 0, 1),
           ("numbers_swapped", JR.with_markers_swapped(g1, 100, 101), 272, 0),
           ("intervals_swapped", JR.with_intervals_swapped(o17, 4), 16, 0), ("truncated", JH.cut_scan(g1, 0.8), 0, 1)]
    # (two whole intervals of equal length that change places are a valid stream of another image)
    # a scan damaged inside one interval, every marker in place: the lanes run, one is irregular
    s, e = JH.scan_bounds(g7)
    p = JR.marker_positions(g7)[20] + 2
    broken = bytearray(g7)
    broken[p:p + 6] = b"\x00\x01\x02\x03\x04\x05"
    out.append(("broken_interval", bytes(broken), 39, 1))
    return tuple(out)


def test_batch_is_what_it_claims():
    tables = set()
    for name, j, lanes, handed in _batch():
        if lanes:
            assert len(JR.marker_positions(j)) == lanes - 1, name
        cls, px, coef, st, why = JR.intervals_decode(j, H, W)
        assert st["intervals"] == lanes and st["handed_over"] == handed, (name, st)
        assert (cls == 0) == (not handed), name
        i = j.index(b"\xff\xc4")
        tables.add(j[i:j.index(b"\xff\xda")])
    assert len(tables) >= 3  # grey, colour and optimised Huffman tables


def test_interval_path_on_against_off_and_host():
    names = [b[0] for b in _batch()]
    jpegs = [b[1] for b in _batch()]
    want = [JH.lanes_decode(j, H, W) for j in jpegs]
    dec = runtime.JpegDecoder(H, W, max_batch=len(jpegs))
    on, st_on = dec.decode(jpegs)
    on, st_on = on.cpu().numpy(), st_on.copy()
    ist, stats_on = dec.interval_stats(), dec.stats()
    dec.set_interval_path(False)
    off, st_off = dec.decode(jpegs)
    off, st_off = off.cpu().numpy(), st_off.copy()
    ist_off, stats_off = dec.interval_stats(), dec.stats()
    assert np.array_equal(st_on, st_off), dict(zip(names, zip(st_on, st_off)))
    assert st_on.tolist() == [abi.LM_JPEG_OK if w[0] == 0 else abi.LM_JPEG_NEEDS_HOST for w in want]
    for i, name in enumerate(names):
        assert np.array_equal(on[i], off[i]), name  # (a frame that needs the host: the same undefined bytes, too)
        if st_on[i] == abi.LM_JPEG_OK:
            assert np.array_equal(on[i], JH.host_decode(jpegs[i], H, W)), name
    # the counts
    lanes = sum(b[2] for b in _batch())
    ran = [b for b in _batch() if b[2]]
    assert ist["intervals"] == lanes and ist["frames_interval"] == sum(1 for b in ran if not b[3])
    assert ist["frames_handed_over"] == sum(b[3] for b in _batch()) >= 5
    s, e = JH.scan_bounds(jpegs[names.index("optimized_444_ri17")])
    p = JR.marker_positions(jpegs[names.index("optimized_444_ri17")])
    assert ist["longest_interval_bytes"] >= max(b - a for a, b in zip([s] + [q + 2 for q in p], p + [e]))
    assert ist["parse_ms"] > 0
    assert (ist_off["intervals"], ist_off["frames_interval"], ist_off["frames_handed_over"]) == (0, 0, 0)
    # lm_jpeg_stats keeps its meaning: the subsequences of every frame, whichever path took it
    assert stats_on["subsequences"] == stats_off["subsequences"] > 0
    assert stats_on["frames_needing_host"] == stats_off["frames_needing_host"] == sum(1 for w in want if w[0])
    assert stats_on["table_sets"] == stats_off["table_sets"] >= 3
    # back on, smaller batches on the same context, in another order
    dec.set_interval_path(True)
    for sel in ([0], [11, 3, 9, 4], list(range(len(jpegs)))[::-1]):
        out, st = dec.decode([jpegs[i] for i in sel])
        assert st.tolist() == [int(st_on[i]) for i in sel]
        got = out.cpu().numpy()
        for k, i in enumerate(sel):
            assert np.array_equal(got[k], on[i]), (sel, names[i])
    dec.close()


def test_interval_path_default_follows_the_environment():
    j = _batch()[0][1]
    for value, lanes in (("0", 0), ("1", 272), (None, 272)):
        old = os.environ.pop("LM_JPEG_RST", None)
        if value is not None:
            os.environ["LM_JPEG_RST"] = value
        try:
            dec = runtime.JpegDecoder(H, W, max_batch=1)
        finally:
            os.environ.pop("LM_JPEG_RST", None)
            if old is not None:
                os.environ["LM_JPEG_RST"] = old
        out, st = dec.decode([j])
        assert st.tolist() == [abi.LM_JPEG_OK] and dec.interval_stats()["intervals"] == lanes
        assert np.array_equal(out.cpu().numpy()[0], JH.host_decode(j, H, W))
        dec.close()


def test_round_trip_encode_with_restarts_then_decode():
    for tag, h, w, ri in (("grey", 128, 136, 8), ("grey", 24, 40, 1), ("rgb", 37, 53, 2)):
        frames = _mixed(tag, h, w)
        enc = runtime.JpegEncoder(h, w, _fmt(tag), quality=92, max_batch=5, restart_interval=ri)
        files = enc.encode(frames)
        enc.close()
        dec = runtime.JpegDecoder(h, w, max_batch=5)
        out, status = dec.decode(files)
        assert (status == abi.LM_JPEG_OK).all()
        ist = dec.interval_stats()
        assert ist["frames_interval"] == 5 and ist["frames_handed_over"] == 0
        assert ist["intervals"] == 5 * RH.intervals(h, w, EH.GRAY8 if tag == "grey" else EH.RGB24, ri)
        got = out.cpu().numpy()
        dec.close()
        for i, j in enumerate(files):
            assert np.array_equal(got[i], JH.host_decode(j, h, w)), (tag, i)


# ---- the program: a video transcoded once, then tracked with LM_DECODE=device through the interval path
def _timing(out):
    lines = [ln for ln in out.splitlines() if ln.startswith("LM_TIMING ")]
    assert len(lines) == 1, out
    f = lines[0].split()[1:]
    return {k: float(v) for k, v in zip(f[::2], f[1::2])}


def test_program_transcodes_and_tracks_through_the_interval_path(tmp_path):
    import subprocess

    from locomouse_cpp_amd import synthetic as S
    from test_cli import cli_args, run_cli
    cfg = S.SyntheticConfig()
    n = 40
    paths = MW.write_inputs(str(tmp_path), cfg, n, stem="mouse_R", bits=24, jpeg=dict(mode="RGB", quality=92, subsampling=2))
    source = paths["video"]
    avi = str(tmp_path / "restart" / "mouse_R.avi")
    os.makedirs(os.path.dirname(avi))
    p = subprocess.run([runtime.TRANSCODE_CLI_PATH, source, avi, "92:8"], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, LM_BATCH="16"))
    assert p.returncode == 0 and f"Transcoded {n} frames" in p.stdout, p.stdout + p.stderr
    # the file: grey JPEG frames with a restart interval of 8 MCUs, channel 0 of the source's frames, re-encoded
    rows, cols = cfg.rows, cfg.cols
    info = EH.avi_info(avi)
    assert info == dict(rows=rows, cols=cols, frames=n, fps=EH.avi_info(source)["fps"] or 30, mjpeg=True)
    chunks = EH.avi_chunks(avi)
    src = EH.avi_frames(source)
    ni = RH.intervals(rows, cols, EH.GRAY8, 8)
    for i in (0, 17, n - 1):
        assert chunks[i] == RH.pillow_encode(src[i], 92, 8), i
        pr = runtime.jpeg_probe(chunks[i])
        assert (pr["status"], pr["components"], pr["restart_interval"]) == (abi.LM_JPEG_OK, 1, 8)
        assert len(RH.markers(chunks[i])) == ni - 1
    # a decoder of its own on the file's frames: every frame through the interval path
    dec = runtime.JpegDecoder(rows, cols, max_batch=n)
    out, status = dec.decode(chunks)
    ist = dec.interval_stats()
    dec.close()
    assert (status == abi.LM_JPEG_OK).all()
    assert (ist["frames_interval"], ist["frames_handed_over"], ist["intervals"]) == (n, 0, n * ni)
    assert np.array_equal(out.cpu().numpy(), EH.avi_frames(avi))
    # the program on the transcoded file: the device decoder's tracks are the host decoder's
    got = {}
    for mode in ("host", "device"):
        d = tmp_path / mode
        d.mkdir()
        rc, text = run_cli(cli_args(dict(paths, video=avi), side="R", outdir=str(d)),
                           env={"LM_BATCH": "16", "LM_DECODE": mode, "LM_TIMING": "1"})
        assert rc == 0, (mode, text)
        got[mode] = ((d / "output_mouse_R.yml").read_bytes(), _timing(text))
    assert got["host"][0] == got["device"][0] and len(got["host"][0]) > 1000
    t = got["device"][1]
    assert t["decode_fallback_frames"] == 0 and t["decode_device_ms"] > 0 and t["frames"] == n
    # and with the interval path switched off in the same build: the same file
    d = tmp_path / "off"
    d.mkdir()
    rc, text = run_cli(cli_args(dict(paths, video=avi), side="R", outdir=str(d)),
                       env={"LM_BATCH": "16", "LM_DECODE": "device", "LM_TIMING": "1", "LM_JPEG_RST": "0"})
    assert rc == 0, text
    assert (d / "output_mouse_R.yml").read_bytes() == got["device"][0] and _timing(text)["decode_fallback_frames"] == 0
