"""Device JPEG decode on the GPU (include/locomouse_jpeg.h): every stream of
the shared list decodes with status LM_JPEG_OK, no fallback, to the host
decoder's bytes, at the smallest and the default subsequence size; out-of-scope
and damaged frames come back with their status; decoded frames feed the
detection path in device memory."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_harness as JH  # noqa: E402

from locomouse_cpp_amd import abi, runtime  # noqa: E402

pytestmark = pytest.mark.gpu

STREAMS = JH.stream_list()
SUBSEQS = (abi.LM_JPEG_SUBSEQ_MIN, 0)  # the minimum, and the default


def _want(rows, cols, jpegs):
    out = [JH.host_decode(j, rows, cols) for j in jpegs]
    assert not any(isinstance(w, str) for w in out), out
    return np.stack(out)


def _decode(dec, jpegs):
    import torch
    d, status = dec.decode(jpegs)
    torch.cuda.synchronize()
    return d.cpu().numpy(), status


@pytest.mark.parametrize("subseq", SUBSEQS, ids=["subseq_min", "subseq_default"])
def test_streams_decode_to_the_host_decoders_bytes(subseq):
    """One context per frame size; every case of the list, each as one batch."""
    decs = {}
    try:
        for name, rows, cols, jpegs in STREAMS:
            dec = decs.get((rows, cols))
            if dec is None:
                dec = decs[(rows, cols)] = runtime.JpegDecoder(rows, cols, max_batch=3, subseq_bytes=subseq)
            got, status = _decode(dec, jpegs)
            st = dec.stats()
            assert status.tolist() == [abi.LM_JPEG_OK] * len(jpegs), (name, status, st)
            assert st["frames_needing_host"] == 0, (name, st)
            s = subseq or abi.LM_JPEG_SUBSEQ_DEFAULT
            assert st["subsequences"] == sum(-(-(e - b) // s) for b, e in map(JH.scan_bounds, jpegs)), (name, st)
            assert st["sync_rounds"] <= st["subsequences"] and st["max_chunk_rounds"] <= abi.LM_JPEG_CHUNK
            bad = np.argwhere(got != _want(rows, cols, jpegs))
            assert bad.size == 0, f"{name}: {len(bad)} samples differ, first {bad[:4].tolist()}"
            if name.startswith("optimize"):  # every frame brings its own tables
                assert st["table_sets"] == len(jpegs)
            if name == "long_scan":  # the cross-wave and cross-chunk carries run
                assert st["max_subsequences"] > 3 * abi.LM_JPEG_CHUNK, st
            if name == "flat" and not subseq:
                assert st["subsequences"] == 1
    finally:
        for d in decs.values():
            d.close()


def test_q100_streams_contain_stuffed_bytes():
    by = {s[0]: s for s in STREAMS}
    for n in ("grey_q100", "colour_q100_range_limit"):
        assert all(b"\xff\x00" in j[slice(*JH.scan_bounds(j))] for j in by[n][3])


def _mixed_batch(rows, cols):
    """Frames of one size with scans from a few bytes to many chunks, grey and
    colour, with and without restart markers and DHT, several table sets."""
    import media_writers as MW
    rng = np.random.default_rng(7)
    noisy = rng.integers(0, 256, size=(1, rows, cols)).astype(np.uint8)
    f = JH.frames(4, rows, cols, 21)
    js = MW.jpeg_frames(np.full((1, rows, cols), 90, np.uint8), mode="L", quality=50)
    js += MW.jpeg_frames(noisy, mode="L", quality=95)
    js += MW.jpeg_frames(f[:1], mode="RGB", quality=85, subsampling=2)
    js += MW.jpeg_frames(f[1:2], mode="RGB", quality=70, subsampling=1, strip_dht=True)
    js += MW.jpeg_frames(f[2:3], mode="RGB", quality=90, subsampling=0, optimize=True)
    js += MW.jpeg_frames(f[3:4], mode="L", quality=80, restart_marker_blocks=5, optimize=True)
    js += MW.jpeg_frames(noisy, mode="RGB", quality=100, subsampling=0, restart_marker_rows=1)
    return js


@pytest.mark.parametrize("subseq", SUBSEQS, ids=["subseq_min", "subseq_default"])
def test_one_batch_mixes_all_sizes_of_scan(subseq):
    rows, cols = 64, 176
    js = _mixed_batch(rows, cols)
    sizes = [e - b for b, e in map(JH.scan_bounds, js)]
    # from a corner of one chunk to more than three chunks (a scan below one subsequence: "flat" of the list)
    chunk_bytes = abi.LM_JPEG_CHUNK * abi.LM_JPEG_SUBSEQ_DEFAULT
    assert min(sizes) < chunk_bytes // 16 and max(sizes) > 3 * chunk_bytes
    dec = runtime.JpegDecoder(rows, cols, max_batch=len(js), subseq_bytes=subseq)
    try:
        got, status = _decode(dec, js)
        st = dec.stats()
        assert status.tolist() == [abi.LM_JPEG_OK] * len(js) and st["frames_needing_host"] == 0, (status, st)
        assert st["table_sets"] >= 4
        assert np.array_equal(got, _want(rows, cols, js))
    finally:
        dec.close()


def test_context_reused_with_batches_of_1_3_2():
    name, rows, cols, _ = STREAMS[0]
    import media_writers as MW
    js = MW.jpeg_frames(JH.frames(6, rows, cols, 99), mode="RGB", quality=88, subsampling=2)
    want = _want(rows, cols, js)
    dec = runtime.JpegDecoder(rows, cols, max_batch=3)
    try:
        at = 0
        for n in (1, 3, 2):
            got, status = _decode(dec, js[at:at + n])
            assert status.tolist() == [abi.LM_JPEG_OK] * n and dec.stats()["frames_needing_host"] == 0
            assert np.array_equal(got, want[at:at + n])
            at += n
        with pytest.raises(runtime.LMError):
            dec.decode(js[:4])  # more than max_batch
    finally:
        dec.close()


def test_out_of_scope_and_damaged_frames():
    """16-bit tables and a cut scan need the host; progressive is rejected with
    the host decoder's message; good frames of the same batch still decode,
    and so does the next call on the context."""
    rows, cols, prog = JH.progressive_stream()
    import media_writers as MW
    good = MW.jpeg_frames(JH.frames(2, rows, cols, 5), mode="RGB", quality=85, subsampling=2)
    qt = [[257 + 27 * i for i in range(64)]]
    q16 = MW.jpeg_frames(JH.frames(1, rows, cols, 6), mode="L", qtables=qt)[0]
    assert q16.find(b"\xff\xc1") >= 0
    cut = JH.cut_scan(good[1], 0.7)
    other_size = MW.jpeg_frames(JH.frames(1, rows + 8, cols, 5), mode="L")[0]
    want = _want(rows, cols, good)
    for subseq in SUBSEQS:
        dec = runtime.JpegDecoder(rows, cols, max_batch=6, subseq_bytes=subseq)
        try:
            got, status = _decode(dec, [good[0], q16, prog, cut, other_size, good[1]])
            assert status.tolist() == [abi.LM_JPEG_OK, abi.LM_JPEG_NEEDS_HOST, abi.LM_JPEG_REJECTED,
                                       abi.LM_JPEG_NEEDS_HOST, abi.LM_JPEG_NEEDS_HOST, abi.LM_JPEG_OK]
            assert runtime.lib().lm_last_error().decode() == JH.host_decode(prog, rows, cols)
            assert dec.stats()["frames_needing_host"] == 4
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[5], want[1])
            # the host decoder gives the frames the device handed back
            assert not isinstance(JH.host_decode(q16, rows, cols), str)
            assert not isinstance(JH.host_decode(cut, rows, cols), str)
            got, status = _decode(dec, good)  # the context is unharmed
            assert status.tolist() == [abi.LM_JPEG_OK] * 2 and np.array_equal(got, want)
        finally:
            dec.close()
    # restart markers the DRI interval asks for but the scan lacks (none at all; the last one)
    by = {s[0]: s for s in STREAMS}
    for name, damage in (("grey_q50", lambda j: JH.with_dri(j, 3)), ("colour_s2_37x53", lambda j: JH.with_dri(j, 3)),
                         ("restart_blocks3_L", JH.without_last_rst), ("restart_rows1_RGB", JH.without_last_rst)):
        _, r, c, jpegs = by[name]
        for subseq in SUBSEQS:
            dec = runtime.JpegDecoder(r, c, max_batch=2, subseq_bytes=subseq)
            try:
                got, status = _decode(dec, [damage(jpegs[0]), jpegs[1]])
                assert status.tolist() == [abi.LM_JPEG_NEEDS_HOST, abi.LM_JPEG_OK], (name, subseq, status)
                assert np.array_equal(got[1], JH.host_decode(jpegs[1], r, c))
            finally:
                dec.close()
    for r, c, j in JH.sixteen_bit_streams():
        dec = runtime.JpegDecoder(r, c, max_batch=1)
        try:
            assert dec.decode([j])[1].tolist() == [abi.LM_JPEG_NEEDS_HOST]
        finally:
            dec.close()


def test_decoded_frames_feed_detection_in_device_memory():
    import torch

    import media_writers as MW
    from locomouse_cpp_amd import synthetic as S
    cfg = S.SyntheticConfig()
    frames = cfg.frames(0, 4)
    rows, cols = frames.shape[1:]
    js = MW.jpeg_frames(frames, mode="L", quality=90)
    host = _want(rows, cols, js)
    dec = runtime.JpegDecoder(rows, cols, max_batch=4)
    ctx = runtime.Context(cfg, max_batch=4, device=0)
    try:
        d, status = dec.decode(js)
        assert status.tolist() == [abi.LM_JPEG_OK] * 4 and dec.stats()["frames_needing_host"] == 0
        torch.cuda.synchronize()
        assert np.array_equal(d.cpu().numpy(), host)
        got = ctx.detect_device(d.data_ptr(), rows * cols, 4, 0, raw=False)
        ref = runtime.Context(cfg, max_batch=4, device=0)
        try:
            want = ref.detect(host, 0)
        finally:
            ref.close()
        assert int(want["cand_offset"][-1]) > 0
        for k in ("cand_offset", "cand", "p22d", "side_y", "side_s", "unary", "pw_jc", "pw_ir", "pw_pr", "tail"):
            a, b = got[k], want[k]
            assert a.shape == b.shape, k
            assert all(np.array_equal(a[n], b[n]) for n in a.dtype.names) if a.dtype.names else np.array_equal(a, b), k
    finally:
        ctx.close()
        dec.close()


# ------------------------------------------------ the host mirror and the program

def _cli_timing(out):
    lines = [ln for ln in out.splitlines() if ln.startswith("LM_TIMING ")]
    assert len(lines) == 1, out
    f = lines[0].split()[1:]
    return {k: float(v) for k, v in zip(f[::2], f[1::2])}


def _run_both(tmp_path, env, jpeg, n=40, config_overrides=None, damage=None):
    """The program on one MJPEG video with LM_DECODE=host and =device; returns
    the two YAML files' bytes and the device run's LM_TIMING fields."""
    import media_writers as MW
    from locomouse_cpp_amd import synthetic as S
    from test_cli import cli_args, run_cli
    cfg = S.SyntheticConfig()
    out = {}
    for mode in ("host", "device"):
        d = tmp_path / mode
        d.mkdir()
        paths = MW.write_inputs(str(d), cfg, n, stem="mouse_R", bits=24, jpeg=jpeg, config_overrides=config_overrides)
        if damage:
            damage(paths["video"], cfg)
        rc, text = run_cli(cli_args(paths, side="R", outdir=str(d)), env=dict(env, LM_DECODE=mode, LM_TIMING="1"))
        assert rc == 0, (mode, text)
        out[mode] = ((d / "output_mouse_R.yml").read_bytes(), _cli_timing(text))
    return out


@pytest.mark.parametrize("multi", [False, True], ids=["one_device", "four_device_threads"])
def test_cli_device_decode_writes_the_same_yaml(tmp_path, multi):
    from test_cli import MULTI_DEVICE_ENV
    env = dict(MULTI_DEVICE_ENV, LM_BATCH="16") if multi else {"LM_BATCH": "16"}
    out = _run_both(tmp_path, env, dict(mode="RGB", quality=92, subsampling=2))
    assert out["host"][0] == out["device"][0] and len(out["host"][0]) > 0
    t = out["device"][1]
    assert t["decode_fallback_frames"] == 0 and t["decode_device_ms"] > 0 and t["frames"] == 40 and t["batches"] == 3
    assert out["host"][1]["decode_device_ms"] == 0 and out["host"][1]["decode_fallback_frames"] == 0


def test_host_mirror_bounding_box_pass_on_device_frames():
    """use_provided_bounding_box = 0: the whole-video pass takes the decoded
    frames in device memory (lm_bb_push_device), then the frame loop runs on
    the computed boxes; corners, box sizes and candidate counts equal the
    host-decoded run's.  (Frames the pass finds a mouse box in: bb_scenes.)"""
    import media_writers as MW
    from bb_scenes import bb_frames
    from locomouse_cpp_amd import synthetic as S
    cfg = S.SyntheticConfig()
    cfg.params.use_provided_bounding_box = 0
    js = MW.jpeg_frames(bb_frames(cfg, 12, seed=4), mode="L", quality=95)
    bbp = abi.bb_params(semantics=abi.LM_BB_FIRSTLAST_INTEGER)
    host = JH.run_host_mirror(cfg, js, bbp, batch=5, device_decode=False)
    dev = JH.run_host_mirror(cfg, js, bbp, batch=5, device_decode=True)
    assert np.array_equal(host[0], dev[0]) and host[1] == dev[1] and np.array_equal(host[2], dev[2])
    assert host[2].sum() > 0 and dev[3] == 0 and host[3] == 0


def test_cli_frames_the_device_hands_back_come_from_the_host_decoder(tmp_path):
    """A video mixing in-scope frames with 16-bit-table frames and one whose
    scan is cut at 70 %: the device run falls back for those and still writes
    the host run's YAML."""
    import media_writers as MW

    def damage(video, cfg):
        f = cfg.frames(0, 40)
        js = MW.jpeg_frames(f, mode="L", quality=90)
        qt = [[257 + 27 * i for i in range(64)]]
        for i in (3, 17, 18):
            js[i] = MW.jpeg_frames(f[i:i + 1], mode="L", qtables=qt)[0]
        js[25] = JH.cut_scan(js[25], 0.7)
        MW.write_mjpeg_avi(video, js, cfg.cols, cfg.rows)

    out = _run_both(tmp_path, {"LM_BATCH": "16"}, dict(mode="L", quality=90), damage=damage)
    assert out["host"][0] == out["device"][0] and len(out["host"][0]) > 0
    assert out["device"][1]["decode_fallback_frames"] == 4


def test_cli_device_decode_refuses_other_videos(tmp_path):
    import media_writers as MW
    from locomouse_cpp_amd import synthetic as S
    from test_cli import cli_args, run_cli
    cfg = S.SyntheticConfig()
    paths = MW.write_inputs(str(tmp_path), cfg, 4, stem="mouse_R", bits=24)  # BI_RGB
    rc, text = run_cli(cli_args(paths, side="R", outdir=str(tmp_path)), env={"LM_DECODE": "device"})
    assert rc != 0 and "LM_DECODE=device needs an MJPEG video" in text, text
    rc, text = run_cli(cli_args(paths, side="R", outdir=str(tmp_path)), env={"LM_DECODE": "gpu"})
    assert rc != 0 and "LM_DECODE must be host or device" in text, text
