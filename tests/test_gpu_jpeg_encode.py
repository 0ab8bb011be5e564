"""The device JPEG encoder and the track overlay (include/locomouse_encode.h,
csrc/lm_jpeg_enc.hip): every file is compared byte for byte with the host
encoder's and with Pillow's, the overlay exactly with a numpy restatement, and
the program's preview video with Pillow's encoding of the numpy canvases."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import enc_harness as EH  # noqa: E402
import jpeg_harness as JH  # noqa: E402
import media_writers as MW  # noqa: E402

from locomouse_cpp_amd import abi, runtime  # noqa: E402
from locomouse_cpp_amd import synthetic as S  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [("grey", h, w) for h, w in EH.GREY_SIZES] + [("rgb", h, w) for h, w in EH.COLOUR_SIZES]


def _fmt(tag):
    return abi.LM_ENC_GRAY8 if tag == "grey" else abi.LM_ENC_RGB24


@pytest.mark.parametrize("tag,h,w", SIZES, ids=[f"{t}_{h}x{w}" for t, h, w in SIZES])
def test_device_equals_host_and_pillow(tag, h, w):
    """Every image of the CPU test's case list, one batch per quality."""
    pillow = dict(zip((c[0] for c in EH.cases()), EH.pillow_files()))
    for q in EH.QUALITIES:
        group = [(n, img) for n, img, qq in EH.cases() if qq == q and n.startswith(f"{tag}_{h}x{w}_")]
        assert len(group) >= 7
        enc = runtime.JpegEncoder(h, w, _fmt(tag), quality=q, max_batch=len(group))
        files = enc.encode(np.stack([img for _, img in group]))
        for (name, img), got in zip(group, files):
            assert got == EH.host_encode(img, q), name
            assert got == pillow[name], name
        st = enc.stats()
        assert st["frames"] == len(group) and st["bytes_out"] == sum(map(len, files)) and st["device_ms"] > 0
        enc.close()


@pytest.mark.parametrize("tag", ["grey", "rgb"])
def test_blocks_outnumber_one_workgroups_scan(tag):
    """256 x 1024, n = 2: 4096 (6144) blocks per frame, 16 (24) rounds of the 256-wide scans, and the frames in
    device memory with a pitch wider than a frame."""
    import torch
    h, w, n = 256, 1024, 2
    rng = np.random.default_rng(2561024)
    y, x = np.mgrid[0:h, 0:w]
    base = (128 + 100 * np.sin(x / 17.0) * np.cos(y / 11.0)).astype(np.uint8)
    frames = np.stack([base, rng.integers(0, 256, size=(h, w)).astype(np.uint8)])
    if tag == "rgb":
        frames = np.stack([frames, frames[::-1], 255 - frames], axis=3)
    frames = np.ascontiguousarray(frames)
    fb = frames[0].size
    pitch = fb + 192
    buf = np.zeros(n * pitch, np.uint8)
    for i in range(n):
        buf[i * pitch:i * pitch + fb] = frames[i].reshape(-1)
    d = torch.from_numpy(buf).cuda()
    torch.cuda.synchronize()
    enc = runtime.JpegEncoder(h, w, _fmt(tag), quality=90, max_batch=n)
    files = enc.encode_device(d.data_ptr(), n, pitch=pitch)
    for i in range(n):
        assert files[i] == EH.host_encode(frames[i], 90), i
        assert files[i] == EH.pillow_encode(frames[i], 90), i
    assert files == enc.encode(frames)  # the host-pointer variant
    enc.close()


@pytest.mark.parametrize("tag", ["grey", "rgb"])
def test_reuse_and_batching(tag):
    h, w = 24, 40
    make = EH.grey_images if tag == "grey" else EH.colour_images
    imgs = make(h, w)
    order = ["noise", "const0", "checker", "gradient", "blocks", "const255"]
    stack = np.stack([imgs[k] for k in order])
    want = [EH.host_encode(im, 100) for im in stack]
    enc = runtime.JpegEncoder(h, w, _fmt(tag), quality=100, max_batch=3)
    assert enc.encode(stack[0:1]) == want[0:1]  # batches of 1, 3 and 2 on one context
    assert enc.encode(stack[1:4]) == want[1:4]
    assert enc.encode(stack[4:6]) == want[4:6]
    # a constant frame (a few bytes of scan) next to quality-100 noise: the per-frame offsets
    mixed = enc.encode(stack[[1, 0, 5]])
    assert mixed == [want[1], want[0], want[5]]
    assert len(want[1]) < len(want[0]) // 4
    # alone, in a batch, at another max_batch, after other calls: the same bytes
    other = runtime.JpegEncoder(h, w, _fmt(tag), quality=100, max_batch=6)
    assert other.encode(stack) == want
    assert other.encode(stack[0:1]) == enc.encode(stack[0:1]) == want[0:1]
    with pytest.raises(runtime.LMError) as e:
        enc.encode(stack[0:4])  # more than max_batch
    assert e.value.code == abi.LM_ERR_INVALID_ARGUMENT
    assert enc.encode(stack[3:4]) == want[3:4]  # and the context still works
    enc.close()
    other.close()


def numpy_canvas(raw, cal, flip, marks):
    """include/locomouse_encode.h's overlay, restated."""
    m = cal[:, ::-1] if flip else cal
    g = raw.reshape(-1)[m]
    out = np.repeat(g[:, :, None], 3, axis=2)
    rows, cols = cal.shape
    for x, y, r, c in marks:
        y0, y1, x0, x1 = max(y - r, 0), min(y + r + 1, rows), max(x - r, 0), min(x + r + 1, cols)
        if y0 < y1 and x0 < x1:
            out[y0:y1, x0:x1] = abi.LM_ENC_PALETTE[c]
    return out


def _overlay_case(rows, cols, flip, identity):
    rng = np.random.default_rng(rows * 131 + cols + flip)
    if identity:
        src_rows, src_cols = rows, cols
        cal = np.arange(rows * cols, dtype=np.int32).reshape(rows, cols)
    else:  # a warp into a larger raw frame: a shift, a shear, and a column of repeats
        src_rows, src_cols = rows + 5, cols + 9
        r, c = np.mgrid[0:rows, 0:cols]
        cal = ((r + 2 + (c // 16) % 2) * src_cols + np.minimum(c + 3, src_cols - 1)).astype(np.int32)
        cal[:, 0] = cal[:, 1]
    n = 3
    raw = rng.integers(0, 256, size=(n, src_rows, src_cols)).astype(np.uint8)
    marks = [
        # clipped at the four borders and the corners, radius 0, off the canvas altogether
        [(0, 0, 3, 0), (cols - 1, rows - 1, 3, 1), (cols // 2, 0, 2, 2), (0, rows // 2, 2, 3), (cols - 1, rows // 2, 4, 4),
         (cols // 2, rows - 1, 4, 5), (5, 5, 0, 6), (-40, 3, 3, 7), (3, rows + 40, 3, 7), (-2, -2, 3, 6)],
        # overlapping: the later one wins where they meet
        [(8, 8, 3, 0), (10, 9, 3, 1), (9, 10, 1, 2), (8, 8, 0, 7), (cols - 3, 6, 5, 3), (cols - 5, 8, 5, 4)],
        [],  # a frame with no marks
    ]
    return raw, cal, src_rows, src_cols, marks


@pytest.mark.parametrize("rows,cols", [(17, 23), (64, 96)])
@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("identity", [True, False], ids=["identity", "warp"])
def test_overlay_equals_numpy_and_encodes(rows, cols, flip, identity):
    import torch
    raw, cal, src_rows, src_cols, marks = _overlay_case(rows, cols, flip, identity)
    n = raw.shape[0]
    d = torch.from_numpy(raw).cuda()
    torch.cuda.synchronize()
    enc = runtime.JpegEncoder(rows, cols, abi.LM_ENC_RGB24, quality=90, max_batch=n)
    with pytest.raises(runtime.LMError):  # no geometry yet
        enc.render_device(d.data_ptr(), src_rows * src_cols, marks)
    enc.set_overlay(cal, src_rows, src_cols, flip)
    want = np.stack([numpy_canvas(raw[i], cal, flip, marks[i]) for i in range(n)])
    got = enc.render_device(d.data_ptr(), src_rows * src_cols, marks)
    assert np.array_equal(got, want)
    assert (want[0] != np.repeat(want[0][:, :, :1], 3, axis=2)).any()  # some mark is coloured
    files = enc.render_encode_device(d.data_ptr(), src_rows * src_cols, marks)
    assert files == [EH.pillow_encode(want[i], 90) for i in range(n)]
    assert files == [EH.host_encode(want[i], 90) for i in range(n)]
    assert files == enc.render_encode(raw, marks)  # the host-pointer variant
    # a smaller batch, the frames in another order
    files = enc.render_encode_device(d[2:].data_ptr(), src_rows * src_cols, [marks[1]])
    assert files == [EH.pillow_encode(numpy_canvas(raw[2], cal, flip, marks[1]), 90)]
    enc.close()


def test_overlay_refusals():
    import torch
    rows, cols = 17, 23
    raw, cal, src_rows, src_cols, _ = _overlay_case(rows, cols, 0, True)
    d = torch.from_numpy(raw).cuda()
    torch.cuda.synchronize()
    grey = runtime.JpegEncoder(rows, cols, abi.LM_ENC_GRAY8, max_batch=2)
    with pytest.raises(runtime.LMError) as e:
        grey.set_overlay(cal, src_rows, src_cols, 0)
    assert e.value.code == abi.LM_ERR_INVALID_ARGUMENT and "RGB24" in str(e.value)
    grey.close()
    enc = runtime.JpegEncoder(rows, cols, abi.LM_ENC_RGB24, max_batch=2)
    bad = cal.copy()
    bad[3, 4] = src_rows * src_cols
    for c, sr, sc in ((bad, src_rows, src_cols), (cal[:, :-1], src_rows, src_cols), (-cal - 1, src_rows, src_cols)):
        with pytest.raises(runtime.LMError) as e:
            enc.set_overlay(c, sr, sc, 0)
        assert e.value.code == abi.LM_ERR_INVALID_ARGUMENT
    enc.set_overlay(cal, src_rows, src_cols, 0)
    for mark in ((1, 1, -1, 0), (1, 1, abi.LM_ENC_MAX_RADIUS + 1, 0), (1, 1, 1, 8), (1, 1, 1, -1), (1 << 20, 1, 1, 0)):
        with pytest.raises(runtime.LMError) as e:
            enc.render_device(d.data_ptr(), src_rows * src_cols, [[mark]])
        assert e.value.code == abi.LM_ERR_INVALID_ARGUMENT, mark
    with pytest.raises(runtime.LMError):
        enc.render_device(d.data_ptr(), src_rows * src_cols - 1, [[]])  # pitch below a raw frame
    assert np.array_equal(enc.render_device(d.data_ptr(), src_rows * src_cols, [[]])[0], numpy_canvas(raw[0], cal, 0, []))
    enc.close()


def test_device_decoder_takes_the_encoders_files():
    """JpegDecoder on the device encoder's grey and 4:2:0 files: LM_JPEG_OK, and the host decoder's pixels."""
    for tag, h, w in (("grey", 24, 40), ("rgb", 33, 49), ("grey", 17, 23), ("rgb", 17, 23)):
        imgs = (EH.grey_images if tag == "grey" else EH.colour_images)(h, w)
        stack = np.stack([imgs[k] for k in ("noise", "gradient", "checker", "blocks")])
        for q in (25, 90, 100):
            enc = runtime.JpegEncoder(h, w, _fmt(tag), quality=q, max_batch=4)
            files = enc.encode(stack)
            enc.close()
            for j in files:
                assert runtime.jpeg_probe(j)["status"] == abi.LM_JPEG_OK
            dec = runtime.JpegDecoder(h, w, max_batch=4)
            out, status = dec.decode(files)
            assert (status == abi.LM_JPEG_OK).all(), (tag, h, w, q, status)
            got = out.cpu().numpy()
            dec.close()
            for i, j in enumerate(files):
                assert np.array_equal(got[i], JH.host_decode(j, h, w)), (tag, h, w, q, i)


# ---- the program end to end, on a 12-frame synthetic MJPEG video

N_VIDEO = 12


def _run(cmd, env=None, timeout=300):
    e = dict(os.environ)
    e.update(env or {})
    p = subprocess.run(cmd, capture_output=True, text=True, env=e, timeout=timeout)
    return p.returncode, p.stdout


def _matrix(path, key):
    """An integer matrix of the program's output file (tests/cpp/host_harness.cpp's FileStorage reader)."""
    import ctypes as C

    import host_harness as H
    kind, rows, cols, dt = C.c_int(), C.c_int(), C.c_int(), C.c_char()
    out = np.zeros(1 << 16)
    text = C.create_string_buffer(256)
    rc = H.lib().lmh_fs_node(os.fsencode(path), key.encode(), C.byref(kind), C.byref(rows), C.byref(cols), C.byref(dt),
                             out.ctypes.data, out.size, text, 256)
    assert rc == 0 and kind.value == 6, (key, rc, text.value)
    return out[:rows.value * cols.value].reshape(rows.value, cols.value).astype(np.int32)


def _marks_from_output(yml, n, radius):
    """Preview.hpp's preview_marks, restated from the exported file: the tail (colour 5, radius 1), the paws
    (colours 0..3), the snout (colour 4); bottom view then side view; -1 draws nothing."""
    paws = [_matrix(yml, f"paw_tracks{i}") for i in range(4)]
    snout = _matrix(yml, "snout_tracks0")
    tail = _matrix(yml, "tracks_tail")
    per = []
    for f in range(n):
        m = []
        for t in range(15):
            x, y, z = tail[:, 15 * f + t]
            m += [(x, v, 1, 5) for v in (y, z) if x >= 0 and v >= 0]
        for colour, M in ((0, paws[0]), (1, paws[1]), (2, paws[2]), (3, paws[3]), (4, snout)):
            x, y, z = M[f]
            m += [(x, v, radius, colour) for v in (y, z) if x >= 0 and v >= 0]
        per.append(m)
    return per


def _marks_sit_on_the_scene(jpeg, f, flip, marks, radius):
    """Independent of numpy_canvas: (a) the exported coordinates, read as zero-based columns and rows, lie on the
    synthetic scene's features (lm_synth.h; mirrored when the image is flipped), and (b) in the preview frame as
    Pillow decodes it, the colour sits on the pixel the coordinate names.
      (a) Each paw's bottom-view coordinate lies on one of the four paw discs (radius 6 about
          (cx + dx_k + tri(f + 5 k, 20, 30), 176 -+ 58)), a different disc each: a detection anywhere on a disc is a
          detection of that paw, so the radius is the bound.  Unflipped only (flipped, the tail lies outside the
          tail box and the snout track takes the tail's end): the snout's lies on its disc (radius 5 about
          (cx + 158, 176) and (cx + 158, 48)); the tail line is three rows thick about rows 176 and 48 and the tail
          points are on its centre row, so their rows are exactly 176 and 48 (a base of one would give 177 and 49),
          and their columns lie in cx - 330 .. cx - 150.
      (b) Around each paw's bottom-view coordinate (the marks are 40 columns apart there) the centroid of the
          colourfulness (largest minus smallest channel; the scene is grey) is within half a pixel of the
          coordinate.  The mark is symmetric about it; 4:2:0 chroma sits on a grid of two pixels, so one edge of the
          mark can keep up to half a pixel's weight more than the other: a shift of at most 0.5 (r + 1) / (2 r + 1),
          0.3 pixels, where a base off by one would give a whole pixel.  The pixel a tail point names is cyan
          (a mark three pixels wide keeps at least half its chroma there), and the pixels four rows above and below
          it (three beyond the mark's edge, past the smear of a chroma sample and its interpolation) are grey."""
    import io

    from PIL import Image
    rgb = np.asarray(Image.open(io.BytesIO(jpeg)).convert("RGB")).astype(np.int32)
    cols = rgb.shape[1]
    cx = 500 + S.tri(f, 50, 40)
    sat = rgb.max(axis=2) - rgb.min(axis=2)
    centres = [(cx + (-110, -40, 40, 110)[k] + S.tri(f + 5 * k, 20, 30), 176 + (58 if k & 1 else -58)) for k in range(4)]
    if flip:
        centres = [(cols - 1 - x, y) for x, y in centres]
    taken = set()
    paws = [(x, y) for x, y, _, c in marks if c < 4 and y >= 96]
    assert len(paws) == 4
    for x, y in paws:
        near = [i for i, (px, py) in enumerate(centres) if (x - px) ** 2 + (y - py) ** 2 <= 36]
        assert len(near) == 1 and near[0] not in taken, (f, x, y, centres)
        taken.add(near[0])
        w = radius + 4
        win = sat[y - w:y + w + 1, x - w:x + w + 1].astype(np.float64)
        win[win < 60] = 0
        assert win.sum() > 0
        gy, gx = np.mgrid[-w:w + 1, -w:w + 1]
        assert abs((win * gx).sum() / win.sum()) <= 0.5 and abs((win * gy).sum() / win.sum()) <= 0.5, (f, x, y)
    if flip:
        return
    snout = [(x, y) for x, y, _, c in marks if c == 4]
    assert len(snout) == 2
    for x, y in snout:
        assert (x - (cx + 158)) ** 2 + (y - (176 if y >= 96 else 48)) ** 2 <= 25, (f, x, y)
    tail = [(x, y) for x, y, _, c in marks if c == 5]
    assert len(tail) == 30

    for x, y in tail:
        assert y in (176, 48) and cx - 330 <= x <= cx - 150, (f, x, y)
        px = rgb[y, x]
        assert px[1] - px[0] >= 60 and px[2] - px[0] >= 60, (f, x, y, px.tolist())  # cyan: green and blue over red
        assert sat[y - 4, x] < 60 and sat[y + 4, x] < 60, (f, x, y, sat[y - 4:y + 5, x].tolist())


def test_program_preview_of_a_flipped_video(tmp_path):
    """Side "L": setup.flip reaches the overlay through write_preview, and the marks sit on the mirrored scene."""
    cfg = S.SyntheticConfig(flip=True)
    n = 4
    paths = MW.write_inputs(str(tmp_path), cfg, n, stem="mouse_L", bits=8)
    avi = str(tmp_path / "preview.avi")
    rc, text = _run([runtime.CLI_PATH, "0", paths["config"], paths["video"], paths["background"], paths["model"],
                     paths["calibration"], "L", str(tmp_path)], env={"LM_PREVIEW": avi + ":95"})
    assert rc == 0, text
    marks = _marks_from_output(str(tmp_path / "output_mouse_L.yml"), n, 3)
    assert {c for m in marks for _, _, _, c in m} >= {0, 1, 2, 3, 4}  # (mirrored, the tail is outside its box)
    chunks = EH.avi_chunks(avi)
    assert len(chunks) == n
    frames = cfg.frames(0, n)
    for f in range(n):
        assert chunks[f] == EH.pillow_encode(numpy_canvas(frames[f], cfg.calib, 1, marks[f]), 95), f
        _marks_sit_on_the_scene(chunks[f], f, True, marks[f], 3)


def test_program_writes_the_preview_video(tmp_path):
    cfg = S.SyntheticConfig()
    paths = MW.write_inputs(str(tmp_path), cfg, N_VIDEO, stem="mouse_R", jpeg=dict(mode="RGB", quality=92, subsampling=2))
    frames = paths["decoded"]
    outs = {k: tmp_path / k for k in ("plain", "host", "device")}
    for d in outs.values():
        d.mkdir()

    def args(outdir):
        return ["0", paths["config"], paths["video"], paths["background"], paths["model"], paths["calibration"], "R",
                str(outdir)]

    rc, text = _run([runtime.CLI_PATH, *args(outs["plain"])], env={"LM_BATCH": "5", "LM_PREVIEW": ""})  # empty: off
    assert rc == 0, text
    assert os.listdir(outs["plain"]) == ["output_mouse_R.yml"]
    plain = (outs["plain"] / "output_mouse_R.yml").read_bytes()
    assert len(plain) > 1000
    cal = cfg.calib
    for mode, spec, quality, radius in (("host", "{}", 90, 3), ("device", "{}:75:2", 75, 2)):
        avi = str(outs[mode] / "preview.avi")
        rc, text = _run([runtime.CLI_PATH, *args(outs[mode])],
                        env={"LM_BATCH": "5", "LM_DECODE": mode, "LM_PREVIEW": spec.format(avi), "LM_TIMING": "1"})
        assert rc == 0, text
        yml = str(outs[mode] / "output_mouse_R.yml")
        assert open(yml, "rb").read() == plain  # the results do not know about the preview
        timing = [ln for ln in text.splitlines() if ln.startswith("LM_TIMING ")][0].split()
        assert float(timing[timing.index("preview_ms") + 1]) > 0
        assert EH.avi_info(avi) == dict(rows=cfg.setup.calib_rows, cols=cfg.setup.calib_cols, frames=N_VIDEO, fps=30,
                                        mjpeg=True)
        marks = _marks_from_output(yml, N_VIDEO, radius)
        assert sum(len(m) for m in marks) >= 20 * N_VIDEO  # the tracks are there to be drawn
        assert {c for m in marks for _, _, _, c in m} == {0, 1, 2, 3, 4, 5}
        chunks = EH.avi_chunks(avi)
        for f in range(N_VIDEO):
            canvas = numpy_canvas(frames[f], cal, 0, marks[f])
            assert chunks[f] == EH.pillow_encode(canvas, quality), (mode, f)
            _marks_sit_on_the_scene(chunks[f], f, False, marks[f], radius)
    rc, text = _run([runtime.CLI_PATH, *args(outs["plain"])], env={"LM_PREVIEW": str(tmp_path / "p.avi") + ":0"})
    assert rc == 1 and "Invalid inputs: LM_PREVIEW: quality must be in 1..100, not 0." in text, text


def test_program_keeps_the_sources_frame_rate(tmp_path):
    cfg = S.SyntheticConfig()
    paths = MW.write_inputs(str(tmp_path), cfg, 3, stem="mouse_R")
    MW.write_avi(paths["video"], cfg.frames(0, 3), fps=50)
    avi = str(tmp_path / "preview.avi")
    rc, text = _run([runtime.CLI_PATH, "0", paths["config"], paths["video"], paths["background"], paths["model"],
                     paths["calibration"], "R", str(tmp_path)], env={"LM_PREVIEW": avi})
    assert rc == 0, text
    info = EH.avi_info(avi)
    assert info["fps"] == 50 and info["frames"] == 3
    # an uncompressed source: the canvas is the frame itself, exactly
    marks = _marks_from_output(str(tmp_path / "output_mouse_R.yml"), 3, 3)
    chunks = EH.avi_chunks(avi)
    for f in range(3):
        assert chunks[f] == EH.pillow_encode(numpy_canvas(cfg.frames(f, 1)[0], cfg.calib, 0, marks[f]), 90), f
