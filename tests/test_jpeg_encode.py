"""The JPEG encoder and the preview's other host parts, without a GPU: the host
encoder (host/JpegEncode.cpp) against Pillow byte for byte, the project's own
decoder on its files, the MJPEG AVI writer read back through AviReader, the
interface of include/locomouse_encode.h, its refusals, and a stand-alone
sanitizer run of the encoder."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import enc_harness as EH  # noqa: E402
import jpeg_harness as JH  # noqa: E402
import media_writers as MW  # noqa: E402

from locomouse_cpp_amd import abi, runtime  # noqa: E402

HDR = os.path.join(runtime.ROOT, "include", "locomouse_encode.h")
GROUPS = sorted({name.rsplit("_", 2)[0] for name, _, _ in EH.cases()})  # grey_8x8, rgb_33x49, ...


def _group(g):
    return [(c, p) for c, p in zip(EH.cases(), EH.pillow_files()) if c[0].rsplit("_", 2)[0] == g]


def test_case_list_covers_what_it_must():
    names = [c[0] for c in EH.cases()]
    for h, w in EH.GREY_SIZES:
        for img in ("noise", "const0", "const128", "const255", "checker", "gradient", "blocks"):
            for q in EH.QUALITIES:
                assert f"grey_{h}x{w}_{img}_q{q}" in names
        assert f"grey_{h}x{w}_spike_q5" in names
    for h, w in EH.COLOUR_SIZES:
        for img in ("noise", "const0", "const128", "const255", "checker", "gradient", "blocks", "marks"):
            for q in EH.QUALITIES:
                assert f"rgb_{h}x{w}_{img}_q{q}" in names
        assert f"rgb_{h}x{w}_spike_q5" in names
    assert EH.GREY_SIZES == ((8, 8), (16, 16), (17, 23), (24, 40), (8, 2048))
    assert EH.COLOUR_SIZES == ((8, 8), (9, 17), (16, 16), (17, 23), (24, 40), (33, 49))
    assert EH.QUALITIES == (1, 5, 25, 75, 90, 100)


@pytest.mark.parametrize("group", GROUPS)
def test_host_encoder_equals_pillow(group):
    for (name, img, q), ref in _group(group):
        got = EH.host_encode(img, q)
        assert isinstance(got, bytes), (name, got)
        assert got[:2] == b"\xff\xd8" and got[-2:] == b"\xff\xd9", name
        assert got == ref, f"{name}: {len(got)} bytes against Pillow's {len(ref)}"
        assert len(got) <= EH.slot_bytes(img.shape[0], img.shape[1], EH.fmt_of(img))


def _properties(img, j):
    """Which of the five hard things Pillow's file j of img holds, from the project's decoder's coefficients."""
    s, e = JH.scan_bounds(j)
    out = set()
    if b"\xff\x00" in j[s:e]:
        out.add("stuffed")
    if j.endswith(b"\xff\x00\xff\xd9"):
        out.add("stuffed_fill")
    zz = JH.host_coefficients(j, img.shape[0], img.shape[1]).astype(np.int32)[:, EH.ZIGZAG]
    ac = zz[:, 1:]
    if (np.abs(ac) >= 512).any():
        out.add("ac10")
    for row in ac != 0:
        idx = np.flatnonzero(row)
        if len(idx) and (np.diff(np.concatenate([[-1], idx])) - 1 >= 16).any():  # 16 zeros in front of a coefficient
            out.add("zrl")
            break
    if img.ndim == 2:  # one component: the DC differences run along the blocks
        if (np.abs(np.diff(np.concatenate([[0], zz[:, 0]]))) >= 1024).any():
            out.add("dc11")
    return out


def test_case_list_is_not_vacuous():
    seen = set()
    for (name, img, q), j in zip(EH.cases(), EH.pillow_files()):
        seen |= _properties(img, j)
    assert seen == {"stuffed", "stuffed_fill", "zrl", "dc11", "ac10"}, seen


def test_host_coefficients_are_what_the_decoder_reads_back():
    """The encoder's zig-zag coefficients (the device encoder's first stage) equal what the project's decoder finds in
    the file (natural order; it zeroes Cr, which channel 0 never needs)."""
    for name in ("grey_17x23_noise_q75", "grey_24x40_checker_q100", "rgb_17x23_noise_q90", "rgb_33x49_marks_q75"):
        _, img, q = next(c for c in EH.cases() if c[0] == name)
        mine = EH.host_coefficients(img, q)
        back = JH.host_coefficients(EH.host_encode(img, q), img.shape[0], img.shape[1])[:, EH.ZIGZAG]
        assert mine.shape == back.shape, name
        keep = np.ones(len(mine), bool)
        if img.ndim == 3:
            keep[5::6] = False
        assert np.array_equal(mine[keep], back[keep]), name


@pytest.mark.parametrize("group", GROUPS)
def test_project_decoder_on_the_encoders_files(group):
    for (name, img, q), _ in _group(group):
        j = EH.host_encode(img, q)
        got = JH.host_decode(j, img.shape[0], img.shape[1])
        assert not isinstance(got, str), (name, got)
        assert np.array_equal(got, MW.decode_jpeg_channel0(j)), name


def test_avi_writer_round_trips_through_avireader(tmp_path):
    rows, cols = 33, 49
    imgs = [EH.colour_images(rows, cols)[k] for k in ("noise", "marks", "const0", "gradient", "checker")]
    jpegs = [EH.host_encode(im, q) for im, q in zip(imgs, (90, 75, 100, 5, 100))]
    assert any(len(j) & 1 for j in jpegs) and any(not len(j) & 1 for j in jpegs)  # padded and unpadded chunks
    p = str(tmp_path / "w.avi")
    assert EH.write_avi(p, jpegs, rows, cols, fps=25) == 0
    assert EH.avi_info(p) == dict(rows=rows, cols=cols, frames=5, fps=25, mjpeg=True)
    assert EH.avi_chunks(p) == jpegs
    assert np.array_equal(EH.avi_frames(p), np.stack([MW.decode_jpeg_channel0(j) for j in jpegs]))
    data = open(p, "rb").read()
    assert data[:4] == b"RIFF" and int.from_bytes(data[4:8], "little") == len(data) - 8
    i = data.index(b"idx1")
    assert int.from_bytes(data[i + 4:i + 8], "little") == 16 * 5 and i + 8 + 16 * 5 == len(data)
    movi = data.index(b"movi")
    for k, j in enumerate(jpegs):  # the index names every chunk
        e = data[i + 8 + 16 * k:i + 24 + 16 * k]
        off, size = int.from_bytes(e[8:12], "little"), int.from_bytes(e[12:16], "little")
        assert e[:4] == b"00dc" and size == len(j) and data[movi + off:movi + off + 4] == b"00dc"
        assert data[movi + off + 8:movi + off + 8 + size] == j
    # a grey file and the reader of the uncompressed writer's rate
    g = [EH.host_encode(EH.grey_images(17, 23)["noise"], 90)]
    p2 = str(tmp_path / "g.avi")
    assert EH.write_avi(p2, g, 17, 23, fps=30) == 0 and EH.avi_chunks(p2) == g
    assert EH.write_avi(str(tmp_path / "none" / "w.avi"), g, 17, 23) == 1
    MW.write_avi(str(tmp_path / "raw.avi"), np.zeros((2, 4, 4), np.uint8), fps=50)
    assert EH.avi_info(str(tmp_path / "raw.avi"))["fps"] == 50


def declared_functions(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"^[A-Za-z_][\w\s\*]*?\b(lm_\w+)\s*\(", text, flags=re.M)))


def test_header_and_exports():
    assert set(declared_functions(HDR)) == set(runtime.ENC_EXPORTED)
    assert len(set(runtime.ENC_EXPORTED)) == len(runtime.ENC_EXPORTED)
    assert all(s.startswith("lm_enc_") for s in runtime.ENC_EXPORTED)
    L = runtime.lib()
    for sym in runtime.ENC_EXPORTED:
        assert getattr(L, sym) is not None
    for other in (runtime.EXPORTED, runtime.JPEG_EXPORTED, runtime.BKG_EXPORTED):
        assert not set(runtime.ENC_EXPORTED) & set(other)
    assert L.lm_abi_version() == 6
    assert "lm_jpeg_enc.hip" in runtime.HIP_UNITS
    text = open(HDR).read()
    for name in ("LM_ENC_GRAY8", "LM_ENC_RGB24", "LM_ENC_BLOCK_WORDS", "LM_ENC_MAX_HEADER", "LM_ENC_MAX_BATCH",
                 "LM_ENC_MAX_RADIUS"):
        m = re.search(rf"^#define {name} (\d+)\b", text, flags=re.M)
        assert m and int(m.group(1)) == getattr(abi, name), name
    assert re.search(r"^#define LM_ENC_MAX_BLOCKS \(1 << 20\)", text, flags=re.M) and abi.LM_ENC_MAX_BLOCKS == 1 << 20
    pal = re.search(r"LM_ENC_PALETTE\[LM_ENC_PALETTE_SIZE\]\[3\] = \{(.*?)\};", re.sub(r"/\*.*?\*/", "", text, flags=re.S), flags=re.S)
    rows = re.findall(r"\{(\d+), (\d+), (\d+)\}", pal.group(1))
    assert tuple(tuple(map(int, r)) for r in rows) == abi.LM_ENC_PALETTE and len(rows) == 8
    assert len(set(abi.LM_ENC_PALETTE)) == 8


@pytest.mark.parametrize("name", ["lm_enc_result", "lm_enc_stats", "lm_enc_mark", "lm_enc_overlay"])
def test_struct_layout_matches_the_header(tmp_path, name):
    fields = [f for f, _ in getattr(abi, name)._fields_]
    prints = "".join(f'printf(" %zu", offsetof({name}, {f}));' for f in fields)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "locomouse_encode.h"\n'
                   f'int main(void){{printf("%zu", sizeof({name}));{prints}}}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I" + os.path.join(runtime.ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    cls = getattr(abi, name)
    assert got == [C.sizeof(cls)] + [getattr(cls, f).offset for f in fields]


def test_slot_bytes_is_the_headers_formula():
    L = runtime.lib()
    for rows, cols in ((8, 8), (17, 23), (256, 1024), (1, 1), (65535, 1)):
        for fmt in (abi.LM_ENC_GRAY8, abi.LM_ENC_RGB24):
            assert L.lm_enc_slot_bytes(rows, cols, fmt) == EH.slot_bytes(rows, cols, fmt)
    for rows, cols, fmt in ((0, 8, 0), (8, 65536, 0), (8, 8, 2), (65535, 65535, 0)):
        assert L.lm_enc_slot_bytes(rows, cols, fmt) == -1


def test_null_and_bad_arguments_without_gpu():
    L = runtime.lib()
    INV = abi.LM_ERR_INVALID_ARGUMENT
    assert L.lm_enc_create(0, 8, 8, 0, 90, 4, None) == INV and b"out is NULL" in L.lm_last_error()
    h = C.c_void_p()
    for args, msg in (((0, 0, 8, 0, 90, 4), b"rows and cols"), ((0, 8, 65536, 0, 90, 4), b"rows and cols"),
                      ((0, 8, 8, 2, 90, 4), b"format"), ((0, 8, 8, -1, 90, 4), b"format"),
                      ((0, 8, 8, 0, 0, 4), b"quality"), ((0, 8, 8, 0, 101, 4), b"quality"),
                      ((0, 8, 8, 0, 90, 0), b"max_batch"), ((0, 8, 8, 0, 90, abi.LM_ENC_MAX_BATCH + 1), b"max_batch"),
                      ((0, 65535, 65535, 0, 90, 1), b"frame too large"), ((0, 4096, 4096, 1, 90, 64), b"2^31"),
                      ((-1, 8, 8, 0, 90, 4), b"device")):
        assert L.lm_enc_create(*args, C.byref(h)) == INV and not h.value, args
        assert msg in L.lm_last_error(), (args, L.lm_last_error())
    res = abi.lm_enc_result()
    buf = np.zeros(64, np.uint8)
    assert L.lm_enc_encode(None, buf.ctypes.data, 64, 1, C.byref(res)) == INV and b"null" in L.lm_last_error()
    assert L.lm_enc_encode_device(None, buf.ctypes.data, 64, 1, C.byref(res)) == INV
    assert L.lm_enc_set_overlay(None, None) == INV
    off = np.zeros(2, np.int32)
    assert L.lm_enc_render_encode_device(None, buf.ctypes.data, 64, 1, None, off.ctypes.data, C.byref(res)) == INV
    assert L.lm_enc_render_encode(None, buf.ctypes.data, 64, 1, None, off.ctypes.data, C.byref(res)) == INV
    assert L.lm_enc_render_device(None, buf.ctypes.data, 64, 1, None, off.ctypes.data, buf.ctypes.data) == INV
    assert L.lm_enc_last_stats(None, None) == INV
    assert L.lm_enc_stream(None) is None
    L.lm_enc_destroy(None)


def test_host_encoder_refuses_bad_arguments():
    img = np.zeros((8, 8), np.uint8)
    for q in (0, 101, -5):
        m = EH.host_encode(img, q)
        assert isinstance(m, str) and "quality" in m
    err = C.create_string_buffer(256)
    out = np.zeros(4096, np.uint8)
    assert EH.lib().eh_encode(img.ctypes.data, 0, 8, 0, 90, out.ctypes.data, out.size, err, 256) == -1
    assert b"rows and cols" in err.value
    assert EH.lib().eh_encode(None, 8, 8, 0, 90, out.ctypes.data, out.size, err, 256) == -1 and b"NULL" in err.value


@pytest.mark.parametrize("spec,msg", [
    (":90", "expected path.avi[:quality[:radius]], not :90."), ("p.avi:0", "quality must be in 1..100, not 0."),
    ("p.avi:101", "quality must be in 1..100, not 101."), ("dir:1/p.avi:0:3", "quality must be in 1..100, not 0."),
    ("p.avi:90:65", "radius must be in 0..64, not 65."), ("p.avi:", "expected path.avi[:quality[:radius]], not p.avi:."),
    ("p.avi:90:", "expected path.avi[:quality[:radius]], not p.avi:90:.")])
def test_cli_refuses_a_malformed_preview_value(tmp_path, spec, msg):
    """LM_PREVIEW other than path.avi[:quality[:radius]] stops the program before a device is touched (this test runs
    without one)."""
    from locomouse_cpp_amd import synthetic as S
    cfg = S.SyntheticConfig()
    paths = MW.write_inputs(str(tmp_path), cfg, 2)
    args = ["0", paths["config"], paths["video"], paths["background"], paths["model"], paths["calibration"], "R",
            str(tmp_path)]
    e = dict(os.environ)
    e["LM_PREVIEW"] = spec
    p = subprocess.run([runtime.CLI_PATH, *args], capture_output=True, text=True, env=e, timeout=120)
    assert p.returncode == 1, p.stdout
    assert "Invalid inputs: LM_PREVIEW: " + msg in p.stdout, p.stdout
    assert not os.path.exists(tmp_path / "output_synth_R.yml")


def test_encoder_is_clean_under_the_sanitizers(tmp_path):
    """A stand-alone program (tests/cpp/jpeg_encode_check.cpp) built with -fsanitize=address,undefined encodes 300
    random images and decodes them with the host decoder; nothing is loaded into Python."""
    exe = tmp_path / "jpeg_encode_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", *EH.INCLUDES, "-o", str(exe),
                           os.path.join(EH.HERE, "cpp", "jpeg_encode_check.cpp"),
                           os.path.join(EH.PKG, "host", "JpegEncode.cpp"), os.path.join(EH.PKG, "host", "Jpeg.cpp")])
    r = subprocess.run([str(exe), "300", "20261019"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "300 cases, 0 failures" in r.stdout, r.stdout
