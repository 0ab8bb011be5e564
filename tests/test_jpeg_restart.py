"""Restart intervals in the JPEG encoder, without a GPU: the host encoder
(host/JpegEncode.cpp, encode_jpeg's restart_interval) against Pillow's
restart_marker_blocks byte for byte, the project's decoder on its files, the
worst-case size of include/locomouse_encode.h, and the new entry points'
refusals."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import enc_harness as EH  # noqa: E402
import enc_rst_harness as RH  # noqa: E402
import jpeg_harness as JH  # noqa: E402
import media_writers as MW  # noqa: E402

from locomouse_cpp_amd import abi, runtime  # noqa: E402


def test_case_list_covers_what_it_must():
    names = {c[0]: c for c in RH.cases()}
    assert RH.SHAPES == (("grey", 17, 23), ("rgb", 37, 53))
    assert RH.mcus(17, 23, EH.GRAY8) == (3, 3) and RH.mcus(37, 53, EH.RGB24) == (3, 4)
    for tag, h, w, row, count in (("grey", 17, 23, 3, 9), ("rgb", 37, 53, 4, 12)):
        for img, q in (("noise", 100), ("flat", 100)):
            for ri, nm in ((1, count - 1), (3, (count + 2) // 3 - 1), (row, 2), (count, 0), (count + 5, 0)):
                assert names[f"{tag}_{h}x{w}_{img}_q{q}_ri{ri}"][4] == nm
    assert names["rgb_37x53_noise_q100_ri1"][4] == 11  # the numbering wraps past D7


def test_pillow_writes_the_markers_the_cases_expect():
    """A silent encode without restarts cannot pass: every reference file holds its DRI segment directly in front of
    SOS and exactly the expected markers, numbered 0..7 in turn; and a 1-bit fill that comes out as FF, stuffed, occurs
    in front of a marker."""
    stuffed_fill = 0
    for (name, img, q, ri, nm), ref in zip(RH.cases(), RH.pillow_files()):
        assert RH.dri(ref) == ri, name
        assert RH.markers(ref) == [m & 7 for m in range(nm)], name
        stuffed_fill += len(re.findall(rb"\xff\x00\xff[\xd0-\xd7]", ref))
    assert stuffed_fill > 0


def test_host_encoder_equals_pillow_with_restarts():
    for (name, img, q, ri, nm), ref in zip(RH.cases(), RH.pillow_files()):
        got = RH.host_encode(img, q, ri)
        assert isinstance(got, bytes), (name, got)
        assert got == ref, f"{name}: {len(got)} bytes against Pillow's {len(ref)}"
        assert len(got) <= RH.slot_bytes(img.shape[0], img.shape[1], EH.fmt_of(img), ri)


def test_interval_zero_is_the_plain_encoder():
    for tag, h, w in RH.SHAPES:
        img = RH._image(tag, h, w, "noise")
        assert RH.host_encode(img, 90, 0) == EH.host_encode(img, 90) == EH.pillow_encode(img, 90)


def test_project_decoder_on_the_restart_files():
    for name, img, q, ri, nm in RH.cases():
        j = RH.host_encode(img, q, ri)
        got = JH.host_decode(j, img.shape[0], img.shape[1])
        assert not isinstance(got, str), (name, got)
        assert np.array_equal(got, MW.decode_jpeg_channel0(j)), name


def test_host_encoder_refuses_a_bad_interval():
    img = np.zeros((8, 8), np.uint8)
    for ri in (-1, 65536):
        m = RH.host_encode(img, 90, ri)
        assert isinstance(m, str) and "restart_interval" in m


def test_slot_bytes_restart_is_the_headers_formula():
    L = runtime.lib()
    for rows, cols in ((8, 8), (17, 23), (37, 53), (256, 1024), (1, 1), (65535, 1)):
        for fmt in (abi.LM_ENC_GRAY8, abi.LM_ENC_RGB24):
            assert L.lm_enc_slot_bytes_restart(rows, cols, fmt, 0) == L.lm_enc_slot_bytes(rows, cols, fmt)
            for ri in (1, 2, 3, 8, 128, 65535):
                got = L.lm_enc_slot_bytes_restart(rows, cols, fmt, ri)
                assert got == RH.slot_bytes(rows, cols, fmt, ri), (rows, cols, fmt, ri)
                # the derivation: 1660 bits a block, 7 bits of fill an interval, in whole words; stuffing doubles it
                mh, mw = RH.mcus(rows, cols, fmt)
                nblk, ni = mh * mw * (1 if fmt == abi.LM_ENC_GRAY8 else 6), RH.intervals(rows, cols, fmt, ri)
                worst_bits = 1660 * nblk + 7 * ni
                assert got >= 629 + 2 * ((worst_bits + 7) // 8) + 2 * (ni - 1) + 2
            assert runtime.JpegEncoder.slot_bytes(rows, cols, fmt, 3) == RH.slot_bytes(rows, cols, fmt, 3)
    for rows, cols, fmt, ri in ((0, 8, 0, 1), (8, 65536, 0, 1), (8, 8, 2, 1), (65535, 65535, 0, 1), (8, 8, 0, -1), (8, 8, 0, 65536)):
        assert L.lm_enc_slot_bytes_restart(rows, cols, fmt, ri) == -1
    # one block per interval is what the plain bound does not cover
    assert L.lm_enc_slot_bytes_restart(256, 1024, 0, 1) > L.lm_enc_slot_bytes(256, 1024, 0)


def test_create_restart_refuses_bad_arguments_without_gpu():
    L = runtime.lib()
    INV = abi.LM_ERR_INVALID_ARGUMENT
    assert L.lm_enc_create_restart(0, 8, 8, 0, 90, 4, 1, None) == INV and b"out is NULL" in L.lm_last_error()
    h = C.c_void_p()
    for args, msg in (((0, 8, 8, 0, 90, 4, -1), b"restart_interval"), ((0, 8, 8, 0, 90, 4, 65536), b"restart_interval"),
                      ((0, 0, 8, 0, 90, 4, 1), b"rows and cols"), ((0, 8, 8, 2, 90, 4, 1), b"format"),
                      ((0, 8, 8, 0, 0, 4, 1), b"quality"), ((0, 8, 8, 0, 90, 0, 1), b"max_batch"),
                      ((0, 65535, 65535, 0, 90, 1, 1), b"frame too large"), ((0, 4096, 4096, 1, 90, 64, 1), b"2^31"),
                      ((-1, 8, 8, 0, 90, 4, 1), b"device")):
        assert L.lm_enc_create_restart(*args, C.byref(h)) == INV and not h.value, args
        assert msg in L.lm_last_error(), (args, L.lm_last_error())


def test_header_declares_the_new_entry_points():
    text = open(os.path.join(runtime.ROOT, "include", "locomouse_encode.h")).read()
    assert re.search(r"^lm_status lm_enc_create_restart\(", text, flags=re.M)
    assert re.search(r"^int64_t lm_enc_slot_bytes_restart\(", text, flags=re.M)
    assert {"lm_enc_create_restart", "lm_enc_slot_bytes_restart"} <= set(runtime.ENC_EXPORTED)
    assert runtime.lib().lm_abi_version() == 6


# ---- the decoder's interval path, lane by lane on the CPU (csrc/lm_jpeg_scan.h: lmj_scan_intervals_host)
import subprocess  # noqa: E402

import jpeg_rst_harness as JR  # noqa: E402

JPEG_HDR = os.path.join(runtime.ROOT, "include", "locomouse_jpeg.h")


def test_restart_stream_list_covers_what_it_must():
    names = {s[0]: s for s in JR.restart_streams()}
    for mode, sub in (("L", 2), ("RGB", 0), ("RGB", 1), ("RGB", 2)):
        for tag in ("blocks1", "blocks3", "rows1"):
            assert f"{tag}_{mode}_s{sub}" in names
    assert names["grey_272"][4] == 272 > 4 * 64 and 272 % 64 and 272 % JH.CHUNK
    for name, rows, cols, j, ni in JR.restart_streams():
        assert len(JR.marker_positions(j)) == ni - 1 and ni > 1, name
        assert runtime.jpeg_probe(j)["status"] == abi.LM_JPEG_OK, name


@pytest.mark.parametrize("name,rows,cols,j,ni", JR.restart_streams(), ids=[s[0] for s in JR.restart_streams()])
def test_interval_schedule_equals_the_host_decoder(name, rows, cols, j, ni):
    cls, px, coef, st, why = JR.intervals_decode(j, rows, cols)
    assert cls == 0, why
    assert st["interval"] == 1 and st["intervals"] == ni and st["handed_over"] == 0 and st["err"] == 0
    assert np.array_equal(px, JH.host_decode(j, rows, cols))
    assert np.array_equal(coef, JH.host_coefficients(j, rows, cols))
    p = JR.marker_positions(j)
    s, e = JH.scan_bounds(j)
    assert st["longest"] == max(b - a for a, b in zip([s] + [q + 2 for q in p], p + [e]))


def test_streams_without_restarts_take_the_subsequence_path():
    for name, rows, cols, jpegs in JH.stream_list():
        if name.startswith("restart_") or name == "dense_q100":
            continue
        cls, px, coef, st, why = JR.intervals_decode(jpegs[0], rows, cols)
        ref = JH.lanes_decode(jpegs[0], rows, cols)
        assert (cls, st["interval"], st["intervals"], st["handed_over"]) == (ref[0], 0, 0, 0), name
        assert np.array_equal(px, ref[1]) and np.array_equal(coef, ref[2]), name
    # an interval of at least the MCU count: a DRI segment, one interval, no lane
    img = RH._image("grey", 17, 23, "noise")
    j = RH.host_encode(img, 90, 9)
    cls, px, coef, st, why = JR.intervals_decode(j, 17, 23)
    assert (cls, st["interval"], st["intervals"], st["handed_over"]) == (0, 0, 0, 0)
    assert np.array_equal(px, JH.host_decode(j, 17, 23))


@pytest.mark.parametrize("name,rows,cols,j", JR.damaged_streams(), ids=[s[0] for s in JR.damaged_streams()])
def test_damaged_streams_equal_the_subsequence_path(name, rows, cols, j):
    """Class and pixels are lanes_decode's.  Markers whose numbers are swapped decode on both paths (neither reads the
    numbers); everything else here is handed over and ends as the subsequence path ends it."""
    cls, px, coef, st, why = JR.intervals_decode(j, rows, cols)
    ref_cls, ref_px, ref_coef, ref_st, _ = JH.lanes_decode(j, rows, cols)
    assert cls == ref_cls, (name, why)
    assert np.array_equal(px, ref_px) and np.array_equal(coef, ref_coef)
    assert st["err"] == ref_st["err"]
    if name.endswith("numbers_swapped"):
        assert (cls, st["interval"], st["handed_over"]) == (0, 1, 0)
    elif name.endswith("intervals_swapped"):  # whole MCUs that change places are a valid stream of another image
        assert (cls, st["interval"], st["handed_over"]) in ((0, 1, 0), (1, 0, 1))
    else:
        assert (cls, st["interval"], st["handed_over"]) == (1, 0, 1)
        assert isinstance(JH.host_decode(j, rows, cols), (str, np.ndarray))  # (the host decoder's answer is its own)


def test_interval_path_entry_points_without_gpu(tmp_path):
    L = runtime.lib()
    INV = abi.LM_ERR_INVALID_ARGUMENT
    assert L.lm_jpeg_set_interval_path(None, 1) == INV
    assert L.lm_jpeg_debug_interval_stats(None, None) == INV
    assert {"lm_jpeg_set_interval_path", "lm_jpeg_debug_interval_stats"} <= set(runtime.JPEG_EXPORTED)
    fields = [f for f, _ in abi.lm_jpeg_interval_stats._fields_]
    prints = "".join(f'printf(" %zu", offsetof(lm_jpeg_interval_stats, {f}));' for f in fields)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "locomouse_jpeg.h"\n'
                   f'int main(void){{printf("%zu", sizeof(lm_jpeg_interval_stats));{prints}}}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I" + os.path.dirname(JPEG_HDR), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    cls = abi.lm_jpeg_interval_stats
    assert got == [C.sizeof(cls)] + [getattr(cls, f).offset for f in fields]


def test_interval_schedule_is_clean_under_the_sanitizers(tmp_path):
    """A stand-alone program (tests/cpp/jpeg_rst_fuzz.cpp) built with -fsanitize=address,undefined runs the restart
    streams and seeded damaged copies through the interval schedule and its hand-over; nothing is loaded into
    Python."""
    exe = tmp_path / "jpeg_rst_fuzz"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", *JH.INCLUDES, "-o", str(exe),
                           os.path.join(JH.HERE, "cpp", "jpeg_rst_fuzz.cpp")])
    files = []
    for name, rows, cols, j, ni in JR.restart_streams():
        p = tmp_path / f"{name}.jpg"
        p.write_bytes(j)
        files.append(str(p))
    r = subprocess.run([str(exe), "20261020", "64", *files], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.search(r"(\d+) streams, (\d+) damaged copies, (\d+) finished by the interval path, (\d+) handed over, 0 failures",
                  r.stdout)
    assert m and int(m.group(1)) == len(files) and int(m.group(2)) == 64 * len(files), r.stdout
    assert int(m.group(3)) > len(files) and int(m.group(4)) > 8 * len(files), r.stdout


# ---- the transcode program's refusals (no device is touched: these run without one)
@pytest.mark.parametrize("spec,msg", [
    ("0", "quality must be in 1..100, not 0."), ("101:8", "quality must be in 1..100, not 101."),
    ("90:65536", "restart_mcus must be in 0..65535, not 65536."), ("90:-1", "restart_mcus must be in 0..65535, not -1."),
    ("90:", "expected quality[:restart_mcus], not 90:."), (":8", "expected quality[:restart_mcus], not :8."),
    ("90:8:1", "expected quality[:restart_mcus], not 90:8:1."), ("ninety", "expected quality[:restart_mcus], not ninety.")])
def test_transcode_refuses_a_malformed_argument(tmp_path, spec, msg):
    from locomouse_cpp_amd import synthetic as S
    cfg = S.SyntheticConfig()
    paths = MW.write_inputs(str(tmp_path), cfg, 2)
    out = tmp_path / "out.avi"
    p = subprocess.run([runtime.TRANSCODE_CLI_PATH, paths["video"], str(out), spec], capture_output=True, text=True, timeout=120)
    assert p.returncode == 1, p.stdout
    assert "Invalid inputs: " + msg in p.stdout, p.stdout
    assert not out.exists()


def test_transcode_usage_and_missing_video(tmp_path):
    p = subprocess.run([runtime.TRANSCODE_CLI_PATH, "in.avi"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 1 and "Usage: LocoMouseTranscode in.avi out.avi [quality[:restart_mcus]]" in p.stdout
    p = subprocess.run([runtime.TRANSCODE_CLI_PATH, str(tmp_path / "none.avi"), str(tmp_path / "out.avi")],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 1 and "Invalid inputs: Could not open the video file" in p.stdout
    assert not (tmp_path / "out.avi").exists()
