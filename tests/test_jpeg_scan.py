"""Device JPEG decode, the parts that run without a GPU: the shared scan code
(csrc/lm_jpeg_scan.h) run lane by lane on the CPU against the host decoder
(host/Jpeg.cpp, which test_mjpeg.py pins to libjpeg-turbo), lm_jpeg_probe, the
struct layouts of include/locomouse_jpeg.h, NULL-argument errors, and a
stand-alone sanitizer run over clean and damaged streams."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_harness as JH  # noqa: E402

from locomouse_cpp_amd import abi, runtime  # noqa: E402

STREAMS = JH.stream_list()
HDR = os.path.join(runtime.ROOT, "include", "locomouse_jpeg.h")
# minimum, odd sizes, default, and one subsequence for the whole scan (the sequential decode)
SUBSEQS = (JH.SUBSEQ_MIN, 5, 7, 13, JH.SUBSEQ_DEFAULT)
WHOLE = 1 << 20


@pytest.mark.parametrize("case", STREAMS, ids=[s[0] for s in STREAMS])
def test_subsequence_scan_reproduces_the_host_decoder(case):
    name, rows, cols, jpegs = case
    for j in jpegs:
        want = JH.host_decode(j, rows, cols)
        assert not isinstance(want, str), want
        host_coef = JH.host_coefficients(j, rows, cols)  # Decoder::decode_block's own output
        cls, px, coef, st, why = JH.lanes_decode(j, rows, cols, subseq=WHOLE)
        assert cls == 0 and st["subsequences"] == 1, (cls, why, st)
        assert np.array_equal(coef, host_coef), "one-subsequence decode differs from the host decoder's coefficients"
        assert np.array_equal(px, want), "one-subsequence decode differs from the host decoder's pixels"
        for s in SUBSEQS:
            for lanes in (JH.CHUNK, 3):  # 3 lanes per chunk: the chunk carry runs on every stream
                cls, px, coef, st, why = JH.lanes_decode(j, rows, cols, subseq=s, lanes=lanes)
                assert cls == 0 and st["err"] == 0, (s, lanes, cls, why, st)
                s0, s1 = JH.scan_bounds(j)
                assert st["subsequences"] == -(-(s1 - s0) // s)
                assert st["rounds"] <= st["subsequences"] and st["max_chunk_rounds"] <= lanes
                assert np.array_equal(coef, host_coef), f"coefficients differ from the host decoder's at subseq_bytes={s}, lanes={lanes}"
                bad = np.argwhere(px != want)
                assert bad.size == 0, f"{len(bad)} samples differ at subseq_bytes={s}, first {bad[:4].tolist()}"


def test_streams_cover_what_they_are_meant_to():
    by = {s[0]: s for s in STREAMS}
    for n in ("grey_q100", "colour_q100_range_limit"):  # byte stuffing occurs
        assert all(b"\xff\x00" in j[slice(*JH.scan_bounds(j))] for j in by[n][3])
    for n in ("restart_blocks1_RGB", "restart_blocks3_L", "restart_rows1_RGB"):
        assert all(b"\xff\xdd" in j and b"\xff\xd0" in j for j in by[n][3])
    assert all(b"\xff\xc4" not in j.split(b"\xff\xda")[0] for j in by["avi1_no_dht_RGB"][3])
    s0, s1 = JH.scan_bounds(by["flat"][3][0])
    assert s1 - s0 < JH.SUBSEQ_DEFAULT
    s0, s1 = JH.scan_bounds(by["long_scan"][3][0])
    assert s1 - s0 > 3 * JH.CHUNK * JH.SUBSEQ_DEFAULT
    # ZRL symbols (0xF0) are in use: the sequential decode sees coefficient 63 only
    _, _, coef, _, _ = JH.lanes_decode(by["zrl"][3][0], by["zrl"][1], by["zrl"][2], subseq=WHOLE)
    assert (coef[:, 63] != 0).all() and (coef[:, 1:63] == 0).all()


def test_probe_classifies_streams():
    for name, rows, cols, jpegs in STREAMS:
        for j in jpegs:
            p = runtime.jpeg_probe(j)
            assert p["status"] == abi.LM_JPEG_OK, (name, p)
            assert (p["rows"], p["cols"]) == (rows, cols)
            s0, s1 = JH.scan_bounds(j)
            assert p["scan_bytes"] == s1 - s0
            assert p["components"] == (1 if "_L" in name or "grey" in name or name in ("flat", "zrl", "long_scan") else 3)
    by = {s[0]: s for s in STREAMS}
    assert runtime.jpeg_probe(by["restart_blocks3_RGB"][3][0])["restart_interval"] == 3
    p = runtime.jpeg_probe(by["colour_s2_37x53"][3][0])
    assert (p["h_samp"], p["v_samp"]) == (2, 2)
    p = runtime.jpeg_probe(by["colour_s1_37x53"][3][0])
    assert (p["h_samp"], p["v_samp"]) == (2, 1)
    for rows, cols, j in JH.sixteen_bit_streams():
        p = runtime.jpeg_probe(j)
        assert p["status"] == abi.LM_JPEG_NEEDS_HOST and "16-bit" in p["reason"]
    rows, cols, j = JH.progressive_stream()
    p = runtime.jpeg_probe(j)
    assert p["status"] == abi.LM_JPEG_REJECTED
    assert p["reason"] == JH.host_decode(j, rows, cols)  # the host decoder's message
    p = runtime.jpeg_probe(b"\xff\xd8\xff\xd9")
    assert p["status"] == abi.LM_JPEG_REJECTED and p["reason"] == JH.host_decode(b"\xff\xd8\xff\xd9", 1, 1)
    assert runtime.jpeg_probe(b"nope")["reason"] == "not a JPEG image (no SOI)"
    # everything else the host decoder accepts: NEEDS_HOST with the reason
    from PIL import Image
    import io
    f = JH.frames(1, 16, 24, 1)[0]
    b = io.BytesIO()
    Image.fromarray(np.stack([f, f, f], axis=2), "RGB").save(b, "JPEG", keep_rgb=True)
    adobe = b.getvalue()
    assert b"Adobe" in adobe
    base = by["colour_s0_48x64"][3][0]
    cases = [(adobe, "RGB (Adobe) colour space"),
             (JH.as_three_scans(base), "more than one scan"),
             (JH.with_sos_order(base, (0, 2, 1)), "scan components out of order"),
             (JH.with_sampling(base, 0, 1, 2), "sampling factors out of scope"),   # 4:4:0
             (JH.with_sampling(base, 0, 4, 1), "sampling factors out of scope"),   # 4:1:1
             (JH.with_sampling(base, 1, 2, 1), "sampling factors out of scope"),   # chroma at 2x1
             (JH.with_sampling(base, 2, 1, 2), "sampling factors out of scope")]
    for stream, reason in cases:
        p = runtime.jpeg_probe(stream)
        assert (p["status"], p["reason"]) == (abi.LM_JPEG_NEEDS_HOST, reason), (reason, p)
        assert not isinstance(JH.host_decode(stream, p["rows"], p["cols"]), str)  # the host decoder does take it
    # every rejection of the shared parser carries the host decoder's message
    sof = JH._sof_at(base)
    sos = JH._sos_at(base)
    rejected = [base[:sof + 4] + b"\x0c" + base[sof + 5:],                       # 12-bit samples
                base[:sof + 9] + b"\x02" + base[sof + 10:],                      # two components
                base[:sos] + b"\xff\xd8" + base[sos:],                           # nested SOI
                base[:sos + 5] + b"\x09" + base[sos + 6:],                       # unknown component in SOS
                base[:sos + 6] + b"\x40" + base[sos + 7:],                       # table selector 4
                base[:sof] + base[sos:],                                          # scan before frame header
                base[:sof + 20],                                                  # no scan at all
                base[:sos + 3]]                                                   # truncated segment
    for stream in rejected:
        p = runtime.jpeg_probe(stream)
        want = JH.host_decode(stream, 48, 64)
        assert isinstance(want, str) and (p["status"], p["reason"]) == (abi.LM_JPEG_REJECTED, want), (p, want)


def test_damaged_scan_is_sent_to_the_host():
    name, rows, cols, jpegs = STREAMS[0]
    cut = JH.cut_scan(jpegs[0], 0.7)
    for s in (JH.SUBSEQ_MIN, JH.SUBSEQ_DEFAULT):
        cls, _, _, st, _ = JH.lanes_decode(cut, rows, cols, subseq=s)
        assert cls == 1 and st["err"] != 0 and st["rounds"] <= st["subsequences"]
    assert runtime.jpeg_probe(cut)["status"] == abi.LM_JPEG_OK  # the header is fine: only the scan tells


def test_missing_restart_markers_are_sent_to_the_host():
    """A DRI segment without RSTn in the scan, and a restart stream whose last
    marker is gone: the host decoder resynchronises at each interval, so the
    device must hand these back, never decode them as one continuous scan."""
    by = {s[0]: s for s in STREAMS}
    damaged = []
    for name in ("grey_q50", "colour_s2_37x53"):
        _, rows, cols, jpegs = by[name]
        damaged.append((rows, cols, JH.with_dri(jpegs[0], 3)))
    for name in ("restart_blocks3_L", "restart_rows1_RGB"):
        _, rows, cols, jpegs = by[name]
        damaged.append((rows, cols, JH.without_last_rst(jpegs[0])))
    for rows, cols, j in damaged:
        assert not isinstance(JH.host_decode(j, rows, cols), str)
        for s in (JH.SUBSEQ_MIN, 7, JH.SUBSEQ_DEFAULT, WHOLE):
            cls, _, _, st, _ = JH.lanes_decode(j, rows, cols, subseq=s)
            assert cls == 1 and st["err"] & 8, (s, cls, st)  # LMJ_E_RST


@pytest.mark.parametrize("name", ["lm_jpeg_info", "lm_jpeg_stats"])
def test_struct_layout_matches_header(tmp_path, name):
    src = tmp_path / "sz.c"
    src.write_text(f'#include <stdio.h>\n#include "locomouse_jpeg.h"\nint main(void){{printf("%zu", sizeof({name}));}}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I" + os.path.dirname(HDR), str(src), "-o", str(exe)])
    assert int(subprocess.check_output([str(exe)])) == C.sizeof(getattr(abi, name))


def test_header_constants_and_exports():
    text = open(HDR).read()
    for k in ("LM_JPEG_OK", "LM_JPEG_NEEDS_HOST", "LM_JPEG_REJECTED", "LM_JPEG_SUBSEQ_MIN", "LM_JPEG_SUBSEQ_DEFAULT",
              "LM_JPEG_CHUNK"):
        assert f"#define {k} {getattr(abi, k)} " in text
    assert (JH.SUBSEQ_MIN, JH.SUBSEQ_DEFAULT, JH.CHUNK) == (abi.LM_JPEG_SUBSEQ_MIN, abi.LM_JPEG_SUBSEQ_DEFAULT,
                                                           abi.LM_JPEG_CHUNK)
    L = runtime.lib()
    for sym in runtime.JPEG_EXPORTED:
        assert getattr(L, sym) is not None and f"{sym}(" in text
    assert L.lm_abi_version() == 6 and not set(runtime.JPEG_EXPORTED) & set(runtime.EXPORTED)


def test_null_arguments_without_gpu():
    L = runtime.lib()
    assert L.lm_jpeg_create(0, 8, 8, 4, 0, None) == abi.LM_ERR_INVALID_ARGUMENT
    assert b"out is NULL" in L.lm_last_error()
    h = C.c_void_p()
    assert L.lm_jpeg_create(0, 8, 8, 0, 0, C.byref(h)) == abi.LM_ERR_INVALID_ARGUMENT and not h.value
    assert L.lm_jpeg_create(0, 8, 8, 4, abi.LM_JPEG_SUBSEQ_MIN - 1, C.byref(h)) == abi.LM_ERR_INVALID_ARGUMENT
    assert L.lm_jpeg_create(0, 0, 8, 4, 0, C.byref(h)) == abi.LM_ERR_INVALID_ARGUMENT
    assert L.lm_jpeg_decode_device(None, None, None, 0, None, 0, None) == abi.LM_ERR_INVALID_ARGUMENT
    assert L.lm_jpeg_probe(None, 0, None) == abi.LM_ERR_INVALID_ARGUMENT
    assert L.lm_jpeg_debug_stats(None, None) == abi.LM_ERR_INVALID_ARGUMENT
    assert L.lm_jpeg_stream(None) is None
    L.lm_jpeg_destroy(None)


def test_scan_code_is_clean_under_the_sanitizers(tmp_path):
    """A stand-alone program (tests/cpp/jpeg_scan_fuzz.cpp) built with
    -fsanitize=address,undefined runs the stream list plus truncated and
    corrupted copies, and copies with restart markers missing, through the
    same host scan; nothing is loaded into Python."""
    exe = tmp_path / "jpeg_scan_fuzz"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",  # the runtimes in the program itself
                           *JH.INCLUDES, "-o", str(exe), os.path.join(JH.HERE, "cpp", "jpeg_scan_fuzz.cpp"),
                           os.path.join(JH.PKG, "host", "Jpeg.cpp")])
    files = []
    for name, rows, cols, jpegs in STREAMS:
        p = tmp_path / f"{name}.jpg"
        p.write_bytes(jpegs[0])
        files.append(str(p))
    r = subprocess.run([str(exe), "20261019", "24", *files], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    # 24 seeded copies of each stream, plus the constructed ones (a DRI without markers; a marker taken out)
    import re
    m = re.search(r"(\d+) streams, (\d+) damaged copies, 0 failures", r.stdout)
    assert m and int(m.group(1)) == len(files) and int(m.group(2)) >= 26 * len(files), r.stdout
