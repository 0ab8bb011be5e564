"""ctypes access to tests/cpp/jpeg_rst_harness.cpp (the device decoder's
interval path run lane by lane on the CPU, with its hand-over to the
subsequence path), and the restart streams, clean and damaged, that the
interval-path tests share (CPU and GPU).  The harness links no GPU library."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import jpeg_harness as JH
import media_writers as MW

SO = os.path.join(JH.BUILD, "libjpeg_rst_harness.so")
SRC = os.path.join(JH.HERE, "cpp", "jpeg_rst_harness.cpp")


def _deps():
    return [SRC, os.path.join(JH.PKG, "csrc", "lm_jpeg_scan.h"), os.path.join(JH.PKG, "csrc", "lm_jpeg_hdr.h")]


def build(verbose=False):
    os.makedirs(JH.BUILD, exist_ok=True)
    cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", *JH.INCLUDES, "-o", SO, SRC]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return SO


_lib = None


def lib():
    """The harness, built on first use (and again when a source is newer)."""
    global _lib
    if _lib is None:
        if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in _deps()):
            build()
        L = C.CDLL(SO)
        L.jrh_intervals_decode.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                           C.c_int64, C.c_void_p, C.c_char_p, C.c_int]
        L.jrh_intervals_decode.restype = C.c_int
        _lib = L
    return _lib


def intervals_decode(data, rows, cols, subseq=JH.SUBSEQ_DEFAULT, lanes=JH.CHUNK):
    """The interval path lane by lane on the CPU, handing over to the subsequence scheme as the device does:
    (class, pixels, coefficients, stats dict, reason)."""
    out = np.zeros((rows, cols), np.uint8)
    coef = np.zeros((3 * ((rows + 15) // 8 + 1) * ((cols + 15) // 8 + 1), 64), np.int16)
    st = np.zeros(6, np.uint32)
    err = C.create_string_buffer(256)
    cls = lib().jrh_intervals_decode(data, len(data), rows, cols, subseq, lanes, out.ctypes.data, coef.ctypes.data, coef.size,
                                     st.ctypes.data, err, 256)
    stats = dict(interval=int(st[0]), intervals=int(st[1]), handed_over=int(st[2]), err=int(st[3]), blocks=int(st[4]),
                 longest=int(st[5]))
    return cls, out, coef[:int(st[4])], stats, err.value.decode()


# ---- streams
@functools.lru_cache(maxsize=None)
def restart_streams():
    """[(name, rows, cols, jpeg, intervals)]: the harness's restart streams (intervals of 1 and 3 MCUs and of one MCU
    row; L and RGB at 4:4:4, 4:2:2 and 4:2:0; 45 x 70), and a 128 x 136 grey frame at one block per interval: 272
    intervals, more than four waves of lanes with a partial last one."""
    out = []
    f = JH.frames(1, 45, 70, 7)
    for mode, sub, mcu in (("L", 2, (8, 8)), ("RGB", 0, (8, 8)), ("RGB", 1, (8, 16)), ("RGB", 2, (16, 16))):
        mh, mw = (45 + mcu[0] - 1) // mcu[0], (70 + mcu[1] - 1) // mcu[1]
        for tag, kw, ri in (("blocks1", dict(restart_marker_blocks=1), 1), ("blocks3", dict(restart_marker_blocks=3), 3),
                            ("rows1", dict(restart_marker_rows=1), mw)):
            j = MW.jpeg_frames(f, mode=mode, quality=80, subsampling=sub, **kw)[0]
            out.append((f"{tag}_{mode}_s{sub}", 45, 70, j, (mh * mw + ri - 1) // ri))
    g = JH.frames(1, 128, 136, 272)
    out.append(("grey_272", 128, 136, MW.jpeg_frames(g, mode="L", quality=90, restart_marker_blocks=1)[0], 272))
    return tuple(out)


def marker_positions(j):
    """Offsets in j of the FF of every restart marker of the scan."""
    s, e = JH.scan_bounds(j)
    return [i for i in range(s, e - 1) if j[i] == 0xFF and 0xD0 <= j[i + 1] <= 0xD7]


def without_marker(j, k):
    p = marker_positions(j)[k]
    return j[:p] + j[p + 2:]


def with_markers_swapped(j, a, b):
    """Markers a and b exchange their numbers (the bytes between stay)."""
    p = marker_positions(j)
    d = bytearray(j)
    d[p[a] + 1], d[p[b] + 1] = j[p[b] + 1], j[p[a] + 1]
    assert d[p[a] + 1] != j[p[a] + 1]
    return bytes(d)


def with_intervals_swapped(j, k):
    """Intervals k and k + 1 (each with the marker behind it) exchange places: every marker stays where one belongs,
    the blocks do not."""
    p = marker_positions(j)
    a, b, c = p[k - 1] + 2 if k else JH.scan_bounds(j)[0], p[k] + 2, p[k + 1] + 2
    return j[:a] + j[b:c] + j[a:b] + j[c:]


@functools.lru_cache(maxsize=None)
def damaged_streams():
    """[(name, rows, cols, jpeg)]: a DRI segment without markers, the last marker missing, a middle one missing, two
    markers' numbers swapped, two intervals swapped, a truncated tail."""
    out = []
    plain = MW.jpeg_frames(JH.frames(1, 45, 70, 7), mode="L", quality=80)[0]
    out.append(("with_dri", 45, 70, JH.with_dri(plain, 3)))
    for name, rows, cols, j, ni in restart_streams():
        if name not in ("blocks1_L_s2", "blocks3_RGB_s2", "grey_272"):
            continue
        out.append((f"{name}_without_last", rows, cols, JH.without_last_rst(j)))
        out.append((f"{name}_without_middle", rows, cols, without_marker(j, (ni - 1) // 2)))
        out.append((f"{name}_numbers_swapped", rows, cols, with_markers_swapped(j, 1, 2)))
        out.append((f"{name}_intervals_swapped", rows, cols, with_intervals_swapped(j, 2)))
        out.append((f"{name}_truncated", rows, cols, JH.cut_scan(j, 0.8)))
    return tuple(out)
