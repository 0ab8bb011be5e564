"""ctypes access to tests/cpp/enc_rst_harness.cpp (the host JPEG encoder with
restart intervals), Pillow as its reference, and the cases the restart tests
share (CPU and GPU).  The harness links no GPU library."""
import ctypes as C
import functools
import io
import os
import re
import subprocess

import numpy as np

import enc_harness as EH

BUILD = EH.BUILD
SO = os.path.join(BUILD, "libenc_rst_harness.so")
SRC = os.path.join(EH.HERE, "cpp", "enc_rst_harness.cpp")
HOST_SRCS = [os.path.join(EH.PKG, "host", "JpegEncode.cpp")]


def _deps():
    return [SRC, *HOST_SRCS, os.path.join(EH.PKG, "host", "JpegEncode.hpp"),
            os.path.join(EH.PKG, "csrc", "lm_jpeg_enc_core.h"), os.path.join(EH.PKG, "csrc", "lm_jpeg_hdr.h")]


def build(verbose=False):
    os.makedirs(BUILD, exist_ok=True)
    cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", *EH.INCLUDES, "-o", SO, SRC, *HOST_SRCS]
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
        L.erh_encode.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_char_p,
                                 C.c_int]
        L.erh_encode.restype = C.c_int64
        _lib = L
    return _lib


def mcus(rows, cols, fmt):
    """(MCU rows, MCUs per row)."""
    m = 8 if fmt == EH.GRAY8 else 16
    return (rows + m - 1) // m, (cols + m - 1) // m


def intervals(rows, cols, fmt, ri):
    mh, mw = mcus(rows, cols, fmt)
    return (mh * mw + ri - 1) // ri


def slot_bytes(rows, cols, fmt, ri):
    """The worst case of one file (include/locomouse_encode.h: lm_enc_slot_bytes_restart)."""
    if ri == 0:
        return EH.slot_bytes(rows, cols, fmt)
    mh, mw = mcus(rows, cols, fmt)
    nblk = mh * mw * (1 if fmt == EH.GRAY8 else 6)
    ni = intervals(rows, cols, fmt, ri)
    return 640 + 2 * 4 * (52 * nblk + (ni + 3) // 4 + 1) + 2 * (ni - 1) + 2


def host_encode(img, quality, ri):
    """The host encoder's file for one image with a restart interval of ri MCUs, or its error message (str)."""
    img = np.ascontiguousarray(img, np.uint8)
    fmt = EH.fmt_of(img)
    out = np.zeros(slot_bytes(img.shape[0], img.shape[1], fmt, min(max(ri, 0), 65535)), np.uint8)
    err = C.create_string_buffer(256)
    n = lib().erh_encode(img.ctypes.data, img.shape[0], img.shape[1], fmt, quality, ri, out.ctypes.data, out.size, err, 256)
    if n == -1:
        return err.value.decode()
    assert n >= 0, "the file passed its worst case"
    return out[:n].tobytes()


def pillow_encode(img, quality, ri):
    """Pillow's file with restart_marker_blocks=ri (libjpeg's restart_interval, in MCUs)."""
    from PIL import Image
    b = io.BytesIO()
    if img.ndim == 2:
        Image.fromarray(np.ascontiguousarray(img, np.uint8), "L").save(b, "JPEG", quality=quality, restart_marker_blocks=ri)
    else:
        Image.fromarray(np.ascontiguousarray(img, np.uint8), "RGB").save(b, "JPEG", quality=quality, subsampling=2,
                                                                        restart_marker_blocks=ri)
    return b.getvalue()


def markers(j):
    """The restart markers of file j's scan, in order (0..7 each).  In entropy-coded data FF is followed by 00 (a
    stuffed byte) or by a marker's second byte, so FF D0..D7 there is a restart marker."""
    s = j.index(b"\xff\xda")
    s += 2 + int.from_bytes(j[s + 2:s + 4], "big")
    return [m[1] - 0xD0 for m in re.findall(rb"\xff[\xd0-\xd7]", j[s:-2])]


def dri(j):
    """The restart interval of file j's DRI segment, which must sit directly in front of SOS; None without one."""
    s = j.index(b"\xff\xda")
    if j[s - 6:s - 2] != b"\xff\xdd\x00\x04":
        assert b"\xff\xdd\x00\x04" not in j[:s]
        return None
    return int.from_bytes(j[s - 2:s], "big")


# ---- the cases: shape x image x quality x interval
SHAPES = (("grey", 17, 23), ("rgb", 37, 53))


def _image(tag, h, w, name):
    if name == "flat":
        return np.full((h, w) if tag == "grey" else (h, w, 3), 77, np.uint8)
    rng = np.random.default_rng(h * 1009 + w + (0 if tag == "grey" else 7))
    return rng.integers(0, 256, size=(h, w) if tag == "grey" else (h, w, 3)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def cases():
    """((name, image, quality, interval, markers expected), ...): per shape, quality-100 noise and a flat frame at
    intervals of 1 and 3 MCUs, one MCU row, the MCU count (no marker) and beyond it."""
    out = []
    for tag, h, w in SHAPES:
        fmt = EH.GRAY8 if tag == "grey" else EH.RGB24
        mh, mw = mcus(h, w, fmt)
        for name, q in (("noise", 100), ("noise", 75), ("flat", 100), ("flat", 90)):
            img = _image(tag, h, w, name)
            img.setflags(write=False)
            for ri in (1, 3, mw, mh * mw, mh * mw + 5, 65535):
                out.append((f"{tag}_{h}x{w}_{name}_q{q}_ri{ri}", img, q, ri, intervals(h, w, fmt, ri) - 1))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def pillow_files():
    """Pillow's file of every case, computed once."""
    return tuple(pillow_encode(img, q, ri) for _, img, q, ri, _ in cases())
