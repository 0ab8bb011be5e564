"""ctypes access to tests/cpp/bkg_harness.cpp (the host statement of
csrc/lm_bkg_core.h and host/Media.cpp's PNG writer and reader; no GPU library),
and the frame stacks the background tests share."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "locomouse_cpp_amd")
BUILD = os.path.join(HERE, "cpp", "_build")
SO = os.path.join(BUILD, "libbkg_harness.so")
SRC = os.path.join(HERE, "cpp", "bkg_harness.cpp")
CHECK_SRC = os.path.join(HERE, "cpp", "bkg_core_check.cpp")
INCLUDES = ["-I" + os.path.join(PKG, "host"), "-I" + os.path.join(PKG, "csrc"), "-I" + os.path.join(ROOT, "include")]
HOST_SRCS = [os.path.join(PKG, "host", f) for f in ("Media.cpp", "Jpeg.cpp")]

PERMILLES = (0, 250, 500, 999, 1000)


def _deps():
    return [SRC, *HOST_SRCS, os.path.join(PKG, "host", "Media.hpp"), os.path.join(PKG, "csrc", "lm_bkg_core.h")]


def build(verbose=False):
    os.makedirs(BUILD, exist_ok=True)
    cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", *INCLUDES, "-o", SO, SRC, *HOST_SRCS, "-lz"]
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
        L.bh_median.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_void_p]
        L.bh_rank.argtypes = [C.c_int32, C.c_int64]
        L.bh_rank.restype = C.c_uint32
        L.bh_write_png.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_void_p]
        L.bh_read_png.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_int64]
        _lib = L
    return _lib


def host_median(buf, pitch, k, rows, cols, pushes, permille):
    """csrc/lm_bkg_core.h on the host: `buf` holds k frames `pitch` bytes apart, pushed in `pushes` (sizes)."""
    out = np.zeros((rows, cols), np.uint8)
    pn = np.asarray(pushes, np.int32)
    assert int(pn.sum()) == k
    rc = lib().bh_median(buf.ctypes.data, pitch, pn.ctypes.data, len(pn), rows * cols, permille, out.ctypes.data)
    assert rc == 0, rc
    return out


def numpy_median(stack, permille):
    """The statement every layer is compared with."""
    k = stack.shape[0]
    return np.sort(stack, axis=0)[(permille * (k - 1)) // 1000]


def patterned(k, rows, cols, seed):
    """k random u8 frames with the value patterns in fixed columns (as many as
    the width holds): constant 0, constant 255, alternating {0, 255}, two values
    with an exact tie at even k, a ramp that hits another bin every frame,
    values within +-2 of 128."""
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, size=(k, rows, cols), dtype=np.uint8)
    i = np.arange(k)
    pats = [np.zeros(k), np.full(k, 255), np.where(i % 2, 255, 0), np.where(i < k // 2, 200, 40),
            (37 + 5 * i) % 256, 126 + rng.integers(0, 5, size=k)]
    for c, p in enumerate(pats):
        if c < cols:
            f[:, :, c] = p.astype(np.uint8)[:, None]
    if cols >= 12:  # the same again next to the right edge (the last, possibly short, group of pixels)
        for c, p in enumerate(pats):
            f[:, -1, cols - 1 - c] = p.astype(np.uint8)
    return f


def padded(stack, pad):
    """(buffer, pitch): the frames `rows * cols + pad` bytes apart, 0xEE between them."""
    k = stack.shape[0]
    fb = stack.shape[1] * stack.shape[2]
    buf = np.full(k * (fb + pad), 0xEE, np.uint8)
    buf.reshape(k, fb + pad)[:, :fb] = stack.reshape(k, fb)
    return buf, fb + pad


def pushes_of(k, max_batch):
    return [min(max_batch, k - s) for s in range(0, k, max_batch)]


# (name, rows, cols, pad, K, max_batch): the smallest shapes at which the indexing can go wrong
SHAPES = (("1x1", 1, 1, 0, 1, 1), ("3x37_padded_evenK", 3, 37, 5, 2, 2), ("8x64_short_last_batch", 8, 64, 0, 7, 3),
          ("16x130_dword_and_tail", 16, 130, 0, 33, 33), ("5x7_unaligned_pitch", 5, 7, 2, 9, 4))


@functools.lru_cache(maxsize=None)
def shape_stack(name):
    for n, rows, cols, pad, k, mb in SHAPES:
        if n == name:
            f = patterned(k, rows, cols, seed=rows * 1000 + cols)
            f.setflags(write=False)
            return f
    raise KeyError(name)


# ---- host/Background.hpp's checks that precede any GPU call (tests/cpp/bkg_host_harness.cpp; links the host library)
HOST_SO = os.path.join(BUILD, "libbkg_host_harness.so")
HOST_SRC = os.path.join(HERE, "cpp", "bkg_host_harness.cpp")


def build_host(verbose=False):
    os.makedirs(BUILD, exist_ok=True)
    cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", *INCLUDES, "-o", HOST_SO, HOST_SRC, "-L" + PKG,
           "-llocomouse_host", "-llocomouse_hip", "-Wl,-rpath,$ORIGIN/../../../locomouse_cpp_amd"]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return HOST_SO


_host_lib = None


def host_lib():
    global _host_lib
    if _host_lib is None:
        from locomouse_cpp_amd import runtime
        runtime.lib()  # torch's HIP runtime first, then the C-ABI library
        deps = [HOST_SRC, os.path.join(PKG, "liblocomouse_host.so"), os.path.join(PKG, "host", "Background.hpp"),
                os.path.join(PKG, "host", "LocoMouse.hpp")]
        if not os.path.exists(HOST_SO) or any(os.path.getmtime(d) > os.path.getmtime(HOST_SO) for d in deps):
            build_host()
        _host_lib = C.CDLL(HOST_SO)
    return _host_lib


def refusal(n_frames, rows=8, cols=8, stride=1, permille=500):
    """The message estimate_background refuses such a video with, before it reads a frame."""
    msg = C.create_string_buffer(512)
    rc = host_lib().bhh_refusal(C.c_uint(n_frames), rows, cols, stride, permille, msg, 512)
    assert rc == 0, rc
    return msg.value.decode()


def parse_spec(spec):
    """(stride, permille) of an LM_BACKGROUND value, or the parser's message (str)."""
    s, p = C.c_int(), C.c_int()
    msg = C.create_string_buffer(512)
    if host_lib().bhh_parse(spec.encode(), C.byref(s), C.byref(p), msg, 512):
        return msg.value.decode()
    return s.value, p.value
