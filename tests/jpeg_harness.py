"""ctypes access to tests/cpp/jpeg_harness.cpp (the host JPEG decoder, and the
device decoder's scan code run lane by lane on the CPU), and the JPEG streams
the device-decode tests share.  The harness links no GPU library."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "locomouse_cpp_amd")
BUILD = os.path.join(HERE, "cpp", "_build")
SO = os.path.join(BUILD, "libjpeg_harness.so")
SRC = os.path.join(HERE, "cpp", "jpeg_harness.cpp")
INCLUDES = ["-I" + os.path.join(PKG, "host"), "-I" + os.path.join(PKG, "csrc"), "-I" + os.path.join(ROOT, "include")]

sys.path.insert(0, HERE)
import media_writers as MW  # noqa: E402

SUBSEQ_MIN, SUBSEQ_DEFAULT, CHUNK = 4, 64, 128  # include/locomouse_jpeg.h


def _deps():
    return [SRC, os.path.join(PKG, "host", "Jpeg.cpp"), os.path.join(PKG, "host", "Jpeg.hpp"),
            os.path.join(PKG, "csrc", "lm_jpeg_scan.h"), os.path.join(PKG, "csrc", "lm_jpeg_hdr.h")]


def build(verbose=False):
    os.makedirs(BUILD, exist_ok=True)
    cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", *INCLUDES, "-o", SO, SRC,
           os.path.join(PKG, "host", "Jpeg.cpp")]
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
        L.jh_host_decode.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_char_p, C.c_int]
        L.jh_host_decode.restype = C.c_int
        L.jh_lanes_decode.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_int64, C.c_void_p, C.c_char_p, C.c_int]
        L.jh_lanes_decode.restype = C.c_int
        L.jh_host_coefficients.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_int64]
        L.jh_host_coefficients.restype = C.c_int64
        _lib = L
    return _lib


def host_decode(data, rows, cols):
    """The host decoder's channel 0 (rows x cols u8), or the rejection message (str)."""
    out = np.zeros((rows, cols), np.uint8)
    err = C.create_string_buffer(256)
    if lib().jh_host_decode(data, len(data), rows, cols, out.ctypes.data, err, 256):
        return err.value.decode()
    return out


def host_coefficients(data, rows, cols):
    """The host decoder's quantised coefficients [blocks, 64] in scan order (Cr blocks zeroed)."""
    coef = np.zeros((3 * ((rows + 15) // 8 + 1) * ((cols + 15) // 8 + 1), 64), np.int16)
    n = lib().jh_host_coefficients(data, len(data), coef.ctypes.data, coef.size)
    assert n >= 0, "the host decoder gave no coefficients"
    return coef[:n]


def lanes_decode(data, rows, cols, subseq=SUBSEQ_DEFAULT, lanes=CHUNK, max_blocks=None):
    """The subsequence scheme lane by lane on the CPU: (class, pixels, coefficients, stats dict, reason)."""
    out = np.zeros((rows, cols), np.uint8)
    nb = max_blocks or 3 * ((rows + 15) // 8 + 1) * ((cols + 15) // 8 + 1)
    coef = np.zeros((nb, 64), np.int16)
    st = np.zeros(5, np.uint32)
    err = C.create_string_buffer(256)
    cls = lib().jh_lanes_decode(data, len(data), rows, cols, subseq, lanes, out.ctypes.data, coef.ctypes.data, coef.size,
                                st.ctypes.data, err, 256)
    stats = dict(subsequences=int(st[0]), rounds=int(st[1]), max_chunk_rounds=int(st[2]), err=int(st[3]), blocks=int(st[4]))
    return cls, out, coef[:int(st[4])], stats, err.value.decode()


def frames(n, h, w, seed):
    """test_mjpeg._frames: smooth structure + noise + hard edges."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    out = []
    for k in range(n):
        base = 128 + 90 * np.sin(x / (3.0 + k) + y / 7.0) * np.cos(y / (5.0 + k))
        base += rng.normal(0, 25, size=(h, w))
        base[(x // 9 + y // 5 + k) % 4 == 0] = 255 if k % 2 else 0
        out.append(np.clip(base, 0, 255).astype(np.uint8))
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def stream_list():
    """[(name, rows, cols, [jpeg bytes, ...])]: the in-scope streams every
    decoder test runs (built once per process)."""
    S = []

    def add(name, f, **kw):
        S.append((name, f.shape[1], f.shape[2], MW.jpeg_frames(f, **kw)))

    for q in (5, 50, 95, 100):
        add(f"grey_q{q}", frames(2, 37, 53, q), mode="L", quality=q)
    for sub in (0, 1, 2):
        for shape in ((37, 53), (48, 64), (17, 9), (1, 1), (8, 200)):
            add(f"colour_s{sub}_{shape[0]}x{shape[1]}", frames(2, *shape, sub), mode="RGB", quality=85, subsampling=sub)
    f = frames(2, 40, 40, 3)
    f[:, ::2, ::2] = 255
    f[:, 1::2, 1::2] = 0
    add("colour_q100_range_limit", f, mode="RGB", quality=100, subsampling=2)
    for mode in ("L", "RGB"):
        for tag, kw in (("blocks3", dict(restart_marker_blocks=3)), ("rows1", dict(restart_marker_rows=1)),
                        ("blocks1", dict(restart_marker_blocks=1))):
            add(f"restart_{tag}_{mode}", frames(2, 45, 70, 7), mode=mode, quality=80, subsampling=2, **kw)
    for mode in ("L", "RGB"):
        add(f"avi1_no_dht_{mode}", frames(2, 32, 48, 11), mode=mode, quality=70, subsampling=1, strip_dht=True)
    add("optimize_rgb", frames(3, 33, 65, 4), mode="RGB", quality=90, optimize=True)
    add("optimize_grey", frames(3, 33, 65, 5), mode="L", quality=90, optimize=True)
    add("flat", np.full((1, 24, 40), 128, np.uint8), mode="L", quality=90)
    # one high-frequency cosine per block: long zero runs (ZRL symbols)
    y, x = np.mgrid[0:32, 0:48]
    zr = 128 + 100 * np.cos((2 * (x % 8) + 1) * 7 * np.pi / 16) * np.cos((2 * (y % 8) + 1) * 7 * np.pi / 16)
    add("zrl", np.clip(zr, 0, 255).astype(np.uint8)[None], mode="L", quality=95)
    # symbols longer than the smallest subsequence: the sync rounds walk lane by lane
    rng = np.random.default_rng(100)
    add("dense_q100", rng.integers(0, 256, size=(1, 16, 40)).astype(np.uint8), mode="RGB", quality=100, subsampling=0,
        restart_marker_rows=1)
    rng = np.random.default_rng(64512)
    add("long_scan", rng.integers(0, 256, size=(1, 64, 512)).astype(np.uint8), mode="L", quality=95)
    return tuple(S)


def sixteen_bit_streams():
    """SOF1 frames with 16-bit quantisation tables (test_mjpeg's), grey and colour: out of the device's scope."""
    qt = [[257 + 27 * i for i in range(64)], [300 + 25 * i for i in range(64)]]
    f = frames(1, 40, 48, 11)
    return [(40, 48, MW.jpeg_frames(f, mode="L", qtables=qt[:1])[0]),
            (40, 48, MW.jpeg_frames(f, mode="RGB", qtables=qt, subsampling=0)[0])]


def progressive_stream():
    return 24, 24, MW.jpeg_frames(frames(1, 24, 24, 2), mode="L", progressive=True)[0]


def scan_bounds(j):
    """(start, end) of the first scan's entropy-coded bytes."""
    i = 2
    while j[i + 1] != 0xDA:
        i += 2 + (j[i + 2] << 8 | j[i + 3])
    s = i + 2 + (j[i + 2] << 8 | j[i + 3])
    e = s
    while not (j[e] == 0xFF and j[e + 1] != 0 and not 0xD0 <= j[e + 1] <= 0xD7):
        e += 1
    return s, e


def cut_scan(j, frac=0.7):
    """The stream with its scan cut at `frac` of its length (EOI kept)."""
    s, e = scan_bounds(j)
    return j[:s + int((e - s) * frac)] + b"\xff\xd9"


# ---- the host mirror on an MJPEG video in memory (tests/cpp/jpeg_host_harness.cpp; needs the GPU libraries)
HOST_SO = os.path.join(BUILD, "libjpeg_host_harness.so")
HOST_SRC = os.path.join(HERE, "cpp", "jpeg_host_harness.cpp")


def build_host(verbose=False):
    os.makedirs(BUILD, exist_ok=True)
    cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", *INCLUDES, "-o", HOST_SO, HOST_SRC, "-L" + PKG,
           "-llocomouse_host", "-llocomouse_hip", "-Wl,-rpath,$ORIGIN/../../../locomouse_cpp_amd"]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return HOST_SO


_host_lib = None


def run_host_mirror(cfg, jpegs, bb_params, batch=16, device_decode=False):
    """getBoundingBox (whole-video pass) + the frame loop of the host mirror on
    the JPEG frames; returns (corners [n, 3], (side, bottom) box sizes,
    candidate counts [n, 2], fallback frames)."""
    global _host_lib
    from locomouse_cpp_amd import runtime
    from locomouse_cpp_amd.abi import lm_rect
    if _host_lib is None:
        runtime.lib()  # torch's HIP runtime first, then the C-ABI library
        deps = [HOST_SRC, os.path.join(ROOT, "include", "locomouse_jpeg.h"), os.path.join(ROOT, "include", "locomouse_hip.h"),
                os.path.join(PKG, "liblocomouse_host.so"),
                *[os.path.join(PKG, "host", f) for f in os.listdir(os.path.join(PKG, "host")) if f.endswith(".hpp")]]
        if not os.path.exists(HOST_SO) or any(os.path.getmtime(d) > os.path.getmtime(HOST_SO) for d in deps):
            build_host()
        _host_lib = C.CDLL(HOST_SO)
        _host_lib.jhh_run.restype = C.c_int
    n = len(jpegs)
    keep = [bytes(j) for j in jpegs]
    ptrs = (C.c_char_p * n)(*keep)
    sizes = (C.c_size_t * n)(*[len(j) for j in keep])
    corners = np.zeros((n, 3), np.uint32)
    boxes = (lm_rect * 2)()
    cands = np.zeros((n, 2), np.int32)
    fb = C.c_int32(0)
    err = C.create_string_buffer(512)
    rc = _host_lib.jhh_run(C.byref(cfg.setup), C.byref(cfg.params), C.byref(cfg.model), C.byref(bb_params), ptrs, sizes,
                           C.c_int(n), C.c_int(batch), C.c_int(int(device_decode)), C.c_void_p(corners.ctypes.data),
                           boxes, C.c_void_p(cands.ctypes.data), C.byref(fb), err, C.c_int(512))
    if rc:
        raise RuntimeError(err.value.decode())
    return corners, (boxes[0].tuple(), boxes[1].tuple()), cands, fb.value


def _sos_at(j):
    i = 2
    while j[i + 1] != 0xDA:
        i += 2 + (j[i + 2] << 8 | j[i + 3])
    return i


def with_dri(j, interval):
    """The stream with a DRI segment put in front of its SOS (and no RSTn in the scan)."""
    i = _sos_at(j)
    return j[:i] + b"\xff\xdd\x00\x04" + bytes([interval >> 8, interval & 255]) + j[i:]


def without_last_rst(j):
    """A restart-marker stream with its last RSTn taken out."""
    s, e = scan_bounds(j)
    k = max(j.rfind(bytes([0xFF, 0xD0 + m]), s, e) for m in range(8))
    assert k >= 0
    return j[:k] + j[k + 2:]


def _sof_at(j):
    i = 2
    while j[i + 1] not in (0xC0, 0xC1):
        i += 2 + (j[i + 2] << 8 | j[i + 3])
    return i


def with_sampling(j, comp, h, v):
    """The stream with component `comp`'s sampling factors rewritten in its SOF (header surgery: the scan no longer fits)."""
    i = _sof_at(j) + 4 + 6 + 3 * comp + 1
    return j[:i] + bytes([h << 4 | v]) + j[i + 1:]


def with_sos_order(j, order):
    """A 3-component stream whose SOS names its components in another order."""
    i = _sos_at(j) + 5
    sel = [j[i + 2 * k:i + 2 * k + 2] for k in range(3)]
    return j[:i] + b"".join(sel[k] for k in order) + j[i + 6:]


def as_three_scans(j):
    """A 3-component stream rewritten as non-interleaved: its SOS is split into
    three one-component SOS segments (the scan bytes follow the first; the rest
    are empty scans).  Only the headers matter to the tests that use it."""
    i = _sos_at(j)
    n = 2 + (j[i + 2] << 8 | j[i + 3])
    sel = [j[i + 5 + 2 * k:i + 7 + 2 * k] for k in range(3)]
    tail = j[i + n - 3:i + n]
    one = [b"\xff\xda\x00\x08\x01" + sel[k] + tail for k in range(3)]
    s, e = scan_bounds(j)
    return j[:i] + one[0] + j[s:e] + one[1] + one[2] + j[e:]
