"""The calibration estimate's definition (include/locomouse_calib.h,
csrc/lm_calib_core.h) restated for the tests: the per-view record in numpy, the
fit and the map operation for operation in Python floats (so they equal the
C++, built with -ffp-contract=off, to the bit), the frames the record tests
share, a marker-video generator with a "camera" that resamples the side view
by a column table, and ctypes access to tests/cpp/calib_host_harness.cpp (the
core's host record and host/Calibration.hpp's parser, checks and writer)."""
import ctypes as C
import functools
import math
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "locomouse_cpp_amd")
BUILD = os.path.join(HERE, "cpp", "_build")
CHECK_SRC = os.path.join(HERE, "cpp", "calib_core_check.cpp")
INCLUDES = ["-I" + os.path.join(PKG, "host"), "-I" + os.path.join(PKG, "csrc"), "-I" + os.path.join(ROOT, "include")]

RECORD_DTYPE = np.dtype([(n, "<i4") for n in ("peak", "px", "py", "n_above", "n_in", "clipped")]
                        + [(n, "<i8") for n in ("S", "Sx", "Sy")])
DEFAULTS = dict(threshold=40, radius=12, min_peak=80, min_area=12, max_stray=8)


def opts_of(**kw):
    o = dict(DEFAULTS)
    o.update(kw)
    return o


# ---------------------------------------------------------------- the record

def ref_record(frame, bkg, split_row, view, o):
    """One view's record of one frame [rows, cols] u8, as a tuple in RECORD_DTYPE's order."""
    rows, cols = frame.shape
    r0, r1 = (split_row, rows) if view else (0, split_row)
    d = np.maximum(frame.astype(np.int32) - bkg.astype(np.int32), 0)
    v = d[r0:r1]
    peak = int(v.max())
    at = int(np.argmax(v))  # the first position in row-major order that holds the maximum
    py, px = r0 + at // cols, at % cols
    thr, R = o["threshold"], o["radius"]
    n_above = int((v > thr).sum())
    wr0, wr1 = max(py - R, r0), min(py + R, r1 - 1)
    wc0, wc1 = max(px - R, 0), min(px + R, cols - 1)
    clipped = int(py - R < r0 or py + R > r1 - 1 or px - R < 0 or px + R > cols - 1)
    w = d[wr0:wr1 + 1, wc0:wc1 + 1].astype(np.int64)
    w = np.where(w > thr, w, 0)
    cc = np.arange(wc0, wc1 + 1, dtype=np.int64)[None, :]
    rr = np.arange(wr0, wr1 + 1, dtype=np.int64)[:, None]
    return (peak, px, py, n_above, int((w > 0).sum()), clipped, int(w.sum()), int((w * cc).sum()), int((w * rr).sum()))


def ref_records(frames, bkg, split_row, o):
    """[n, 2] RECORD_DTYPE (side, bottom) of frames [n, rows, cols] u8."""
    out = np.zeros((len(frames), 2), RECORD_DTYPE)
    for f, frame in enumerate(frames):
        for view in (0, 1):
            out[f, view] = ref_record(frame, bkg, split_row, view, o)
    return out


def assert_records_equal(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for name in RECORD_DTYPE.names:
        bad = np.argwhere(got[name] != want[name])
        assert len(bad) == 0, (what, name, bad[:4].tolist(), got[name][tuple(bad[0])], want[name][tuple(bad[0])])


# ---------------------------------------------------------------- the fit and the map

class Refusal(Exception):
    def __init__(self, kind, text):
        super().__init__(text)
        self.kind = kind  # "count", "range", "definite" or "monotone"


def _view_ok(r, o):
    return (r["peak"] >= o["min_peak"] and r["n_in"] >= o["min_area"] and r["n_above"] - r["n_in"] <= o["max_stray"]
            and r["clipped"] == 0)


def ref_samples(rec, o):
    """[(frame, xb, xs)] in frame order."""
    out = []
    for f in range(len(rec)):
        s, b = rec[f, 0], rec[f, 1]
        if _view_ok(s, o) and _view_ok(b, o) and s["S"] > 0 and b["S"] > 0:
            out.append((f, float(int(b["Sx"])) / float(int(b["S"])), float(int(s["Sx"])) / float(int(s["S"]))))
    return out


def _t(x, cols):
    half = float(cols) / 2.0
    return (x - half) / half


def ref_poly(coef, t):
    p = coef[-1]
    for k in range(len(coef) - 2, -1, -1):
        p = p * t + coef[k]
    return p


def ref_poly_dt(coef, t):
    deg = len(coef) - 1
    d = float(deg) * coef[deg]
    for k in range(deg - 1, 0, -1):
        d = d * t + float(k) * coef[k]
    return d


def _solve(sm, use, cols, degree):
    N = degree + 1
    M = [0.0] * (2 * degree + 1)
    bv = [0.0] * N
    for (f, xb, xs), u in zip(sm, use):
        if not u:
            continue
        t = _t(xb, cols)
        pw = 1.0
        for k in range(2 * degree + 1):
            M[k] = M[k] + pw
            if k < N:
                bv[k] = bv[k] + pw * xs
            pw = pw * t
    L = [[0.0] * N for _ in range(N)]
    for j in range(N):
        s = M[j + j]
        for k in range(j):
            s = s - L[j][k] * L[j][k]
        if not s > 0.0:
            return None
        L[j][j] = math.sqrt(s)
        for i in range(j + 1, N):
            v = M[i + j]
            for k in range(j):
                v = v - L[i][k] * L[j][k]
            L[i][j] = v / L[j][j]
    y = [0.0] * N
    for i in range(N):
        v = bv[i]
        for k in range(i):
            v = v - L[i][k] * y[k]
        y[i] = v / L[i][i]
    coef = [0.0] * N
    for i in range(N - 1, -1, -1):
        v = y[i]
        for k in range(i + 1, N):
            v = v - L[k][i] * coef[k]
        coef[i] = v / L[i][i]
    return coef


def _count_range(sm, use, cols, degree):
    xs = [s[1] for s, u in zip(sm, use) if u]
    n = len(xs)
    lo, hi = (min(xs), max(xs)) if n else (0.0, 0.0)
    if n < 8 * (degree + 1):
        raise Refusal("count", f"{n} samples, {8 * (degree + 1)} needed")
    if hi - lo < float(cols) / 4.0:
        raise Refusal("range", f"{lo} to {hi}")
    return n, lo, hi


def ref_fit(rec, cols, o, degree=2, max_resid=1.5):
    sm = ref_samples(rec, o)
    use = [True] * len(sm)
    for rnd in range(2):
        n, lo, hi = _count_range(sm, use, cols, degree)
        coef = _solve(sm, use, cols, degree)
        if coef is None:
            raise Refusal("definite", "not positive definite")
        if rnd == 0:
            for i, (f, xb, xs) in enumerate(sm):
                if abs(xs - ref_poly(coef, _t(xb, cols))) > max_resid:
                    use[i] = False
    ss, worst = 0.0, 0.0
    for (f, xb, xs), u in zip(sm, use):
        if u:
            r = xs - ref_poly(coef, _t(xb, cols))
            ss = ss + r * r
            worst = max(worst, abs(r))
    return dict(n_frames=len(rec), n_samples=len(sm), n_used=n, degree=degree, rms=math.sqrt(ss / float(n)),
                max_abs_resid=worst, lo=lo, hi=hi, coef=coef)


def ref_warp(fit, cols, c):
    half = float(cols) / 2.0
    coef = fit["coef"]
    for end, outside in ((fit["lo"], c < fit["lo"]), (fit["hi"], c > fit["hi"])):
        if outside:
            t = _t(end, cols)
            return ref_poly(coef, t) + ref_poly_dt(coef, t) / half * (c - end)
    return ref_poly(coef, _t(c, cols))


def ref_columns(fit, cols):
    m = []
    for c in range(cols):
        v = math.floor(ref_warp(fit, cols, float(c)) + 0.5)
        v = int(min(max(v, 0), cols - 1))
        if m and v < m[-1]:
            raise Refusal("monotone", f"column {c} maps to {v} after {m[-1]}")
        m.append(v)
    return m


def ref_map(fit, rows, cols, split_row):
    m = np.array(ref_columns(fit, cols), np.int64)
    idx = np.arange(rows * cols, dtype=np.int64).reshape(rows, cols)
    idx[:split_row] = np.arange(split_row, dtype=np.int64)[:, None] * cols + m[None, :]
    boxes = np.array([[0, 0, cols, split_row], [0, split_row, cols, rows - split_row]], np.int32)
    return idx.astype(np.int32), boxes


def records_of_points(points, o=None, cols=1024, weight=20011):
    """Records [n, 2] whose samples are the given (xb, xs) pairs (None: a frame without a marker): S is a fixed
    integer and Sx the nearest integer to x * S, so the coordinates are what the division gives, not x itself."""
    o = o or DEFAULTS
    rec = np.zeros((len(points), 2), RECORD_DTYPE)
    for f, p in enumerate(points):
        if p is None:
            continue
        for view, x in ((1, p[0]), (0, p[1])):
            S = weight + 7 * f + view
            rec[f, view] = (200, int(x), 40 + 100 * view, o["min_area"] + 30, o["min_area"] + 30, 0, S, int(round(x * S)),
                            (40 + 100 * view) * S)
    return rec


# ---------------------------------------------------------------- frames of the record tests

# (name, rows, cols, split_row, radius): the smallest shapes at which the kernel's indexing can go wrong
RECORD_SHAPES = (("16x130_s5", 16, 130, 5, 3), ("8x64_s1", 8, 64, 1, 3), ("8x64_s7", 8, 64, 7, 3),
                 ("8x64_s7_R100", 8, 64, 7, 100), ("16x130_s5_R0", 16, 130, 5, 0))


@functools.lru_cache(maxsize=None)
def record_scene(rows, cols, split_row, dark_bkg=False, thr=40):
    """(frames [n, rows, cols] u8, background [rows, cols] u8), read-only: noise; an all-dark frame; a frame darker
    than its background; a saturated frame; two equal peaks per view; the peak at each corner of each view; a frame
    whose blob is d == threshold next to d == threshold + 1; random blobs."""
    rng = np.random.default_rng(rows * 100000 + cols * 10 + split_row)
    B = np.zeros((rows, cols), np.int32) if dark_bkg else rng.integers(0, 61, size=(rows, cols)).astype(np.int32)
    frames = []

    def add(delta):
        frames.append(np.clip(B + delta, 0, 255).astype(np.uint8))

    frames.append(rng.integers(0, 256, size=(rows, cols), dtype=np.uint8))
    frames.append(np.zeros((rows, cols), np.uint8))           # all dark
    frames.append((B // 2).astype(np.uint8))                  # darker than the background wherever it is not 0
    frames.append(np.full((rows, cols), 255, np.uint8))       # saturated (d = 255 everywhere with a zero background)
    views = ((0, split_row), (split_row, rows))
    d = np.zeros((rows, cols), np.int32)                      # two equal peaks per view: the first must win
    for r0, r1 in views:
        d[r1 - 1, cols // 3] = 150
        d[r0, cols - 2] = 150
        d[r1 - 1, 1] = 149
    add(d)
    for cr in range(4):                                       # the peak at each corner of both views
        d = rng.integers(0, 30, size=(rows, cols)).astype(np.int32)
        for r0, r1 in views:
            r = r0 if cr < 2 else r1 - 1
            c = 0 if cr % 2 == 0 else cols - 1
            d[r, c] = 180
            d[r, max(c - 1, 0) if c else 1] = max(d[r, max(c - 1, 0) if c else 1], thr + 5)
        add(d)
    d = np.zeros((rows, cols), np.int32)                      # d == threshold is not counted
    for r0, r1 in views:
        d[r0:r1, cols // 2 - 2:cols // 2 + 3] = thr
        d[(r0 + r1) // 2, cols // 2] = thr + 1
    add(d)
    for k in range(3):                                        # blobs on noise
        d = rng.integers(0, thr + 2, size=(rows, cols)).astype(np.int32)
        for r0, r1 in views:
            r, c = int(rng.integers(r0, r1)), int(rng.integers(0, cols))
            d[max(r - 1, r0):min(r + 2, r1), max(c - 2, 0):c + 3] += 120
        add(d)
    out = np.stack(frames)
    out.setflags(write=False)
    Bu = B.astype(np.uint8)
    Bu.setflags(write=False)
    return out, Bu


def padded(stack, pad):
    """(buffer, pitch): the frames `rows * cols + pad` bytes apart, 0xEE between them."""
    k = stack.shape[0]
    fb = stack.shape[1] * stack.shape[2]
    buf = np.full(k * (fb + pad), 0xEE, np.uint8)
    buf.reshape(k, fb + pad)[:, :fb] = stack.reshape(k, fb)
    return buf, fb + pad


# ---------------------------------------------------------------- the marker video

ROWS, COLS, SPLIT = 256, 1024, 96
N_MARKER = 200
DISC_RADIUS, SWEEP = 5, (120, 900)


def camera_table(cols=COLS, offset=30, stretch=1.125):
    """h: camera column c of the side view shows scene column h[c] = floor((c + offset) / stretch)."""
    return np.floor((np.arange(cols) + offset) / stretch).astype(np.int64)


def through_camera(frames, h, split_row=SPLIT):
    """The frames as the camera records them: the side view's columns resampled by h, the bottom view as it is."""
    out = np.array(frames, copy=True)
    out[:, :split_row, :] = frames[:, :split_row, :][:, :, h]
    return out


def map_from_table(h, rows=ROWS, cols=COLS, split_row=SPLIT):
    """A calibration map built directly from h: the corrected side view's column c is the first camera column that
    shows scene column c (the nearest one that shows anything where none does)."""
    m = np.searchsorted(h, np.arange(cols), side="left")
    m = np.clip(m, 0, cols - 1)
    idx = np.arange(rows * cols, dtype=np.int64).reshape(rows, cols)
    idx[:split_row] = np.arange(split_row, dtype=np.int64)[:, None] * cols + m[None, :]
    return idx.astype(np.int32)


@functools.lru_cache(maxsize=None)
def marker_video(n=N_MARKER, seed=20261020):
    """n frames [ROWS, COLS] u8 of a bright disc seen in both views, sweeping x over SWEEP with y wandering, on a
    background of 16..31 plus noise of 0..5 per frame (far below the threshold), its side view through the camera
    of camera_table().  Read-only."""
    rng = np.random.default_rng(seed)
    clean = np.zeros((n, ROWS, COLS), np.uint8)
    rr = np.arange(-DISC_RADIUS, DISC_RADIUS + 1)
    disc = (rr[:, None] ** 2 + rr[None, :] ** 2) <= DISC_RADIUS ** 2
    for f in range(n):
        x = SWEEP[0] + ((SWEEP[1] - SWEEP[0]) * f) // (n - 1)
        for y in (48 + int(round(20 * math.sin(0.37 * f))), 176 + int(round(40 * math.sin(0.23 * f)))):
            clean[f, y - DISC_RADIUS:y + DISC_RADIUS + 1, x - DISC_RADIUS:x + DISC_RADIUS + 1][disc] = 180
    cam = through_camera(clean, camera_table())
    base = rng.integers(16, 32, size=(ROWS, COLS), dtype=np.uint8)
    cam += base[None]
    cam += rng.integers(0, 6, size=cam.shape, dtype=np.uint8)
    cam.setflags(write=False)
    return cam


def covered_columns(lo, hi):
    return np.arange(int(math.ceil(lo)), int(math.floor(hi)) + 1)


# ---------------------------------------------------------------- tests/cpp/calib_host_harness.cpp

HOST_SO = os.path.join(BUILD, "libcalib_host_harness.so")
HOST_SRC = os.path.join(HERE, "cpp", "calib_host_harness.cpp")


def build_host(verbose=False):
    os.makedirs(BUILD, exist_ok=True)
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", *INCLUDES, "-o", HOST_SO, HOST_SRC,
           "-L" + PKG, "-llocomouse_host", "-llocomouse_hip", "-Wl,-rpath,$ORIGIN/../../../locomouse_cpp_amd"]
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
        deps = [HOST_SRC, os.path.join(PKG, "liblocomouse_host.so"), os.path.join(PKG, "host", "Calibration.hpp"),
                os.path.join(PKG, "csrc", "lm_calib_core.h"), os.path.join(ROOT, "include", "locomouse_calib.h")]
        if not os.path.exists(HOST_SO) or any(os.path.getmtime(d) > os.path.getmtime(HOST_SO) for d in deps):
            build_host()
        L = C.CDLL(HOST_SO)
        L.chh_records.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.chh_parse.argtypes = [C.c_char_p, C.c_void_p, C.POINTER(C.c_double), C.c_char_p, C.c_int]
        L.chh_refusal.argtypes = [C.c_uint, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int]
        L.chh_write_yaml.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_int, C.c_char_p, C.c_int]
        _host_lib = L
    return _host_lib


def _opts_array(o):
    return (C.c_int32 * 6)(o["threshold"], o["radius"], o["min_peak"], o["min_area"], o["max_stray"], 0)


def host_records(buf, pitch, n, bkg, rows, cols, split_row, o):
    """csrc/lm_calib_core.h's record on the host for n frames `pitch` bytes apart in `buf`."""
    out = np.zeros((n, 2), RECORD_DTYPE)
    bkg = np.ascontiguousarray(bkg, np.uint8)
    rc = host_lib().chh_records(buf.ctypes.data, C.c_int64(pitch), n, bkg.ctypes.data, rows, cols, split_row, _opts_array(o),
                                out.ctypes.data)
    assert rc == 0, rc
    return out


def parse_spec(spec):
    """((threshold, radius, min_peak, min_area, max_stray), max_resid) of an LM_CALIB value, or the parser's message."""
    five = (C.c_int32 * 5)()
    resid = C.c_double()
    msg = C.create_string_buffer(512)
    if host_lib().chh_parse(spec.encode(), five, C.byref(resid), msg, 512):
        return msg.value.decode()
    return tuple(five), resid.value


def refusal(n_frames, rows, cols, split_row, degree=2):
    """The message estimate_calibration refuses such a video with, before it reads a frame or touches a device."""
    msg = C.create_string_buffer(512)
    rc = host_lib().chh_refusal(C.c_uint(n_frames), rows, cols, split_row, degree, msg, 512)
    assert rc == 0, rc
    return msg.value.decode()


def write_yaml(path, fit_raw, m, boxes, samples, split_row):
    """write_calibration_yaml of a result put together from lm_calib_fit's and lm_calib_map's outputs."""
    m = np.ascontiguousarray(m, np.int32)
    boxes = np.ascontiguousarray(boxes, np.int32)
    samples = np.ascontiguousarray(samples, np.float64).reshape(-1, 3)
    msg = C.create_string_buffer(512)
    rc = host_lib().chh_write_yaml(os.fsencode(path), m.shape[0], m.shape[1], split_row, C.byref(fit_raw), m.ctypes.data,
                                   boxes.ctypes.data, samples.ctypes.data, len(samples), msg, 512)
    return msg.value.decode() if rc else None
