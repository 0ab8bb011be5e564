"""ctypes access to tests/cpp/train_harness.cpp (the host build of
csrc/lm_train_core.h; no GPU library), and the sample sets the training
tests share."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "locomouse_cpp_amd")
BUILD = os.path.join(HERE, "cpp", "_build")
SO = os.path.join(BUILD, "libtrain_harness.so")
SRC = os.path.join(HERE, "cpp", "train_harness.cpp")
CHECK_SRC = os.path.join(HERE, "cpp", "train_core_check.cpp")
CORE = os.path.join(PKG, "csrc", "lm_train_core.h")
INCLUDES = ["-I" + os.path.join(PKG, "csrc"), "-I" + os.path.join(ROOT, "include")]


def build(verbose=False):
    os.makedirs(BUILD, exist_ok=True)
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", *INCLUDES, "-o", SO, SRC]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return SO


_lib = None


def lib():
    """The harness, built on first use (and again when a source is newer)."""
    global _lib
    if _lib is None:
        if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in (SRC, CORE)):
            build()
        L = C.CDLL(SO)
        L.th_objective.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_double, C.c_double,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.c_void_p]
        L.th_objective.restype = C.c_int64
        L.th_hessvec.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.th_margins.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]
        L.th_linesearch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_double, C.c_double,
                                    C.c_double, C.c_double, C.POINTER(C.c_double)]
        L.th_fused_score.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double]
        L.th_fused_score.restype = C.c_float
        _lib = L
    return _lib


def padded(P):
    """(buffer, pitch): the patches [N, D] in rows of lmt_pitch(D) bytes, zeros after D."""
    P = np.ascontiguousarray(P, np.uint8)
    n, d = P.shape
    pitch = lib().th_pitch(d)
    buf = np.zeros((n, pitch), np.uint8)
    buf[:, :d] = P
    return buf, pitch


def host_objective(P, y, c_pos, c_neg, wb):
    buf, pitch = padded(P)
    n, d = P.shape
    y = np.ascontiguousarray(y, np.int8)
    wb = np.ascontiguousarray(wb, np.float64)
    z, a, g = np.zeros(n), np.zeros(n), np.zeros(d + 1)
    F = C.c_double()
    na = lib().th_objective(buf.ctypes.data, pitch, y.ctypes.data, n, d, c_pos, c_neg, wb.ctypes.data, z.ctypes.data,
                            a.ctypes.data, C.byref(F), g.ctypes.data)
    return F.value, g, z, a, na


def host_hessvec(P, a, v):
    buf, pitch = padded(P)
    n, d = P.shape
    a = np.ascontiguousarray(a, np.float64)
    v = np.ascontiguousarray(v, np.float64)
    out = np.zeros(d + 1)
    lib().th_hessvec(buf.ctypes.data, pitch, n, d, a.ctypes.data, v.ctypes.data, out.ctypes.data)
    return out


def host_linesearch(y, z, xd, c_pos, c_neg, wd, dd, gd):
    y = np.ascontiguousarray(y, np.int8)
    z = np.ascontiguousarray(z, np.float64)
    xd = np.ascontiguousarray(xd, np.float64)
    dF = C.c_double()
    k = lib().th_linesearch(y.ctypes.data, z.ctypes.data, xd.ctypes.data, len(y), c_pos, c_neg, wd, dd, gd, C.byref(dF))
    return k, dF.value


def fused_score(patch, W, rho):
    """filter2D's fused fp32 chain over one u8 patch with float64 weights W (np.float32)."""
    patch = np.ascontiguousarray(patch, np.uint8)
    W = np.ascontiguousarray(W, np.float64)
    assert patch.size == W.size
    return np.float32(lib().th_fused_score(patch.ctypes.data, W.ctypes.data, W.size, float(rho)))


# ---- sample sets.  KINDS: what the data looks like; every set is u8 [N, D] with labels +1 / -1.
KINDS = ("separable", "overlapping", "duplicated", "one_class", "constant_column", "costs")


def kind_costs(kind):
    return (10.0, 1.0) if kind == "costs" else (1.0, 1.0)


@functools.lru_cache(maxsize=None)
def sample_set(kind, n, d, seed=0):
    """(P u8 [n, d], y int8 [n]), read-only.  A blob per class on a textured
    ground: far apart (separable), close (overlapping, costs), every row
    twice (duplicated), positives only (one_class), column 0 at 200
    (constant_column)."""
    rng = np.random.default_rng(1000 * d + 7 * n + seed + sum(map(ord, kind)))
    y = np.where(np.arange(n) % 3 == 0, 1, -1).astype(np.int8)
    if kind == "one_class":
        y[:] = 1
    sep = 90.0 if kind == "separable" else 12.0
    tmpl = rng.uniform(-1, 1, size=d)
    P = 110.0 + 25.0 * rng.standard_normal((n, d)) + sep * y[:, None].astype(np.float64) * tmpl[None, :]
    P = np.clip(np.rint(P), 0, 255).astype(np.uint8)
    if kind == "duplicated":
        h = (n + 1) // 2
        P[h:] = P[:n - h]
        y[h:] = y[:n - h]
        if n >= 4:  # one duplicated patch carries both labels
            P[n - 1] = P[0]
            y[n - 1] = -y[0]
    if kind == "constant_column":
        P[:, 0] = 200
    P.setflags(write=False)
    y.setflags(write=False)
    return P, y


# ---- host/Train.hpp's pure host functions and host/Inputs.hpp's model writer
# (tests/cpp/train_host_harness.cpp; links the host library, no GPU call)
HOST_SO = os.path.join(BUILD, "libtrain_host_harness.so")
HOST_SRC = os.path.join(HERE, "cpp", "train_host_harness.cpp")
MODEL_ORDER = ("paw_side", "paw_bottom", "tail_side", "tail_bottom", "snout_side", "snout_bottom")  # the model file's
FEATURES = ("paw_bottom", "snout_bottom", "tail_bottom", "paw_side", "snout_side", "tail_side")  # TrainFeature


def build_host(verbose=False):
    os.makedirs(BUILD, exist_ok=True)
    cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-I" + os.path.join(PKG, "host"), *INCLUDES, "-o",
           HOST_SO, HOST_SRC, "-L" + PKG, "-llocomouse_host", "-llocomouse_hip",
           "-Wl,-rpath,$ORIGIN/../../../locomouse_cpp_amd"]
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
        deps = [HOST_SRC, os.path.join(PKG, "liblocomouse_host.so"), os.path.join(PKG, "host", "Train.hpp"),
                os.path.join(PKG, "host", "Inputs.hpp")]
        if not os.path.exists(HOST_SO) or any(os.path.getmtime(d) > os.path.getmtime(HOST_SO) for d in deps):
            build_host()
        L = C.CDLL(HOST_SO)
        P, I, D = C.c_void_p, C.c_int, C.c_double
        L.thh_select_mined.argtypes = [P, I, P, I, I, P, I, P, I]
        L.thh_initial_negatives.argtypes = [I, I, P, I, P, I, I, I, I, P, I]
        L.thh_parse_spec.argtypes = [C.c_char_p, P, C.c_char_p, I]
        L.thh_write_model.argtypes = [C.c_char_p, P, P, P, P]
        L.thh_load_model.argtypes = [C.c_char_p, P, I, P, P, P]
        _host_lib = L
    return _host_lib


def _triples(a):
    a = np.ascontiguousarray(np.asarray(a, np.int32).reshape(-1, 3))
    return a, a.ctypes.data if len(a) else None, len(a)


def select_mined(cands, labels, r_neg, seen=()):
    """host/Train.hpp select_mined: [(frame, x, y)] taken from cands, in their order."""
    c, cp, nc = _triples(cands)
    l, lp, nl = _triples(labels)
    s, sp, ns = _triples(list(seen))
    out = np.zeros((max(nc, 1), 3), np.int32)
    n = host_lib().thh_select_mined(cp, nc, lp, nl, r_neg, sp, ns, out.ctypes.data,
                                    len(out))
    return [tuple(map(int, r)) for r in out[:n]]


def initial_negatives(feature, frame, labels, view, rows, cols, r_neg, neg_per_frame):
    l, lp, nl = _triples(labels)
    v = np.asarray(view, np.int32)
    out = np.zeros((max(neg_per_frame, 1), 3), np.int32)
    n = host_lib().thh_initial_negatives(feature, frame, lp, nl, v.ctypes.data, rows, cols, r_neg,
                                         neg_per_frame, out.ctypes.data, len(out))
    return [tuple(map(int, r)) for r in out[:n]]


def parse_spec(spec):
    """(c_pos, c_neg, eps, rounds, neg_per_frame) of an LM_TRAIN value, or the parser's message (str)."""
    out = np.zeros(5)
    msg = C.create_string_buffer(512)
    if host_lib().thh_parse_spec(spec.encode(), out.ctypes.data, msg, 512):
        return msg.value.decode()
    return float(out[0]), float(out[1]), float(out[2]), int(out[3]), int(out[4])


def write_model(path, weights, biases):
    """weights / biases: dicts by detector name (synthetic.DETECTOR_SPECS)."""
    ws = [np.ascontiguousarray(weights[n], np.float64) for n in MODEL_ORDER]
    flat = np.concatenate([w.reshape(-1) for w in ws])
    rows = np.array([w.shape[0] for w in ws], np.int32)
    cols = np.array([w.shape[1] for w in ws], np.int32)
    b = np.array([biases[n] for n in MODEL_ORDER], np.float64)
    rc = host_lib().thh_write_model(os.fsencode(path), flat.ctypes.data, rows.ctypes.data, cols.ctypes.data, b.ctypes.data)
    assert rc == 0, rc


def load_model(path):
    """(weights, biases) dicts by detector name, through host/Inputs.hpp's load_model."""
    flat = np.zeros(1 << 16)
    rows, cols = np.zeros(6, np.int32), np.zeros(6, np.int32)
    b = np.zeros(6)
    rc = host_lib().thh_load_model(os.fsencode(path), flat.ctypes.data, len(flat), rows.ctypes.data, cols.ctypes.data,
                                   b.ctypes.data)
    assert rc == 0, rc
    weights, off = {}, 0
    for k, n in enumerate(MODEL_ORDER):
        weights[n] = flat[off:off + rows[k] * cols[k]].reshape(rows[k], cols[k]).copy()
        off += rows[k] * cols[k]
    return weights, dict(zip(MODEL_ORDER, map(float, b)))
