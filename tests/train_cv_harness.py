"""ctypes access to tests/cpp/train_cv_harness.cpp (host/Train.hpp's pure host
functions of the cross-validation and csrc/lm_train_core.h's host statement
with a held-out group; links the host library, no GPU call), their Python
restatements, and what the cross-validation tests share."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np

import train_harness as TH

SO = os.path.join(TH.BUILD, "libtrain_cv_harness.so")
SRC = os.path.join(TH.HERE, "cpp", "train_cv_harness.cpp")
SCALES = (0.01, 0.1, 0.3, 1.0, 3.0, 10.0, 30.0, 100.0)  # the cost scales 0.01 .. 100


def build(verbose=False):
    os.makedirs(TH.BUILD, exist_ok=True)
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wall",
           "-I" + os.path.join(TH.PKG, "host"), *TH.INCLUDES, "-o", SO, SRC, "-L" + TH.PKG, "-llocomouse_host",
           "-llocomouse_hip", "-Wl,-rpath,$ORIGIN/../../../locomouse_cpp_amd"]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        from locomouse_cpp_amd import runtime
        runtime.lib()  # torch's HIP runtime first, then the C-ABI library
        deps = [SRC, TH.CORE, os.path.join(TH.PKG, "liblocomouse_host.so"), os.path.join(TH.PKG, "host", "Train.hpp")]
        if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
            build()
        L = C.CDLL(SO)
        P, I, D = C.c_void_p, C.c_int, C.c_double
        L.thc_parse_cv.argtypes = [C.c_char_p, P, I, C.c_char_p, I]
        L.thc_folds.argtypes = [P, I, I, P]
        L.thc_select.argtypes = [P, P, I, P]
        L.thc_check_cv.argtypes = [P, I, I, P, I, C.c_char_p, I]
        L.thc_objective.argtypes = [P, C.c_int64, P, P, C.c_int64, I, D, D, I, P, P, P, C.POINTER(D), P]
        L.thc_objective.restype = C.c_int64
        L.thc_linesearch.argtypes = [P, P, P, P, C.c_int64, D, D, I, D, D, D, C.POINTER(D)]
        _lib = L
    return _lib


def parse_cv(spec):
    """(folds, [scales]) of an LM_TRAIN_CV value, or the parser's message (str)."""
    out = np.zeros(40)
    msg = C.create_string_buffer(512)
    if lib().thc_parse_cv(spec.encode(), out.ctypes.data, len(out), msg, 512):
        return msg.value.decode()
    return int(out[0]), [float(v) for v in out[2:2 + int(out[1])]]


def check_cv(label_frames, folds, scales):
    """host/Train.hpp check_train_cv for one feature with these labelled frames: "" or its message."""
    f = np.ascontiguousarray(label_frames, np.int32)
    s = np.ascontiguousarray(scales, np.float64)
    msg = C.create_string_buffer(512)
    rc = lib().thc_check_cv(f.ctypes.data, len(f), folds, s.ctypes.data, len(s), msg, 512)
    return msg.value.decode() if rc else ""


def folds(sample_frames, k):
    f = np.ascontiguousarray(sample_frames, np.int32)
    out = np.zeros(len(f), np.int32)
    lib().thc_folds(f.ctypes.data, len(f), k, out.ctypes.data)
    return out


def select(scales, rows):
    """(index of the chosen row, scores); rows [(n_pos, n_neg, miss_pos, miss_neg)]."""
    s = np.ascontiguousarray(scales, np.float64)
    r = np.ascontiguousarray(rows, np.int64).reshape(-1, 4)
    sc = np.zeros(len(s))
    return int(lib().thc_select(s.ctypes.data, r.ctypes.data, len(s), sc.ctypes.data)), sc


def host_objective(P, y, group, c_pos, c_neg, held_out, wb):
    buf, pitch = TH.padded(P)
    n, d = P.shape
    y = np.ascontiguousarray(y, np.int8)
    group = np.ascontiguousarray(group, np.uint8)
    wb = np.ascontiguousarray(wb, np.float64)
    z, a, g = np.zeros(n), np.zeros(n), np.zeros(d + 1)
    F = C.c_double()
    na = lib().thc_objective(buf.ctypes.data, pitch, y.ctypes.data, group.ctypes.data, n, d, c_pos, c_neg, held_out,
                             wb.ctypes.data, z.ctypes.data, a.ctypes.data, C.byref(F), g.ctypes.data)
    return F.value, g, z, a, na


def host_linesearch(y, group, z, xd, c_pos, c_neg, held_out, wd, dd, gd):
    y = np.ascontiguousarray(y, np.int8)
    group = np.ascontiguousarray(group, np.uint8)
    z = np.ascontiguousarray(z, np.float64)
    xd = np.ascontiguousarray(xd, np.float64)
    dF = C.c_double()
    k = lib().thc_linesearch(y.ctypes.data, group.ctypes.data, z.ctypes.data, xd.ctypes.data, len(y), c_pos, c_neg,
                             held_out, wd, dd, gd, C.byref(dF))
    return k, dF.value


# ---- the restatements

def ref_folds(sample_frames, k):
    """Frame rank r of the sorted distinct frames is fold r mod k; a sample takes its frame's fold."""
    rank = {f: r for r, f in enumerate(sorted(set(int(f) for f in sample_frames)))}
    return np.array([rank[int(f)] % k for f in sample_frames], np.int32)


def ref_score(row):
    """The balanced error as an exact fraction; a class without samples leaves its term out."""
    n_pos, n_neg, miss_pos, miss_neg = map(int, row)
    s = Fraction(0)
    if n_pos:
        s += Fraction(miss_pos, n_pos)
    if n_neg:
        s += Fraction(miss_neg, n_neg)
    return s / 2


def ref_select(scales, rows):
    """The smallest score wins; a tie goes to the smaller scale."""
    return min(range(len(scales)), key=lambda k: (ref_score(rows[k]), scales[k]))


def pooled(held, n_scales):
    """Rows per scale from the held-out dicts of problems listed fold by fold, the scales in turn."""
    rows = np.zeros((n_scales, 4), np.int64)
    for q, h in enumerate(held):
        rows[q % n_scales] += (h["n_pos"], h["n_neg"], h["miss_pos"], h["miss_neg"])
    return rows


# ---- the problems of the company tests (tests/test_gpu_train_cv.py; their sets are checked on the CPU in
# tests/test_train_cv.py): "overlapping" sets with groups i mod 5, costs (1, 1) times a scale
COMPANY_CASES = (((5, 7), 200), ((24, 24), 300))
POOL = ((0.01, -1), (0.01, 0), (0.1, 1), (0.3, 2), (1.0, -1), (1.0, 3), (3.0, 4), (10.0, 0), (30.0, 1), (100.0, 2),
        (100.0, -1), (100.0, 4))  # (scale, held_out)


def company_groups(n):
    return (np.arange(n) % 5).astype(np.int32)


def company_lists(pb):
    """Problem lists of length 1, 2, PB - 1, PB, PB + 1 and 2 PB + 1 over POOL, one problem twice in a list."""
    out, off = [], 0
    for n in sorted({1, 2, max(pb - 1, 1), pb, pb + 1, 2 * pb + 1}):
        lst = [POOL[(off + i) % len(POOL)] for i in range(max(n - 1, 1))]
        if n >= 2:
            lst.append(lst[0])
        off += max(n - 1, 1)
        out.append(lst)
    return out
