"""numpy restatement of the reference's histogram matching, written from its
lines (LocoMouse_class.cpp: cropBoundingBox :1437-1443, histogramMatching
:3313-3387, computeNormalizedCDF :3389-3414), for tests/test_match.py and
tests/test_gpu_match.py.  Nothing here calls the library.

calcHist gives exact counts as float32 (exact below 2^24; the statement keeps
integers and converts once, as the project's definition does);
hist / (cols * rows) is a MatExpr scale: convertTo(hist, alpha = 1.0 / n)
evaluates float(h) * float(alpha) for CV_32F."""
import numpy as np

F = np.float32


def hist(image):
    """[256] int64 counts of a u8 array of any shape."""
    image = np.asarray(image)
    assert image.dtype == np.uint8
    return np.bincount(image.reshape(-1), minlength=256).astype(np.int64)


def cdf_of_hist(h, n):
    scale = F(1.0 / float(n))
    c = np.zeros(256, F)
    acc = F(F(h[0]) * scale)
    c[0] = acc
    for i in range(1, 256):
        acc = F(acc + F(F(h[i]) * scale))
        c[i] = acc
    return c


def cdf(image):
    image = np.asarray(image)
    return cdf_of_hist(hist(image), image.size)


def table(c, ref):
    """(T [256] uint8, entries decided by the second loop) -- :3351-3380."""
    c = np.asarray(c, F)
    ref = np.asarray(ref, F)
    T = np.zeros(256, np.uint8)
    cur, fallback = 0, 0
    for i in range(256):
        assigned = False
        for j in range(cur, 256):
            if ref[j] >= c[i]:
                T[i] = j
                cur = j
                assigned = True
                break
        if not assigned:
            min_diff = F(1)
            for j in range(cur, 256):
                d = F(c[i] - ref[j])
                if d < min_diff:
                    min_diff = d
                    cur = j
            T[i] = cur
            fallback += 1
    return T, fallback


def corrected(cfg, frame, method=0, adj=None):
    """I_UNPAD of one frame of a SyntheticConfig-like cfg: background
    subtraction, normalize(NORM_MINMAX) -> CV_8U (with the TM methods' table
    `adj` on top), the calibration gather and the flip."""
    su = cfg.setup
    f = np.asarray(frame, np.uint8).reshape(-1).astype(np.int32)
    b = cfg.background.reshape(-1).astype(np.int32)
    d = np.maximum(f - b, 0)
    mn, mx = float(d.min()), float(d.max())
    scale = 255.0 * (1.0 / (mx - mn) if mx - mn > 2.220446049250313e-16 else 0.0)
    shift = 0.0 - mn * scale
    p = np.arange(256)
    if abs(scale - 1.0) < 2.220446049250313e-16 and abs(shift) < 2.220446049250313e-16:
        lut = p.astype(np.int64)
    else:
        t = F(F(p.astype(F) * F(scale)) + F(shift))
        lut = np.clip(np.rint(t).astype(np.int64), 0, 255)
    if method != 0:
        lut = np.asarray(adj, np.int64)[lut]
    img = lut[d][cfg.calib.reshape(-1)].reshape(su.calib_rows, su.calib_cols).astype(np.uint8)
    return img[:, ::-1] if su.flip else img


def bottom_rect(cfg, geom, corner=None):
    """(y, x, h, w) of I_BOTTOM_MOUSE in I_UNPAD for the bottom-right corner
    (x, y bottom) -- the provided box's when None."""
    bb = cfg.params.bounding_box_bottom
    cx, cy = (bb.x + bb.width, bb.y + bb.height) if corner is None else (int(corner[0]), int(corner[1]))
    w, h = geom.bb_bottom_mouse.width, geom.bb_bottom_mouse.height
    return cy - h + 1, cx - w + 1, h, w
