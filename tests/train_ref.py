"""numpy float64 restatement of the detector training (include/locomouse_train.h,
csrc/lm_train_core.h): the objective every layer is tested against, its
gradient with the fp64 rounding bound of that evaluation, the active-set
Hessian product, the line search, the truncated Newton solver, and the
selection of mined negatives (host/Train.hpp)."""
import numpy as np

LS_STEPS, ARMIJO, CG_TOL = 24, 1e-4, 1e-3
U = 2.0 ** -52


def xtilde(P):
    """[N, D + 1] float64: the patches / 255 and a column of ones."""
    P = np.asarray(P)
    X = P.reshape(P.shape[0], -1).astype(np.float64) / 255.0
    return np.hstack([X, np.ones((X.shape[0], 1))])


def costs(y, c_pos, c_neg):
    return np.where(np.asarray(y) > 0, float(c_pos), float(c_neg))


def objective(Xt, y, c_pos, c_neg, wb):
    """F, grad F, the active costs, and the rounding bounds of F and of each
    gradient entry: (N + D + 2) 2^-52 times the sum of the absolute values of
    the terms that make it up."""
    y = np.asarray(y, np.float64)
    n, d1 = Xt.shape
    z = Xt @ wb
    m = 1.0 - y * z
    a = np.where(m > 0, costs(y, c_pos, c_neg), 0.0)
    F = 0.5 * float(wb @ wb) + float(np.sum(a * m * m))
    t = a * (z - y)
    g = wb + 2.0 * (Xt.T @ t)
    # the terms, with every margin written out as the sum it is: z_i - y_i has
    # the terms w_k x_ik, b and -y_i, of absolute sum az_i + 1
    az = np.abs(Xt) @ np.abs(wb)
    k = (n + d1 + 1) * U
    sF = k * (0.5 * float(wb @ wb) + float(np.sum(a * (1.0 + az) ** 2)))
    sg = k * (np.abs(wb) + 2.0 * (np.abs(Xt).T @ (a * (az + 1.0))))
    return F, g, a, sF, sg


def hessvec(Xt, a, v):
    return v + 2.0 * (Xt.T @ (a * (Xt @ v)))


def ls_delta(y, z, xd, lam, c):
    m0 = np.maximum(1.0 - y * z, 0.0)
    m1 = np.maximum(1.0 - y * (z + lam * xd), 0.0)
    return c * ((m1 - m0) * (m1 + m0))


def linesearch(y, z, xd, c, wd, dd, gd):
    """(k, dF): the first lambda = 2^-k with F(wb + lambda d) - F(wb) <= ARMIJO lambda g.d, or (-1, 0)."""
    y = np.asarray(y, np.float64)
    lam = 1.0
    for k in range(LS_STEPS):
        dF = lam * wd + 0.5 * lam * lam * dd + float(np.sum(ls_delta(y, z, xd, lam, c)))
        if dF <= ARMIJO * lam * gd:
            return k, dF
        lam *= 0.5
    return -1, 0.0


def solve(P, y, c_pos, c_neg, eps, max_iter=100, cg_cap=None):
    """The truncated Newton method of lm_train_solve: (w, b, stats)."""
    Xt = xtilde(P)
    y = np.asarray(y, np.float64)
    c = costs(y, c_pos, c_neg)
    n, d1 = Xt.shape
    cg_cap = min(d1, 96) if cg_cap is None else cg_cap
    wb = np.zeros(d1)
    g0 = None
    cg_iters = 0
    it = 0
    while True:
        z = Xt @ wb
        F, g, a, _, _ = objective(Xt, y, c_pos, c_neg, wb)
        gn = float(np.linalg.norm(g))
        g0 = gn if g0 is None else g0
        conv = gn <= eps * g0
        if conv or it >= max_iter:
            break
        d = np.zeros(d1)
        r = -g
        p = r.copy()
        rr = float(r @ r)
        for _ in range(cg_cap):
            hp = hessvec(Xt, a, p)
            alpha = rr / float(p @ hp)
            d += alpha * p
            r -= alpha * hp
            rr1 = float(r @ r)
            cg_iters += 1
            p = r + (rr1 / rr) * p
            rr = rr1
            if not np.sqrt(rr) > CG_TOL * gn:
                break
        k, _ = linesearch(y, z, Xt @ d, c, float(wb @ d), float(d @ d), float(g @ d))
        if k < 0:
            break
        wb = wb + 2.0 ** -k * d
        it += 1
    return wb[:-1], wb[-1], {"objective": F, "grad_norm": gn, "grad_norm0": g0, "outer_iters": it,
                             "cg_iters": cg_iters, "converged": int(conv), "n_active": int(np.count_nonzero(a))}


def select_mined(cands, labels, r_neg, seen):
    """The mined negatives of one round (host/Train.hpp select_mined): cands
    [(frame, x, y)] in candidate order, labels [(frame, x, y)]; a candidate is
    taken when it is at Chebyshev distance >= r_neg from every label of its
    frame and (frame, x, y) is not in `seen`, which grows by what is taken."""
    out = []
    for f, x, y in cands:
        key = (int(f), int(x), int(y))
        if key in seen:
            continue
        if any(lf == f and max(abs(lx - x), abs(ly - y)) < r_neg for lf, lx, ly in labels):
            continue
        seen.add(key)
        out.append(key)
    return out


def initial_negatives(feature, frame, labels, view, rows, cols, r_neg, neg_per_frame):
    """host/Train.hpp initial_negatives: points of a splitmix64 sequence keyed
    by (feature, frame, index) inside the view box (x, y, width, height)
    clipped to the image, at Chebyshev distance >= r_neg from the frame's labels."""
    from locomouse_cpp_amd.synthetic import splitmix64
    x0, y0 = max(view[0], 0), max(view[1], 0)
    x1, y1 = min(view[0] + view[2], cols), min(view[1] + view[3], rows)
    out = []
    if x1 <= x0 or y1 <= y0:
        return out
    key = (feature << 56) ^ (frame << 24)
    for k in range(64 * neg_per_frame):
        if len(out) >= neg_per_frame:
            break
        h = int(splitmix64(np.uint64(key ^ k)))
        x, y = x0 + h % (x1 - x0), y0 + int(splitmix64(np.uint64(h))) % (y1 - y0)
        if any(lf == frame and max(abs(lx - x), abs(ly - y)) < r_neg for lf, lx, ly in labels):
            continue
        out.append((frame, x, y))
    return out
