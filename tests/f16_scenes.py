"""Scenes for the f16 correlation (k_corr_f16<NCH>, lm_corr.hip) at every
chunk count NCH = f16_nch(kw) = (kw + 46) // 16 = 2..10, detector heights 1..7,
output sizes on every residue of the 128 x 64 workgroup tile that gates a
wave, a 32 x 32 accumulator tile or a ballot word, windows above 64 KiB of LDS
and at the 160 KiB cap.  Shared by test_f16_scenes.py (CPU: the conditions on
the inputs that keep the GPU comparison from passing vacuously) and
test_gpu_f16_shapes.py (GPU: bit-exact against the oracle).

Why bit-exact: detector weights are n / 4096 with small integer n, exact in
f16 after the kernel's per-detector power-of-two scaling; pixels are u8; so
every partial sum is a multiple of 2^-12 and exact in fp32 in any order while
255 * sum|n| + |bias| * 4096 < 2^24 (`exactness_bound`).
"""
import functools
from dataclasses import dataclass

import numpy as np

from locomouse_cpp_amd import abi
from locomouse_cpp_amd import synthetic as S

ROWS, COLS = 256, 1024
TAILS = ("tail_bottom", "tail_side")
SIDE_BIAS0 = 512.0
RATE = 0.02  # point detectors: share of the zero-bias scores above the bias
DET_ID = {n: i for i, n in enumerate(abi.DETECTORS)}

# (x, y, width, height) of the provided boxes; the outputs of a view's point
# detectors are width x height (ow x oh), tail_sub_bounding_box = 1 gives the
# tail detectors the same
BOX_A = {"bottom": (300, 106, 161, 97), "side": (300, 3, 161, 90)}     # ow = 33 (mod 128); oh = 33, 26 (mod 64)
BOX_B = {"bottom": (300, 106, 225, 129), "side": (300, 3, 225, 65)}    # ow = 97 (mod 128); oh = 1 (mod 64)
BOX_FULL = {"bottom": (300, 106, 128, 64), "side": (300, 3, 128, 64)}  # exact multiples of the tile
BOX_HALF = {"bottom": (300, 106, 160, 96), "side": (300, 3, 160, 32)}  # a wave's second 32-tile / second wave row exactly off
BOX_65 = {"bottom": (300, 106, 193, 70), "side": (300, 3, 193, 40)}    # ow = 65 (mod 128): one column into the second wave
BOXES = {"A": BOX_A, "B": BOX_B, "FULL": BOX_FULL, "HALF": BOX_HALF, "65": BOX_65}
# (ow mod 128, bottom oh mod 64, side oh mod 64) each box set is meant to give
BOX_RESIDUES = {"A": (33, 33, 26), "B": (97, 1, 1), "FULL": (0, 0, 0), "HALF": (32, 32, 32), "65": (65, 6, 40)}


def nch_of(kw):
    return (kw + 46) // 16


def kw_range(nch):
    return max(1, 16 * nch - 46), 16 * nch - 31


def class_sizes(nch):
    """The six detectors (rows, cols) of one class: one launch group of six."""
    lo, hi = kw_range(nch)
    return {"paw_bottom": (5, hi), "snout_bottom": (7, lo), "tail_bottom": (4, max(1, hi - 1)), "paw_side": (2, hi),
            "snout_side": (1, lo), "tail_side": (3, (lo + hi) // 2)}


def mixed_sizes():
    """Six classes in one context (six launch groups): 3, 4, 6, 7, 9, 10."""
    return {"paw_bottom": (5, kw_range(10)[1]), "snout_bottom": (7, kw_range(7)[0]), "tail_bottom": (4, kw_range(4)[1]),
            "paw_side": (2, kw_range(9)[1]), "snout_side": (1, kw_range(3)[0]), "tail_side": (3, kw_range(6)[1] - 3)}


def tall_sizes(kh):
    """An NCH-10 case whose bottom point detectors are kh rows tall."""
    s = class_sizes(10)
    s["paw_bottom"] = (kh, 129)
    s["snout_bottom"] = (kh, 114)
    return s


@dataclass(frozen=True)
class Case:
    name: str
    sizes: tuple          # ((detector, (rows, cols)), ...)
    boxes: str            # name of the box set
    kind: str = "sweep"   # sweep | dense | tall
    n: int = 3            # frames compared
    flip: bool = False
    moving: bool = False  # per-frame corners (edge_scenes.moving_corners)
    seam: bool = False    # frames 1.. in batches of two after a halo frame
    seed: int = 0

    def size(self, name):
        return dict(self.sizes)[name]

    @property
    def classes(self):
        return sorted({nch_of(kw) for _, (_, kw) in self.sizes})


def _case(name, sizes, boxes, **kw):
    return Case(name=name, sizes=tuple(sorted(sizes.items())), boxes=boxes, **kw)


def _cases():
    out = []
    for nch in range(2, 11):
        out.append(_case(f"nch{nch}", class_sizes(nch), "A" if nch % 2 else "B", seed=nch))
    out.append(_case("mixed", mixed_sizes(), "A", seed=20))
    out.append(_case("ow128_oh64", class_sizes(8), "FULL", seed=21))
    out.append(_case("ow160_oh96", class_sizes(3), "HALF", seed=22))
    out.append(_case("ow193", class_sizes(6), "65", seed=23))
    out.append(_case("moving", class_sizes(9), "A", moving=True, seed=24))
    out.append(_case("flip", class_sizes(7), "A", flip=True, seed=25))
    out.append(_case("seam", class_sizes(8), "B", seam=True, n=5, seed=26))
    out.append(_case("dense_tail", class_sizes(5), "A", kind="dense", seed=27))
    out.append(_case("tall64", tall_sizes(64), "A", kind="tall", seed=28))
    out.append(_case("tall247", tall_sizes(247), "A", kind="tall", seed=29))
    return {c.name: c for c in out}


CASES = _cases()
SWEEP = [c.name for c in CASES.values() if c.kind == "sweep"]
TALL = [c.name for c in CASES.values() if c.kind == "tall"]


def quantized_detector(kh, kw, seed):
    """Integer numerators over 4096: -4..4, or -1..1 above 16,000 taps (the
    exactness bound)."""
    rng = np.random.default_rng(1000 + seed)
    hi = 1 if kh * kw > 16000 else 4
    n = rng.integers(-hi, hi + 1, size=(kh, kw))
    # a point detector of a few taps answers to brightness alone, and only pixels above 25 can be candidates: the
    # numerators' sum is positive
    if n.sum() < 0:
        n = -n
    if n.sum() == 0:
        n.flat[int(np.argmax(n.ravel() < hi))] += 1
    return n.astype(np.float64) / 4096.0


def noise_frames(background, n, seed):
    """The background plus half-density noise of 0..199, clipped to 255."""
    rng = np.random.default_rng(2000 + seed)
    on = rng.random((n,) + background.shape) < 0.5
    amp = rng.integers(0, 200, size=(n,) + background.shape)
    return np.minimum(background.astype(np.int32)[None] + np.where(on, amp, 0), 255).astype(np.uint8)


def exactness_bound(w, bias):
    """255 * sum|n_ij| + |bias| * 4096: below 2^24 every partial sum is exact in fp32."""
    n = np.abs(np.round(w * 4096.0)).sum()
    return 255.0 * n + abs(bias) * 4096.0


def _config(case, weights, biases):
    cfg = S.SyntheticConfig(rows=ROWS, cols=COLS, flip=case.flip, weights=weights, biases=biases,
                            bounding_boxes=BOXES[case.boxes])
    cfg.params.tail_sub_bounding_box = 1.0
    # matching's overlap is (int)(bottom detector columns * (1 - side_bottom_min_overlap)) pixels and divides the
    # side scores: 0 below four columns at the default 0.7 (the reference then asserts on a NaN score), so the
    # classes with narrower bottom detectors (NCH 2, 3) match with a minimum overlap of 0
    if min(weights[n].shape[1] for n in ("paw_bottom", "snout_bottom")) < 4:
        cfg.params.side_bottom_min_overlap = 0.0
    return cfg


@dataclass
class Scene:
    case: Case
    cfg: object
    frames: np.ndarray   # every frame the oracle ran (the seam case: the halo frame first)
    bb: object           # per-frame corners or None
    drop: int            # leading oracle frames that are not compared (the halo)
    ref: object          # oracle.OracleRun over `frames` (KEEP_DEBUG)

    @property
    def result(self):
        from locomouse_cpp_amd.results import slice_results
        return slice_results(self.ref.result, self.drop) if self.drop else self.ref.result


@functools.lru_cache(maxsize=None)
def scene(name):
    """The case's configuration, frames and oracle run (computed once per
    process, shared by every test, never modified)."""
    from oracle import oracle as O
    import edge_scenes as E
    case = CASES[name]
    W = {n: quantized_detector(kh, kw, 16 * case.seed + DET_ID[n]) for n, (kh, kw) in case.sizes}
    # the zero-bias score maps: the side point detectors run only after a non-empty bottom list, so the bottom
    # detectors get bias 0; the side point detectors get SIDE_BIAS0 (exact on the grid, added back below), which keeps
    # their half-positive maps out of the candidate stages
    c0 = _config(case, W, {n: (SIDE_BIAS0 if n in ("paw_side", "snout_side") else 0.0) for n in W})
    total = case.n + (1 if case.seam else 0)
    frames = noise_frames(c0.background, total, case.seed)
    bb = E.moving_corners(c0, total) if case.moving else None
    r0 = O.OracleRun(c0, frames[:1], bb=None if bb is None else bb[:1], flags=O.KEEP_DEBUG)
    biases = {}
    for n in W:
        v = np.sort(r0.scores(0, DET_ID[n]).ravel().astype(np.float64))
        if n in ("paw_side", "snout_side"):
            v += SIDE_BIAS0
        q = 0.5 if n in TAILS else 1.0 - RATE
        biases[n] = float(v[int(q * (len(v) - 1))])
    if case.kind == "dense":
        biases["tail_bottom"] = -1e6
    cfg = _config(case, W, biases)
    ref = O.OracleRun(cfg, frames, bb=bb, flags=O.KEEP_DEBUG)
    return Scene(case=case, cfg=cfg, frames=frames, bb=bb, drop=1 if case.seam else 0, ref=ref)


def f16(cfg):
    cfg.setup.corr_precision = abi.LM_CORR_F16
    return cfg


def gpu_config(sc):
    """A fresh LM_CORR_F16 configuration of the scene (the cached one stays as the oracle saw it)."""
    return f16(_config(sc.case, sc.cfg.weights, sc.cfg.biases))


def boundary_config(kh, kw):
    """A default scene whose paw_bottom is kh x kw (one non-zero tap)."""
    w = np.zeros((kh, kw))
    w[kh // 2, kw // 2] = 1.0 / 4096
    return f16(S.SyntheticConfig(rows=ROWS, cols=COLS, weights={"paw_bottom": w}))
