"""Detector training (include/locomouse_train.h), the parts that run without
a GPU: the header and the exported names, NULL and bad arguments, the host
build of csrc/lm_train_core.h (the arithmetic the kernels run per sample)
against the numpy restatement in tests/train_ref.py, a stand-alone sanitizer
run of it, the restated solver itself, and the selection of mined negatives
(host/Train.hpp) against its numpy restatement on an oracle result."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import media_writers as MW  # noqa: E402
import train_harness as TH  # noqa: E402
import train_ref as R  # noqa: E402

from locomouse_cpp_amd import abi, runtime  # noqa: E402
from locomouse_cpp_amd import synthetic as S  # noqa: E402

HDR = os.path.join(runtime.ROOT, "include", "locomouse_train.h")

# (N, D): one sample, one tap, rows shorter and longer than the 16-byte padding, the paw detector's size
SHAPES = ((1, 1), (1, 35), (2, 16), (33, 17), (64, 576), (200, 35))


def declared_functions(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"^[A-Za-z_][\w\s\*]*?\b(lm_\w+)\s*\(", text, flags=re.M)))


def test_header_and_exports():
    assert set(declared_functions(HDR)) == set(runtime.TRAIN_EXPORTED)
    assert len(set(runtime.TRAIN_EXPORTED)) == len(runtime.TRAIN_EXPORTED)
    L = runtime.lib()
    for sym in runtime.TRAIN_EXPORTED:
        assert getattr(L, sym) is not None
    others = set(runtime.EXPORTED) | set(runtime.JPEG_EXPORTED) | set(runtime.BKG_EXPORTED) | set(runtime.ENC_EXPORTED)
    assert not set(runtime.TRAIN_EXPORTED) & others
    assert L.lm_abi_version() == 6
    text = open(HDR).read()
    assert int(re.search(r"^#define LM_TRAIN_MAX_SIDE (\d+)\b", text, flags=re.M).group(1)) == abi.LM_TRAIN_MAX_SIDE
    assert re.search(r"^#define LM_TRAIN_MAX_SAMPLES \(1 << 22\)", text, flags=re.M) and abi.LM_TRAIN_MAX_SAMPLES == 1 << 22
    assert "lm_train.hip" in runtime.HIP_UNITS


@pytest.mark.parametrize("name", ["lm_train_point", "lm_train_stats"])
def test_struct_layout_matches_header(tmp_path, name):
    src = tmp_path / "sz.c"
    src.write_text(f'#include <stdio.h>\n#include "locomouse_train.h"\nint main(void){{printf("%zu", sizeof({name}));}}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I" + os.path.dirname(HDR), str(src), "-o", str(exe)])
    assert int(subprocess.check_output([str(exe)])) == C.sizeof(getattr(abi, name))


def test_null_and_bad_arguments_without_gpu():
    L = runtime.lib()
    E = abi.LM_ERR_INVALID_ARGUMENT
    assert L.lm_train_create(0, 24, 24, 100, None) == E
    assert b"out is NULL" in L.lm_last_error()
    h = C.c_void_p()
    for kh, kw, ms in ((0, 24, 10), (24, 0, 10), (65, 24, 10), (24, 65, 10), (24, 24, 0), (24, 24, (1 << 22) + 1),
                       (-1, 24, 10)):
        assert L.lm_train_create(0, kh, kw, ms, C.byref(h)) == E and not h.value
    buf = np.zeros(64, np.float64)
    rho = C.c_double()
    assert L.lm_train_add_patches(None, buf.ctypes.data, buf.ctypes.data, 1) == E
    assert L.lm_train_gather(None, None, None, 64, 1, None, 0) == E
    assert L.lm_train_gather_device(None, None, None, 64, 1, None, 0) == E
    assert L.lm_train_samples(None, None, None) == E
    assert L.lm_train_reset(None) == E
    assert L.lm_train_patches(None, 0, 0, None, None) == E
    assert L.lm_train_solve(None, 1.0, 1.0, 1e-6, 10, buf.ctypes.data, C.byref(rho), None) == E
    assert L.lm_train_margins(None, buf.ctypes.data, 0.0, buf.ctypes.data) == E
    assert L.lm_train_stream(None) is None
    L.lm_train_destroy(None)


def test_shared_constants():
    L = TH.lib()
    assert [L.th_pitch(d) for d in (1, 15, 16, 17, 576, 4096)] == [16, 16, 16, 32, 576, 4096]
    assert L.th_ls_steps() == R.LS_STEPS and L.th_xt_block() == 1024


@pytest.mark.parametrize("kind", TH.KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_statement_equals_numpy(kind, shape):
    n, d = shape
    P, y = TH.sample_set(kind, n, d)
    cp, cn = TH.kind_costs(kind)
    Xt = R.xtilde(P)
    rng = np.random.default_rng(n * 31 + d)
    for scale in (0.0, 0.05, 3.0):  # every sample active; a mixed active set; most inactive or far off
        wb = scale * rng.standard_normal(d + 1)
        F, g, a, sF, sg = R.objective(Xt, y, cp, cn, wb)
        hF, hg, hz, ha, hna = TH.host_objective(P, y, cp, cn, wb)
        z = Xt @ wb
        az = np.abs(Xt) @ np.abs(wb)
        assert np.all(np.abs(hz - z) <= 2 * (d + 1) * 2.0 ** -53 * az + 1e-300)
        flip = (ha != a)  # the active set may differ only where a margin sits on the hinge
        assert np.all(np.abs(1 - y[flip] * z[flip]) <= 4 * (d + 1) * 2.0 ** -53 * (1 + az[flip]))
        assert abs(hF - F) <= sF
        assert np.all(np.abs(hg - g) <= sg)
        assert hna == np.count_nonzero(ha)
        v = rng.standard_normal(d + 1)
        Hv = R.hessvec(Xt, ha, v)
        bound = (n + d + 2) * 2.0 ** -52 * (np.abs(v) + 2 * (np.abs(Xt).T @ (ha * (np.abs(Xt) @ np.abs(v)))))
        assert np.all(np.abs(TH.host_hessvec(P, ha, v) - Hv) <= bound)
        # the line search along -g from the same margins: the same step, the same change of F
        dvec = -g
        xd = Xt @ dvec
        c = R.costs(y, cp, cn)
        args = (float(wb @ dvec), float(dvec @ dvec), float(g @ dvec))
        k, dF = R.linesearch(y, z, xd, c, *args)
        hk, hdF = TH.host_linesearch(y, z, xd, cp, cn, *args)
        if np.any(g):
            assert k >= 0
        terms = abs(args[0]) + args[1] + float(np.sum(c * (2 + np.abs(z) + np.abs(xd)) ** 2))
        assert hk == k or abs(dF - R.ARMIJO * 2.0 ** -k * args[2]) <= (n + 4) * 2.0 ** -52 * terms
        if hk == k:
            assert abs(hdF - dF) <= (n + 4) * 2.0 ** -52 * terms


def test_core_under_the_sanitizers(tmp_path):
    exe = tmp_path / "train_core_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",  # the runtimes in the program itself
                           *TH.INCLUDES, "-o", str(exe), TH.CHECK_SRC])
    r = subprocess.run([str(exe), "300"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "300 cases, 0 failures" in r.stdout


@pytest.mark.parametrize("kind", TH.KINDS)
def test_restated_solver_reaches_the_minimiser(kind):
    """The method itself, in numpy: it ends at eps, and scipy's L-BFGS-B lands
    within |grad F| of it, as strong convexity promises."""
    from scipy.optimize import minimize
    P, y = TH.sample_set(kind, 120, 35)
    cp, cn = TH.kind_costs(kind)
    w, b, st = R.solve(P, y, cp, cn, 1e-8)
    assert st["converged"] == 1 and st["outer_iters"] <= 40
    Xt = R.xtilde(P)
    wb = np.append(w, b)
    F, g, a, sF, sg = R.objective(Xt, y, cp, cn, wb)
    assert np.linalg.norm(g) <= 1e-8 * st["grad_norm0"] + np.linalg.norm(sg)
    res = minimize(lambda v: R.objective(Xt, y, cp, cn, v)[:2], np.zeros(len(wb)), jac=True, method="L-BFGS-B",
                   options={"ftol": 0.0, "gtol": 0.0, "maxiter": 20000, "maxfun": 100000, "maxcor": 30})
    gs = np.linalg.norm(R.objective(Xt, y, cp, cn, res.x)[1])
    assert np.linalg.norm(res.x - wb) <= gs + np.linalg.norm(g)


# ------------------------------------------------- host/Train.hpp, the program

def test_train_spec_parser():
    assert TH.parse_spec("10:1:1e-6:2:60") == (10.0, 1.0, 1e-6, 2, 60)
    assert TH.parse_spec("4") == (4.0, 1.0, 1e-6, 2, 60)  # trailing fields keep their defaults
    assert TH.parse_spec("4:0.5:1e-9:0:0") == (4.0, 0.5, 1e-9, 0, 0)
    for bad in ("", "x", "0", "-1", "1:0", "1:1:0", "1:1:nan", "1:1:inf", "1:1:1e-6:-1", "1:1:1e-6:2.5", "1:1:1e-6:2:x",
                "1:1:1e-6:2:60:7", "1:1:1e-6:101"):
        msg = TH.parse_spec(bad)
        assert isinstance(msg, str) and msg.startswith("LM_TRAIN: "), (bad, msg)


def paw_labels(cfg, frames):
    """[(frame, x, y)] of the synthetic scene's bottom-view paws (synth_frame's px, py)."""
    sc = S.scene(cfg.rows, cfg.cols)
    out = []
    for f in frames:
        cx = sc["cx0"] + S.tri(f, 50, 40)
        for k in range(4):
            out.append((f, cx + (-110, -40, 40, 110)[k] + S.tri(f + 5 * k, 20, 30), sc["bottom_cy"] + (58 if k & 1 else -58)))
    return out


def test_mined_selection_equals_numpy_on_an_oracle_result():
    from oracle import oracle as O
    cfg = S.SyntheticConfig()
    n = 6
    res = O.OracleRun(cfg, cfg.frames(0, n)).result
    box = cfg.params.bounding_box_bottom
    cands = []
    for f in range(n):  # list 0: paw_bottom; exportPointTracks' corner - width + 1 + x
        lo, hi = int(res["cand_offset"][4 * f]), int(res["cand_offset"][4 * f + 1])
        cands += [(f, box.x + 1 + int(x), box.y + 1 + int(y)) for x, y in zip(res["cand"]["x"][lo:hi], res["cand"]["y"][lo:hi])]
    assert len(cands) >= 4 * n
    labels = paw_labels(cfg, range(n))
    for r_neg in (1, 6, 40):
        seen = set()
        want = R.select_mined(cands, labels, r_neg, seen)
        got = TH.select_mined(cands, labels, r_neg)
        assert got == want
        assert TH.select_mined(cands + cands[:3], labels, r_neg, seen) == []  # a second round adds none
        taken_before = cands[:2]
        assert TH.select_mined(cands, labels, r_neg, taken_before) == [c for c in want if c not in taken_before]
    far = TH.select_mined(cands, labels, 6)
    assert far and all(max(abs(x - lx), abs(y - ly)) >= 6 for f, x, y in far for lf, lx, ly in labels if lf == f)
    assert len(TH.select_mined(cands, labels, 6)) < len(cands)  # the candidates on the paws are not negatives
    assert TH.select_mined(cands, [(99, 0, 0)], 1000) == list(dict.fromkeys(cands))  # labels of other frames do not count


def test_initial_negatives_equal_numpy():
    cfg = S.SyntheticConfig()
    vb = cfg.setup.view_box_bottom
    view = (vb.x, vb.y, vb.width, vb.height)
    for feature, frame, r_neg, k in ((0, 0, 6, 60), (1, 23, 7, 60), (3, 100000, 5, 7), (0, 5, 300, 20)):
        labels = paw_labels(cfg, [frame])
        got = TH.initial_negatives(feature, frame, labels, view, cfg.rows, cfg.cols, r_neg, k)
        assert got == R.initial_negatives(feature, frame, labels, view, cfg.rows, cfg.cols, r_neg, k)
        assert len(got) <= k and (len(got) == k or r_neg == 300)
        for f, x, y in got:
            assert f == frame and vb.x <= x < vb.x + vb.width and vb.y <= y < vb.y + vb.height
            assert all(max(abs(x - lx), abs(y - ly)) >= r_neg for _, lx, ly in labels)
    # keyed by feature and frame; a box that leaves the image is clipped; an empty one gives none
    a = TH.initial_negatives(0, 1, [], view, cfg.rows, cfg.cols, 6, 10)
    assert a != TH.initial_negatives(1, 1, [], view, cfg.rows, cfg.cols, 6, 10)
    assert a != [(1, x, y) for _, x, y in TH.initial_negatives(0, 2, [], view, cfg.rows, cfg.cols, 6, 10)]
    big = TH.initial_negatives(0, 1, [], (-50, 200, 2000, 500), cfg.rows, cfg.cols, 6, 40)
    assert len(big) == 40 and all(0 <= x < cfg.cols and 200 <= y < cfg.rows for _, x, y in big)
    assert TH.initial_negatives(0, 1, [], (0, 300, 10, 10), cfg.rows, cfg.cols, 6, 10) == []


def test_model_file_round_trip(tmp_path):
    cfg = S.SyntheticConfig()
    w = {k: v.copy() for k, v in cfg.weights.items()}
    w["paw_bottom"][0, :4] = (-0.0, 3.0, 1e-310, -1.0 / 3.0)  # a signed zero, an integer, a denormal
    b = dict(cfg.biases, paw_bottom=-0.1, tail_side=7.0)
    p = str(tmp_path / "model.yml")
    TH.write_model(p, w, b)
    w2, b2 = TH.load_model(p)
    assert b2 == b
    for k in w:
        assert w2[k].shape == w[k].shape and np.array_equal(w2[k].view(np.uint64), w[k].view(np.uint64)), k
    text = open(p).read()
    keys = re.findall(r"^(\w+):", text, flags=re.M)
    assert keys == ["model" + s for s in ("Paw_side", "Paw_bottom", "Tail_side", "Tail_bottom", "Snout_side", "Snout_bottom")] \
        + ["bias" + s for s in ("Paw_side", "Paw_bottom", "Tail_side", "Tail_bottom", "Snout_side", "Snout_bottom")]
    # the writer of the test fixtures and this one describe the same model
    MW.write_model(str(tmp_path / "ref.yml"), cfg)
    w3, b3 = TH.load_model(str(tmp_path / "ref.yml"))
    assert b3 == cfg.biases and all(np.array_equal(w3[k], cfg.weights[k]) for k in w3)


def write_labels(path, labels_by_feature, dt="i"):
    text = "%YAML:1.0\n---\n"
    for name, pts in labels_by_feature.items():
        text += MW.yaml_matrix("labels_" + name, np.asarray(pts).reshape(-1, 3), dt)
    with open(path, "w") as fh:
        fh.write(text)


def run_train(args, env=None):
    e = {k: v for k, v in os.environ.items() if not k.startswith("LM_")}
    e.update(env or {})
    p = subprocess.run([runtime.TRAIN_CLI_PATH, *map(str, args)], capture_output=True, text=True, env=e, timeout=300)
    return p.returncode, p.stdout


def train_args(paths, labels, out, side="R"):
    return [paths["config"], paths["video"], paths["background"], paths["calibration"], side, labels, paths["model"], out]


def test_program_refuses_malformed_input_before_a_device_is_touched(tmp_path):
    cfg = S.SyntheticConfig(rows=128, cols=256, bounding_boxes={"side": (40, 3, 150, 40), "bottom": (40, 60, 150, 60)})
    paths = MW.write_inputs(str(tmp_path), cfg, 3)
    lab, out = str(tmp_path / "labels.yml"), str(tmp_path / "out.yml")
    good = {"paw_bottom": [(0, 100, 90), (2, 120, 95)]}
    write_labels(lab, good)
    env = {"HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1"}  # no device could be opened

    def refused(args, env_more=None, want=""):
        rc, text = run_train(args, dict(env, **(env_more or {})))
        assert rc == 1 and text.startswith("Invalid inputs: ") and want in text, text
        return text

    refused(train_args(paths, lab, out)[:7], want="Usage: LocoMouseTrain")
    refused(train_args(paths, lab, out) + ["paw_top"], want="Unknown feature: paw_top")
    refused(train_args(paths, lab, out) + ["snout_bottom"], want="labels_snout_bottom is empty or undefined")
    refused(train_args(paths, lab, out, side="X"), want="Mouse side option")
    refused(train_args(paths, str(tmp_path / "none.yml"), out), want="Could not open the labels file")
    refused(train_args(dict(paths, model=str(tmp_path / "none.yml")), lab, out), want="Could not open the model file")
    refused(train_args(dict(paths, video=str(tmp_path / "none.avi")), lab, out), want="Could not open the video file")
    refused(train_args(paths, lab, str(tmp_path / "no_dir" / "out.yml")), want="Could not create the model file")
    for spec in ("0", "1:1:1e-6:x", "1:1:1:1:1:1"):
        refused(train_args(paths, lab, out), {"LM_TRAIN": spec}, want="LM_TRAIN: ")
    refused(train_args(paths, lab, out), {"LM_METHOD": "3"}, want="LM_METHOD")
    refused(train_args(paths, lab, out), {"LM_BACKGROUND": "mean"}, want="LM_BACKGROUND")
    for bad, want in (([(3, 100, 90)], "frame 3 is outside the video's 3 frames"), ([(-1, 100, 90)], "frame -1"),
                      ([(0, 256, 90)], "outside the corrected image"), ([(0, 100, 128)], "outside the corrected image"),
                      ([(0, -1, 90)], "outside the corrected image")):
        write_labels(lab, {"paw_bottom": good["paw_bottom"] + bad})
        refused(train_args(paths, lab, out), want=want)
    write_labels(lab, {"paw_bottom": [(0.0, 100.0, 90.0)]}, dt="d")
    refused(train_args(paths, lab, out), want="must be an integer (dt: i) matrix")
    with open(lab, "w") as fh:
        fh.write("%YAML:1.0\n---\n" + MW.yaml_matrix("labels_paw_bottom", np.zeros((2, 2), np.int32), "i"))
    refused(train_args(paths, lab, out), want="n x 3 matrix")
    with open(lab, "w") as fh:
        fh.write("%YAML:1.0\n---\nother: 1\n")
    refused(train_args(paths, lab, out), want="no feature to train")
    write_labels(lab, good)
    os.makedirs(str(tmp_path / "g"))
    gpaths = MW.write_inputs(str(tmp_path / "g"), cfg, 3, config_overrides={"transform_gray_values": 1})
    text = run_train(train_args(gpaths, lab, out), env)[1]
    assert text.startswith("Invalid inputs: ") and ("transform_gray_values" in text or "gray level transformation" in text)
    assert not os.path.exists(out) or os.path.getsize(out) == 0
