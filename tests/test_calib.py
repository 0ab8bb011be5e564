"""The calibration estimate (include/locomouse_calib.h), the parts that run
without a GPU: the header and the exported names, NULL and bad arguments, the
host record of csrc/lm_calib_core.h against the numpy restatement, lm_calib_fit
and lm_calib_map against the restatement in Python floats (bit for bit), the
refusals, the linear continuation, the yml writer, the LM_CALIB parser, the
program's error paths, a stand-alone sanitizer run of the core against a
brute-force statement, and the conditions the end-to-end GPU test rests on."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import calib_harness as CH  # noqa: E402

from locomouse_cpp_amd import abi, runtime  # noqa: E402

HDR = os.path.join(runtime.ROOT, "include", "locomouse_calib.h")


def declared_functions(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"^[A-Za-z_][\w\s\*]*?\b(lm_\w+)\s*\(", text, flags=re.M)))


def test_header_and_exports():
    assert set(declared_functions(HDR)) == set(runtime.CALIB_EXPORTED)
    assert len(set(runtime.CALIB_EXPORTED)) == len(runtime.CALIB_EXPORTED)
    L = runtime.lib()
    for sym in runtime.CALIB_EXPORTED:
        assert getattr(L, sym) is not None
    for other in (runtime.EXPORTED, runtime.JPEG_EXPORTED, runtime.BKG_EXPORTED, runtime.ENC_EXPORTED, runtime.TRAIN_EXPORTED):
        assert not set(runtime.CALIB_EXPORTED) & set(other)
    assert L.lm_abi_version() == 6
    text = open(HDR).read()
    for name in ("LM_CALIB_MAX_RADIUS", "LM_CALIB_MAX_DEGREE"):
        m = re.search(rf"^#define {name} (\d+)\b", text, flags=re.M)
        assert m and int(m.group(1)) == getattr(abi, name)
    assert re.search(r"^#define LM_CALIB_MAX_FRAMES \(1 << 20\)", text, flags=re.M) and abi.LM_CALIB_MAX_FRAMES == 1 << 20
    assert C.sizeof(abi.lm_calib_record) == 48 == CH.RECORD_DTYPE.itemsize == abi.CALIB_RECORD_DTYPE.itemsize
    assert C.sizeof(abi.lm_calib_opts) == 24 and C.sizeof(abi.lm_calib_fit_result) == 80
    assert "lm_calib.hip" in runtime.HIP_UNITS
    o = runtime.calib_opts()
    assert {k: getattr(o, k) for k in CH.DEFAULTS} == CH.DEFAULTS


def test_null_and_bad_arguments_without_gpu():
    L = runtime.lib()
    E = abi.LM_ERR_INVALID_ARGUMENT
    assert L.lm_calib_create(0, 8, 8, 4, 4, None, None) == E
    assert b"out is NULL" in L.lm_last_error()
    h = C.c_void_p()
    for rows, cols, split, max_batch in ((0, 8, 1, 4), (8, 0, 4, 4), (8, 8, 0, 4), (8, 8, 8, 4), (8, 8, -1, 4), (8, 8, 4, 0),
                                         (8, 8, 4, 65536), (65535, 65535, 4, 4), (70000, 8, 4, 4)):
        assert L.lm_calib_create(0, rows, cols, split, max_batch, None, C.byref(h)) == E and not h.value, (rows, cols, split)
    assert b"2^31" in L.lm_last_error() or b"65535" in L.lm_last_error()
    for bad in (dict(threshold=256), dict(threshold=-1), dict(radius=-1), dict(radius=abi.LM_CALIB_MAX_RADIUS + 1),
                dict(min_peak=256), dict(min_area=0), dict(max_stray=-1)):
        assert L.lm_calib_create(0, 8, 8, 4, 4, C.byref(runtime.calib_opts(**bad)), C.byref(h)) == E and not h.value, bad
        assert next(iter(bad)).encode() in L.lm_last_error()
    buf = np.zeros(64, np.uint8)
    assert L.lm_calib_set_background(None, buf.ctypes.data) == E
    assert L.lm_calib_push(None, buf.ctypes.data, 64, 1) == E
    assert L.lm_calib_push_device(None, None, 64, 1) == E
    assert L.lm_calib_read(None, 0, 1, buf.ctypes.data) == E
    assert L.lm_calib_reset(None) == E
    assert L.lm_calib_frames(None) == -1
    assert L.lm_calib_stream(None) is None
    L.lm_calib_destroy(None)
    L.lm_calib_default_opts(None)
    rec = np.zeros((40, 2), abi.CALIB_RECORD_DTYPE)
    res = abi.lm_calib_fit_result()
    fit = (rec.ctypes.data, 40, 16, 64, 5, None, 2, 1.5, C.byref(res))
    assert L.lm_calib_fit(None, *fit[1:]) == E and L.lm_calib_fit(*fit[:8], None) == E
    for k, v, word in ((1, -1, b"n_frames"), (2, 0, b"rows"), (4, 16, b"split_row"), (6, 0, b"degree"), (6, 4, b"degree"),
                       (7, 0.0, b"max_resid"), (7, float("nan"), b"max_resid")):
        a = list(fit)
        a[k] = v
        assert L.lm_calib_fit(*a) == E and word in L.lm_last_error(), (k, v, L.lm_last_error())
    assert L.lm_calib_fit(*fit[:5], C.byref(runtime.calib_opts(min_area=0)), *fit[6:]) == E
    m = np.zeros((16, 64), np.int32)
    boxes = np.zeros(8, np.int32)
    good = runtime.calib_fit(CH.records_of_points([(x, x) for x in np.linspace(5, 60, 30)]), 16, 64, 5)["raw"]
    assert L.lm_calib_map(None, 16, 64, 5, m.ctypes.data, boxes.ctypes.data) == E
    assert L.lm_calib_map(C.byref(good), 16, 64, 5, None, boxes.ctypes.data) == E
    assert L.lm_calib_map(C.byref(good), 16, 64, 5, m.ctypes.data, None) == E
    assert L.lm_calib_map(C.byref(good), 16, 64, 16, m.ctypes.data, boxes.ctypes.data) == E
    assert L.lm_calib_map(C.byref(abi.lm_calib_fit_result()), 16, 64, 5, m.ctypes.data, boxes.ctypes.data) == E  # degree 0
    assert L.lm_calib_map(C.byref(good), 16, 64, 5, m.ctypes.data, boxes.ctypes.data) == abi.LM_OK


@pytest.mark.parametrize("dark_bkg", [False, True], ids=["bkg", "zero_bkg"])
@pytest.mark.parametrize("shape", CH.RECORD_SHAPES, ids=[s[0] for s in CH.RECORD_SHAPES])
def test_host_record_equals_the_restatement(shape, dark_bkg):
    name, rows, cols, split, radius = shape
    frames, bkg = CH.record_scene(rows, cols, split, dark_bkg)
    o = CH.opts_of(radius=radius)
    want = CH.ref_records(frames, bkg, split, o)
    for pad in (0, 3):
        buf, pitch = CH.padded(frames, pad)
        CH.assert_records_equal(CH.host_records(buf, pitch, len(frames), bkg, rows, cols, split, o), want, (name, pad))
    # the scenes hold what they are meant to: clipped windows, an empty view, a tie
    assert want["clipped"].all() if radius == 100 else want["clipped"].any() == (radius > 0)
    assert (want["peak"][1] == 0).all() and (want["px"][1] == 0).all() and (want["py"][1] == [0, split]).all()
    assert (want["peak"][4] == 150).all() and want["py"][4, 1] == split


def sweep_points(n=60, cols=1024, outliers=(), gaps=()):
    """(xb, xs) of a marker swept over the middle 70 % of the width through a mildly curved warp."""
    pts = []
    for f in range(n):
        xb = 0.15 * cols + 0.7 * cols * f / (n - 1)
        t = (xb - cols / 2) / (cols / 2)
        xs = 0.5 * cols + 0.55 * cols * t + 9.0 * t * t - 4.0 * t ** 3 + 0.3 * np.sin(1.7 * f)
        if f in outliers:
            xs += 6.0 if f % 2 else -6.0
        pts.append(None if f in gaps else (xb, xs))
    return pts


@pytest.mark.parametrize("degree", [1, 2, 3])
def test_fit_and_map_equal_the_restatement_bit_for_bit(degree):
    rows, cols, split = 12, 1024, 5
    o = CH.DEFAULTS
    rec = CH.records_of_points(sweep_points(outliers=(20, 33), gaps=(3, 40)))
    rec["clipped"][10, 0] = 1                    # the side view's window clipped
    rec["peak"][11, 1] = o["min_peak"] - 1       # too faint in the bottom view
    rec["n_in"][12, 0] = rec["n_above"][12, 0] = o["min_area"] - 1  # too small
    rec["n_above"][13, 1] += o["max_stray"] + 1  # something else is bright in the view
    rec["n_above"][14, 1] += o["max_stray"]      # at the limit: still a sample
    want = CH.ref_fit(rec, cols, o, degree)
    got = runtime.calib_fit(rec, rows, cols, split, degree=degree)
    assert want["n_frames"] == 60 and want["n_samples"] == 60 - 2 - 4
    assert want["n_used"] <= want["n_samples"] - 2 and (degree < 3 or want["n_used"] == want["n_samples"] - 2)
    for k in ("n_frames", "n_samples", "n_used", "degree", "rms", "max_abs_resid", "lo", "hi", "coef"):
        assert got[k] == want[k], (k, got[k], want[k])  # floats included: equal to the bit
    assert 0 < want["rms"] <= want["max_abs_resid"]
    m, boxes = runtime.calib_map(got, rows, cols, split)
    wm, wboxes = CH.ref_map(want, rows, cols, split)
    assert np.array_equal(m, wm) and np.array_equal(boxes, wboxes)
    assert boxes.tolist() == [[0, 0, cols, split], [0, split, cols, rows - split]]
    assert np.array_equal(m[split:], np.arange(rows * cols, dtype=np.int32).reshape(rows, cols)[split:])
    assert (np.diff(m[0]) >= 0).all() and all(np.array_equal(m[r] - r * cols, m[0]) for r in range(split))


def _refused(rec, rows, cols, split, **kw):
    with pytest.raises(runtime.LMError) as e:
        fit = runtime.calib_fit(rec, rows, cols, split, **kw)
        runtime.calib_map(fit, rows, cols, split)
    assert e.value.code == abi.LM_ERR_RUNTIME
    return str(e.value)


def test_refusals_name_the_count_or_the_range():
    rows, cols, split = 12, 1024, 5
    o = CH.DEFAULTS
    few = CH.records_of_points(sweep_points(n=23))           # degree 2 needs 24
    with pytest.raises(CH.Refusal) as r:
        CH.ref_fit(few, cols, o, 2)
    assert r.value.kind == "count"
    msg = _refused(few, rows, cols, split)
    assert "23 samples of 23 frames" in msg and "at least 24" in msg, msg
    assert runtime.calib_fit(few, rows, cols, split, degree=1)["n_samples"] == 23  # degree 1 needs 16 only
    dropped = CH.records_of_points(sweep_points(n=24, outliers=(11,)))  # 24 samples, 23 after the outlier is dropped
    with pytest.raises(CH.Refusal) as r:
        CH.ref_fit(dropped, cols, o, 2)
    assert r.value.kind == "count" and int(str(r.value).split()[0]) < 24
    assert f"{str(r.value).split()[0]} samples of 24 frames" in _refused(dropped, rows, cols, split)
    none = np.zeros((50, 2), abi.CALIB_RECORD_DTYPE)
    assert "0 samples of 50 frames" in _refused(none, rows, cols, split)
    assert "0 samples of 0 frames" in _refused(none[:0], rows, cols, split)
    narrow = CH.records_of_points([(400 + 250 * f / 39, 380 + 270 * f / 39) for f in range(40)])  # spans 250 < 1024 / 4
    with pytest.raises(CH.Refusal) as r:
        CH.ref_fit(narrow, cols, o, 2)
    assert r.value.kind == "range"
    msg = _refused(narrow, rows, cols, split)
    sm = CH.ref_samples(narrow, o)
    assert f"{sm[0][1]:.6f} to {sm[-1][1]:.6f}" in msg and "256.0" in msg, msg
    wide = CH.records_of_points([(400 + 257 * f / 39, 380 + 270 * f / 39) for f in range(40)])
    assert runtime.calib_fit(wide, rows, cols, split)["n_used"] == 40
    falling = CH.records_of_points([(100 + 20 * f, 900 - 20 * f) for f in range(40)])  # a mirrored view: a fine fit, no map
    fit = CH.ref_fit(falling, cols, o, 2)
    with pytest.raises(CH.Refusal) as r:
        CH.ref_columns(fit, cols)
    assert r.value.kind == "monotone"
    msg = _refused(falling, rows, cols, split)
    assert "not non-decreasing" in msg and str(r.value) in msg, (msg, str(r.value))


def test_linear_continuation_outside_the_covered_range():
    rows, cols, split = 4, 1024, 2
    half = cols / 2
    pts = []
    for f in range(60):  # covers 300 .. 700 only, with a curvature the ends would show
        xb = 300 + 400 * f / 59
        t = (xb - half) / half
        pts.append((xb, 500 + 470 * t + 60 * t * t))
    fit = runtime.calib_fit(CH.records_of_points(pts), rows, cols, split, degree=2)
    m = runtime.calib_map(fit, rows, cols, split)[0][0].astype(np.int64)
    c = np.arange(cols, dtype=np.float64)
    poly = np.polynomial.polynomial.Polynomial(fit["coef"])
    p = poly((c - half) / half)
    dp = poly.deriv()
    lo, hi = fit["lo"], fit["hi"]
    inside = (c >= lo) & (c <= hi)
    assert np.array_equal(m[inside], np.floor(p[inside] + 0.5).astype(np.int64))
    for end, side in ((lo, c < lo), (hi, c > hi)):
        line = poly((end - half) / half) + dp((end - half) / half) / half * (c[side] - end)
        want = np.clip(np.floor(line + 0.5), 0, cols - 1).astype(np.int64)
        assert np.abs(m[side] - want).max() <= 1 and (m[side] == want).mean() > 0.99  # (numpy's rounding, not the core's)
        assert np.abs(np.floor(p[side] + 0.5) - m[side]).max() >= 5  # the polynomial itself runs away from it
    assert np.array_equal(m, np.array(CH.ref_columns(CH.ref_fit(CH.records_of_points(pts), cols, CH.DEFAULTS, 2), cols)))


def _load_cv_yaml(path):
    """An independent reader for the FileStorage YAML (PyYAML, safe loader with a constructor for !!opencv-matrix)."""
    import yaml

    class Loader(yaml.SafeLoader):
        pass

    def mat(loader, node):
        m = loader.construct_mapping(node, deep=True)
        return np.array(m["data"]).reshape(m["rows"], m["cols"]), m["dt"]

    Loader.add_constructor("tag:yaml.org,2002:opencv-matrix", mat)
    text = open(path).read().replace("%YAML:1.0", "", 1)
    return yaml.load(text, Loader=Loader)


def _fs_matrix(path, key):
    """(dt, matrix) read with the project's FileStorage reader (tests/cpp/host_harness.cpp)."""
    import host_harness as H
    kind, rows, cols = C.c_int(), C.c_int(), C.c_int()
    dt = C.c_char()
    out = np.zeros(1 << 16)
    text = C.create_string_buffer(256)
    rc = H.lib().lmh_fs_node(os.fsencode(path), key.encode(), C.byref(kind), C.byref(rows), C.byref(cols), C.byref(dt),
                             out.ctypes.data, out.size, text, 256)
    assert rc == 0 and kind.value == 6, (key, rc, text.value)
    return dt.value.decode(), out[:rows.value * cols.value].reshape(rows.value, cols.value)


def test_yaml_round_trip(tmp_path):
    rows, cols, split = 6, 200, 2
    pts = [(20 + 160 * f / 39, 30 + 150 * f / 39 + 0.2 * np.cos(f)) for f in range(40)]
    rec = CH.records_of_points(pts, cols=cols)
    fit = runtime.calib_fit(rec, rows, cols, split, degree=3)
    m, boxes = runtime.calib_map(fit, rows, cols, split)
    samples = np.array(CH.ref_samples(rec, CH.DEFAULTS))
    path = str(tmp_path / "calibration.yml")
    assert CH.write_yaml(path, fit["raw"], m, boxes, samples, split) is None
    assert open(path).read().startswith("%YAML:1.0")
    want = {"ind_warp_mapping": ("i", m), "view_boxes": ("i", boxes), "warp_coefficients": ("d", np.array([fit["coef"]])),
            "warp_range": ("d", np.array([[fit["lo"], fit["hi"]]])),
            "warp_residuals": ("d", np.array([[fit["rms"], fit["max_abs_resid"]]])),
            "warp_counts": ("i", np.array([[40, 40, fit["n_used"]]])), "warp_samples": ("d", samples)}
    doc = _load_cv_yaml(path)
    assert list(doc) == list(want)
    for key, (dt, a) in want.items():
        assert doc[key][1] == dt and doc[key][0].shape == a.shape and np.array_equal(doc[key][0], a), key  # doubles to the bit
        fdt, fa = _fs_matrix(path, key)
        assert fdt == dt and fa.shape == a.shape and np.array_equal(fa, a), key
    msg = CH.write_yaml(str(tmp_path / "no_such_dir" / "c.yml"), fit["raw"], m, boxes, samples, split)
    assert msg and "Could not write the calibration file" in msg


def test_calibration_spec_parser():
    d = CH.DEFAULTS
    base = (d["threshold"], d["radius"], d["min_peak"], d["min_area"], d["max_stray"])
    assert CH.parse_spec("30") == ((30,) + base[1:], 1.5)
    assert CH.parse_spec("30:8") == ((30, 8) + base[2:], 1.5)
    assert CH.parse_spec("30:8:100:20:0") == ((30, 8, 100, 20, 0), 1.5)
    assert CH.parse_spec("30:8:100:20:0:0.75") == ((30, 8, 100, 20, 0), 0.75)
    assert CH.parse_spec("0:0:0:1:0:2") == ((0, 0, 0, 1, 0), 2.0)
    for bad in ("", ":", "30:", "x", "30:-1", "1.5", "256", "30:8:100:0", "30:8:100:20:0:0", "30:8:100:20:0:-1",
                "30:8:100:20:0:abc", "30:8:100:20:0:1.5:7", "30:8:100:20:0:", "30:5000", "30:8:100:20:0:nan"):
        m = CH.parse_spec(bad)
        assert isinstance(m, str) and m.startswith("LM_CALIB: "), (bad, m)


def test_estimate_calibration_checks_come_before_any_frame_is_read():
    assert "no frames" in CH.refusal(0, 16, 64, 5)
    assert "split_row" in CH.refusal(10, 16, 64, 16) and "split_row" in CH.refusal(10, 16, 64, 0)
    assert "degree" in CH.refusal(10, 16, 64, 5, degree=4)
    assert "no size" in CH.refusal(10, 0, 64, 5)
    m = CH.refusal(abi.LM_CALIB_MAX_FRAMES + 1, 16, 64, 5)
    assert str(abi.LM_CALIB_MAX_FRAMES) in m and "exceed" in m, m


def _run(cmd, env=None, timeout=120):
    e = dict(os.environ)
    e.update(env or {})
    p = subprocess.run(cmd, capture_output=True, text=True, env=e, timeout=timeout)
    return p.returncode, p.stdout


def test_calibrate_program_errors(tmp_path):
    import media_writers as MW
    exe = runtime.CALIB_CLI_PATH
    usage = "Usage: LocoMouseCalibrate video.avi out.yml split_row [degree]"
    for args in ([], ["only.avi"], ["a.avi", "b.yml"], ["a.avi", "b.yml", "96", "2", "extra"], ["a.avi", "b.yml", "0"],
                 ["a.avi", "b.yml", "x"], ["a.avi", "b.yml", "96", "0"], ["a.avi", "b.yml", "96", "4"], ["a.avi", "b.yml", "-3"]):
        rc, out = _run([exe, *args])
        assert rc == 1 and out.startswith(usage), (args, out)
    missing = str(tmp_path / "none.avi")
    out_yml = tmp_path / "out.yml"
    rc, out = _run([exe, missing, str(out_yml), "96"])
    assert rc == 1 and f"Could not open the video file: {missing}." in out, out
    rc, out = _run([exe, missing, str(out_yml), "96"], env={"LM_CALIB": "40:x"})
    assert rc == 1 and out.startswith("Runtime Error: LM_CALIB: radius"), out
    video = str(tmp_path / "v.avi")
    MW.write_avi(video, np.zeros((3, 16, 64), np.uint8), bits=8)
    rc, out = _run([exe, video, str(out_yml), "16"])  # split_row must lie inside the frame
    assert rc == 1 and out.startswith("Runtime Error: ") and "split_row" in out, out
    rc, out = _run([exe, video, str(out_yml), "5"], env={"LM_CALIB_BACKGROUND": str(tmp_path / "none.png")})
    assert rc == 1 and out.startswith("Runtime Error: Could not read the background image"), out
    MW.write_png(str(tmp_path / "small.png"), np.zeros((8, 64), np.uint8))
    rc, out = _run([exe, video, str(out_yml), "5"], env={"LM_CALIB_BACKGROUND": str(tmp_path / "small.png")})
    assert rc == 1 and "8 x 64" in out and "16 x 64" in out, out
    assert not out_yml.exists()


def test_core_is_clean_under_the_sanitizers(tmp_path):
    """A stand-alone program (tests/cpp/calib_core_check.cpp) built with -fsanitize=address,undefined runs
    csrc/lm_calib_core.h's record and fit on 400 random small cases against a brute-force statement; nothing is
    loaded into Python."""
    exe = tmp_path / "calib_core_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",  # the runtimes in the program
                           *CH.INCLUDES, "-o", str(exe), CH.CHECK_SRC])
    r = subprocess.run([str(exe), "400", "20261020"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "400 cases, 0 failures" in r.stdout, r.stdout


@pytest.mark.parametrize("degree", [1, 2])
def test_marker_video_conditions_of_the_end_to_end_test(degree):
    """What tests/test_gpu_calib.py's end-to-end test rests on, from the restatement alone: at least 90 % of the
    marker video's frames are samples, and the map undoes the camera, h[m[c]] == c, on the whole covered range,
    which contains the synthetic configuration's crop columns."""
    from locomouse_cpp_amd import synthetic as S
    video = CH.marker_video()
    bkg = np.sort(video, axis=0)[(500 * (len(video) - 1)) // 1000]  # the median the program estimates
    rec = CH.ref_records(video, bkg, CH.SPLIT, CH.DEFAULTS)
    fit = CH.ref_fit(rec, CH.COLS, CH.DEFAULTS, degree)
    assert fit["n_samples"] >= 0.9 * len(video) and fit["n_used"] >= 0.9 * len(video), fit
    m = np.array(CH.ref_columns(fit, CH.COLS))
    h = CH.camera_table()
    cov = CH.covered_columns(fit["lo"], fit["hi"])
    assert len(cov) >= 700 and np.array_equal(h[m[cov]], cov), (len(cov), int((h[m[cov]] != cov).sum()))
    p = S.SyntheticConfig().params
    for box in (p.bounding_box_side, p.bounding_box_bottom):
        assert fit["lo"] <= box.x and box.x + box.width <= fit["hi"]
    got = runtime.calib_fit(rec, CH.ROWS, CH.COLS, CH.SPLIT, degree=degree)
    assert got["coef"] == fit["coef"] and np.array_equal(runtime.calib_map(got, CH.ROWS, CH.COLS, CH.SPLIT)[0][0], m)
