"""The calibration estimate on the GPU (include/locomouse_calib.h,
csrc/lm_calib.hip): every record is compared exactly with the numpy restatement
of the definition (tests/calib_harness.py), and the program is run end to end:
a marker video seen through a camera that stretches the side view, the
estimated calibration.yml, and LocoMouse's tracks with it against its tracks
with a map built directly from the camera's table."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import calib_harness as CH  # noqa: E402
import media_writers as MW  # noqa: E402

from locomouse_cpp_amd import abi, runtime  # noqa: E402
from locomouse_cpp_amd import synthetic as S  # noqa: E402

pytestmark = pytest.mark.gpu


def push_all(cal, buf, pitch, sizes):
    """The frames of `buf`, `pitch` bytes apart, in pushes of the given sizes (lm_calib_push)."""
    s = 0
    for n in sizes:
        rc = runtime.lib().lm_calib_push(cal._h, buf[s * pitch:].ctypes.data, pitch, n)
        assert rc == abi.LM_OK, runtime.lib().lm_last_error()
        s += n


@pytest.mark.parametrize("pad", [0, 3, 4])
@pytest.mark.parametrize("shape", CH.RECORD_SHAPES, ids=[s[0] for s in CH.RECORD_SHAPES])
def test_records_equal_the_restatement(shape, pad):
    """All-dark and darker-than-background views, a saturated frame, two equal peaks, the peak at each corner,
    d == threshold, R larger than the view and R = 0, at tight, unaligned and aligned pitch, in pushes of 1,
    max_batch and an uneven remainder; without a background (all zero) and with one."""
    name, rows, cols, split, radius = shape
    o = CH.opts_of(radius=radius)
    for dark_bkg in (True, False):
        frames, bkg = CH.record_scene(rows, cols, split, dark_bkg)
        k = len(frames)
        assert k == 13
        buf, pitch = CH.padded(frames, pad)
        cal = runtime.Calibrator(rows, cols, split, max_batch=5, opts=runtime.calib_opts(**o))
        if not dark_bkg:
            cal.set_background(bkg)
        push_all(cal, buf, pitch, [1, 5, 5, 2])
        assert cal.frames == k
        want = CH.ref_records(frames, bkg, split, o)
        CH.assert_records_equal(cal.records(), want, (name, pad, dark_bkg))
        CH.assert_records_equal(cal.records(3, 7), want[3:10], (name, "part"))
        if dark_bkg:
            sat = want[3]  # d = 255 everywhere
            assert (sat["peak"] == 255).all() and (sat["px"] == 0).all() and sat["S"][1] == 255 * sat["n_in"][1]
        cal.close()


def test_one_frame_at_256x1024():
    rows, cols, split = CH.ROWS, CH.COLS, CH.SPLIT
    video = CH.marker_video()
    bkg = np.full((rows, cols), 16, np.uint8)
    cal = runtime.Calibrator(rows, cols, split, max_batch=1)
    cal.set_background(bkg)
    cal.push(video[57:58])
    want = CH.ref_records(video[57:58], bkg, split, CH.DEFAULTS)
    CH.assert_records_equal(cal.records(), want)
    assert (want["peak"] > 150).all() and (want["clipped"] == 0).all() and (want["n_in"] > 60).all()
    cal.close()
    # saturated, the window the whole view: the sums pass 2^32
    o = CH.opts_of(radius=abi.LM_CALIB_MAX_RADIUS)
    cal = runtime.Calibrator(rows, cols, split, max_batch=1, opts=runtime.calib_opts(**o))
    full = np.full((1, rows, cols), 255, np.uint8)
    cal.push(full)
    got = cal.records()
    CH.assert_records_equal(got, CH.ref_records(full, np.zeros((rows, cols), np.uint8), split, o))
    assert got["Sx"][0, 1] == 255 * (rows - split) * (cols * (cols - 1) // 2) > 1 << 32
    assert got["n_in"][0].tolist() == [split * cols, (rows - split) * cols] == got["n_above"][0].tolist()
    cal.close()


def test_push_device_equals_push():
    import torch
    rows, cols, split = 16, 130, 5
    frames, bkg = CH.record_scene(rows, cols, split, False)
    k = len(frames)
    o = CH.opts_of(radius=3)
    host = runtime.Calibrator(rows, cols, split, max_batch=k, opts=runtime.calib_opts(**o))
    host.set_background(bkg)
    host.push(frames)
    want = CH.ref_records(frames, bkg, split, o)
    CH.assert_records_equal(host.records(), want)
    for pad in (0, 3, 4):  # tight, unaligned and aligned pitch
        buf, pitch = CH.padded(frames, pad)
        d = torch.from_numpy(buf).cuda()
        torch.cuda.synchronize()
        dev = runtime.Calibrator(rows, cols, split, max_batch=k, opts=runtime.calib_opts(**o))
        dev.set_background(bkg)
        dev.push_device(d.data_ptr(), pitch, 4)
        dev.push_device(d.data_ptr() + 4 * pitch, pitch, k - 4)
        CH.assert_records_equal(dev.records(), want, pad)  # (waits for the pushes: d may go after it)
        dev.close()
    host.close()


def test_background_reset_and_refused_pushes():
    rows, cols, split = 8, 64, 7
    frames, bkg = CH.record_scene(rows, cols, split, False)
    zero = np.zeros_like(bkg)
    o = CH.opts_of(radius=3)
    cal = runtime.Calibrator(rows, cols, split, max_batch=6, opts=runtime.calib_opts(**o))
    assert cal.frames == 0 and cal.records().shape == (0, 2)
    cal.push(frames[:6])                       # no background yet: all zero
    cal.set_background(bkg)                    # holds for the pushes after it; the records so far stay
    cal.push(frames[6:12])
    want = np.concatenate([CH.ref_records(frames[:6], zero, split, o), CH.ref_records(frames[6:12], bkg, split, o)])
    CH.assert_records_equal(cal.records(), want)
    cal.reset()                                # the background stays
    assert cal.frames == 0
    with pytest.raises(runtime.LMError) as e:  # the records are gone
        cal.records(0, 1)
    assert e.value.code == abi.LM_ERR_INVALID_ARGUMENT
    cal.push(frames[2:5])
    CH.assert_records_equal(cal.records(), CH.ref_records(frames[2:5], bkg, split, o))
    with pytest.raises(runtime.LMError) as e:  # more than max_batch
        cal.push(np.zeros((7, rows, cols), np.uint8))
    assert e.value.code == abi.LM_ERR_INVALID_ARGUMENT and cal.frames == 3
    rc = runtime.lib().lm_calib_push(cal._h, frames.ctypes.data, rows * cols - 1, 2)  # a pitch below the frame size
    assert rc == abi.LM_ERR_INVALID_ARGUMENT and b"pitch" in runtime.lib().lm_last_error() and cal.frames == 3
    with pytest.raises(runtime.LMError):
        cal.records(1, 3)
    CH.assert_records_equal(cal.records(1, 2), CH.ref_records(frames[3:5], bkg, split, o))
    cal.close()


def test_record_buffer_grows_past_its_first_size():
    """More frames than the records' first allocation holds: the kept records are carried over."""
    rows, cols, split = 8, 64, 1
    frames, bkg = CH.record_scene(rows, cols, split, False)
    o = CH.opts_of(radius=3)
    want13 = CH.ref_records(frames, bkg, split, o)
    reps = 90                                  # 1170 frames, past the 1024 the context starts with
    stack = np.ascontiguousarray(np.tile(frames, (reps, 1, 1)))
    cal = runtime.Calibrator(rows, cols, split, max_batch=300, opts=runtime.calib_opts(**o))
    cal.set_background(bkg)
    for s in range(0, len(stack), 300):
        cal.push(stack[s:s + 300])
    assert cal.frames == 13 * reps
    CH.assert_records_equal(cal.records(), np.tile(want13, (reps, 1)))
    cal.close()


# ---- the programs end to end

def _run(cmd, env=None, timeout=300):
    e = dict(os.environ)
    e.update(env or {})
    p = subprocess.run(cmd, capture_output=True, text=True, env=e, timeout=timeout)
    return p.returncode, p.stdout


def _fs_matrix(path, key, cap):
    """A matrix read with the project's FileStorage reader (tests/cpp/host_harness.cpp)."""
    import host_harness as H
    kind, rows, cols = C.c_int(), C.c_int(), C.c_int()
    dt = C.c_char()
    out = np.zeros(cap)
    text = C.create_string_buffer(256)
    rc = H.lib().lmh_fs_node(os.fsencode(path), key.encode(), C.byref(kind), C.byref(rows), C.byref(cols), C.byref(dt),
                             out.ctypes.data, out.size, text, 256)
    assert rc == 0 and kind.value == 6, (key, rc, text.value)
    return out[:rows.value * cols.value].reshape(rows.value, cols.value)


def test_estimated_calibration_undoes_the_camera_and_gives_the_same_tracks(tmp_path):
    rows, cols, split = CH.ROWS, CH.COLS, CH.SPLIT
    h = CH.camera_table()
    video = CH.marker_video()
    marker_avi = str(tmp_path / "marker.avi")
    MW.write_avi(marker_avi, video, bits=8)
    estimated = str(tmp_path / "estimated.yml")
    rc, text = _run([runtime.CALIB_CLI_PATH, marker_avi, estimated, str(split)], env={"LM_TIMING": "1"})
    assert rc == 0, text
    assert text.startswith(f"Calibration of {len(video)} frames: ") and "LM_TIMING background_ms" in text, text

    m = _fs_matrix(estimated, "ind_warp_mapping", rows * cols).astype(np.int64)
    assert m.shape == (rows, cols)
    assert np.array_equal(m[split:], np.arange(rows * cols).reshape(rows, cols)[split:])
    col = m[0]
    assert all(np.array_equal(m[r] - r * cols, col) for r in range(split))
    assert _fs_matrix(estimated, "view_boxes", 8).tolist() == [[0, 0, cols, split], [0, split, cols, rows - split]]
    lo, hi = _fs_matrix(estimated, "warp_range", 2)[0]
    cov = CH.covered_columns(lo, hi)
    assert len(cov) >= 700 and np.array_equal(h[col[cov]], cov), (lo, hi, int((h[col[cov]] != cov).sum()))
    cfg = S.SyntheticConfig()
    for box in (cfg.params.bounding_box_side, cfg.params.bounding_box_bottom):
        assert lo <= box.x and box.x + box.width <= hi
    counts = _fs_matrix(estimated, "warp_counts", 3)[0]
    assert counts[0] == len(video) and counts[2] >= 0.9 * len(video)
    # the program's map is the restatement's, from the median it estimated itself
    bkg = np.sort(video, axis=0)[(500 * (len(video) - 1)) // 1000]
    fit = CH.ref_fit(CH.ref_records(video, bkg, split, CH.DEFAULTS), cols, CH.DEFAULTS, 2)
    assert np.array_equal(col, np.array(CH.ref_columns(fit, cols)))
    assert _fs_matrix(estimated, "warp_coefficients", 4)[0].tolist() == fit["coef"]

    # LocoMouse on a synthetic video seen through the same camera: the estimated map against one built from h
    n = 12
    paths = {k: str(tmp_path / v) for k, v in (("config", "config.yml"), ("video", "mouse_R.avi"), ("background", "mouse_R.png"),
                                              ("model", "model.yml"), ("direct", "direct.yml"))}
    MW.write_config(paths["config"], cfg)
    MW.write_model(paths["model"], cfg)
    MW.write_png(paths["background"], CH.through_camera(cfg.background[None], h)[0])
    MW.write_avi(paths["video"], CH.through_camera(cfg.frames(0, n), h), bits=24)
    direct = CH.map_from_table(h)
    assert np.array_equal(h[direct[0][cov]], cov)
    with open(paths["direct"], "w") as fh:
        fh.write("%YAML:1.0\n---\n" + MW.yaml_matrix("ind_warp_mapping", direct, "i", per_line=32)
                 + MW.yaml_matrix("view_boxes", [[0, 0, cols, split], [0, split, cols, rows - split]], "i"))
    outs = []
    for name, calibration in (("a", estimated), ("b", paths["direct"])):
        out = tmp_path / name
        out.mkdir()
        rc, text = _run([runtime.CLI_PATH, "0", paths["config"], paths["video"], paths["background"], paths["model"],
                         calibration, "R", str(out)], env={"LM_BATCH": "16"})
        assert rc == 0, text
        outs.append((out / "output_mouse_R.yml").read_bytes())
    assert len(outs[0]) > 1000 and outs[0] == outs[1]
