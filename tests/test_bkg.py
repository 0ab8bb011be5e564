"""The background estimate (include/locomouse_bkg.h), the parts that run
without a GPU: the header and the exported names, NULL and bad arguments, the
host statement of csrc/lm_bkg_core.h (the code the kernels run per pixel)
against numpy, a stand-alone sanitizer run of it against a brute-force sort,
host/Media.cpp's PNG writer, and the error paths of the two programs."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bkg_harness as BH  # noqa: E402
import media_writers as MW  # noqa: E402

from locomouse_cpp_amd import abi, runtime  # noqa: E402
from locomouse_cpp_amd import synthetic as S  # noqa: E402

HDR = os.path.join(runtime.ROOT, "include", "locomouse_bkg.h")


def declared_functions(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"^[A-Za-z_][\w\s\*]*?\b(lm_\w+)\s*\(", text, flags=re.M)))


def test_header_and_exports():
    assert set(declared_functions(HDR)) == set(runtime.BKG_EXPORTED)
    assert len(set(runtime.BKG_EXPORTED)) == len(runtime.BKG_EXPORTED)
    L = runtime.lib()
    for sym in runtime.BKG_EXPORTED:
        assert getattr(L, sym) is not None
    assert not set(runtime.BKG_EXPORTED) & set(runtime.EXPORTED)
    assert not set(runtime.BKG_EXPORTED) & set(runtime.JPEG_EXPORTED)
    assert L.lm_abi_version() == 6
    m = re.search(r"^#define LM_BKG_MAX_SAMPLES (\d+)\b", open(HDR).read(), flags=re.M)
    assert m and int(m.group(1)) == abi.LM_BKG_MAX_SAMPLES >= 65535
    assert BH.lib().bh_max_samples() == abi.LM_BKG_MAX_SAMPLES  # the shared header's counters hold it
    assert "lm_bkg.hip" in runtime.HIP_UNITS


def test_null_and_bad_arguments_without_gpu():
    L = runtime.lib()
    assert L.lm_bkg_create(0, 8, 8, 4, None) == abi.LM_ERR_INVALID_ARGUMENT
    assert b"out is NULL" in L.lm_last_error()
    h = C.c_void_p()
    for rows, cols, max_batch in ((0, 8, 4), (8, 0, 4), (8, 8, 0), (-1, 8, 4), (8, 8, 65536)):
        assert L.lm_bkg_create(0, rows, cols, max_batch, C.byref(h)) == abi.LM_ERR_INVALID_ARGUMENT and not h.value
    out = np.zeros(64, np.uint8)
    assert L.lm_bkg_finish(None, 500, out.ctypes.data) == abi.LM_ERR_INVALID_ARGUMENT
    assert L.lm_bkg_push(None, out.ctypes.data, 64, 1) == abi.LM_ERR_INVALID_ARGUMENT
    assert L.lm_bkg_push_device(None, None, 64, 1) == abi.LM_ERR_INVALID_ARGUMENT
    assert L.lm_bkg_reset(None) == abi.LM_ERR_INVALID_ARGUMENT
    assert L.lm_bkg_samples(None) == -1
    assert L.lm_bkg_stream(None) is None
    L.lm_bkg_destroy(None)


def test_rank_is_the_integer_formula():
    L = BH.lib()
    for k in (1, 2, 3, 7, 20, 33, 1000, 1001, 65535):
        for pm in (0, 1, 250, 499, 500, 501, 999, 1000):
            assert L.bh_rank(pm, k) == (pm * (k - 1)) // 1000
    assert L.bh_rank(500, 2) == 0 and L.bh_rank(500, 3) == 1  # the lower median


@pytest.mark.parametrize("shape", BH.SHAPES, ids=[s[0] for s in BH.SHAPES])
def test_host_statement_equals_numpy(shape):
    name, rows, cols, pad, k, max_batch = shape
    stack = BH.shape_stack(name)
    buf, pitch = BH.padded(stack, pad)
    for pm in BH.PERMILLES:
        got = BH.host_median(buf, pitch, k, rows, cols, BH.pushes_of(k, max_batch), pm)
        assert np.array_equal(got, BH.numpy_median(stack, pm)), (name, pm)


def test_host_statement_at_the_workload_frame_size():
    cfg = S.SyntheticConfig()
    stack = cfg.frames(0, 20)
    buf, pitch = BH.padded(stack, 0)
    for pm in (250, 500):
        got = BH.host_median(buf, pitch, 20, cfg.rows, cfg.cols, [20], pm)
        assert np.array_equal(got, BH.numpy_median(stack, pm))


def test_host_counter_does_not_wrap_at_300_frames():
    stack = BH.patterned(300, 8, 8, seed=300)
    stack[:, 0, 0] = 9
    buf, pitch = BH.padded(stack, 0)
    got = BH.host_median(buf, pitch, 300, 8, 8, BH.pushes_of(300, 64), 500)
    assert got[0, 0] == 9 and np.array_equal(got, BH.numpy_median(stack, 500))


def test_core_is_clean_under_the_sanitizers(tmp_path):
    """A stand-alone program (tests/cpp/bkg_core_check.cpp) built with
    -fsanitize=address,undefined runs csrc/lm_bkg_core.h on 400 random small
    cases against a brute-force sort; nothing is loaded into Python."""
    exe = tmp_path / "bkg_core_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",  # the runtimes in the program itself
                           *BH.INCLUDES, "-o", str(exe), BH.CHECK_SRC])
    r = subprocess.run([str(exe), "400", "20261019"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "400 cases, 0 failures" in r.stdout, r.stdout


@pytest.mark.parametrize("shape", [(1, 1), (3, 37), (256, 1024)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_write_png_gray_round_trips(tmp_path, shape):
    from PIL import Image
    rng = np.random.default_rng(shape[1])
    img = rng.integers(0, 256, size=shape, dtype=np.uint8)
    img.flat[0], img.flat[-1] = 0, 255
    p = str(tmp_path / "w.png")
    assert BH.lib().bh_write_png(os.fsencode(p), shape[0], shape[1], img.ctypes.data) == 0
    with Image.open(p) as im:
        assert im.mode == "L" and im.size == (shape[1], shape[0])
        assert np.array_equal(np.asarray(im), img)
    r, c = C.c_int(), C.c_int()
    back = np.zeros(img.size, np.uint8)
    assert BH.lib().bh_read_png(os.fsencode(p), C.byref(r), C.byref(c), back.ctypes.data, back.size) == 0
    assert (r.value, c.value) == shape and np.array_equal(back.reshape(shape), img)
    assert BH.lib().bh_write_png(os.fsencode(str(tmp_path / "no_such_dir" / "w.png")), shape[0], shape[1],
                                 img.ctypes.data) == 1


def test_estimate_background_refusals_name_the_stride_that_fits():
    cap = abi.LM_BKG_MAX_SAMPLES
    m = BH.refusal(cap + 1)
    assert m.endswith("the smallest stride that fits is 2.") and str(cap) in m, m
    assert BH.refusal(200000, stride=3).endswith("the smallest stride that fits is 4.")  # 66,667 sampled; 50,000 at 4
    assert BH.refusal(3 * cap + 1, stride=2).endswith("the smallest stride that fits is 4.")
    assert "no frames" in BH.refusal(0)
    assert "stride" in BH.refusal(10, stride=0) and "permille" in BH.refusal(10, permille=1001)


def test_background_spec_parser():
    assert BH.parse_spec("median") == (1, 500)
    assert BH.parse_spec("median:4") == (4, 500)
    assert BH.parse_spec("median:4:250") == (4, 250)
    assert BH.parse_spec("median:1:0") == (1, 0) and BH.parse_spec("median:7:1000") == (7, 1000)
    for bad in ("", "mean", "median:", "median:0", "median:-1", "median:2:", "median:2:1001", "median:2:5:1", "median:1.5"):
        m = BH.parse_spec(bad)
        assert isinstance(m, str) and m.startswith("LM_BACKGROUND: "), (bad, m)


def _run(cmd, env=None, timeout=120):
    e = dict(os.environ)
    e.update(env or {})
    p = subprocess.run(cmd, capture_output=True, text=True, env=e, timeout=timeout)
    return p.returncode, p.stdout


@pytest.mark.parametrize("spec", ["mean", "median:0", "median:2:1001", "median:2:500:1", "Median", "median:x"])
def test_cli_refuses_another_background_method(tmp_path, spec):
    """LM_BACKGROUND other than median[:stride[:permille]] is refused before a
    device is touched (this test runs without one)."""
    cfg = S.SyntheticConfig()
    paths = MW.write_inputs(str(tmp_path), cfg, 2)
    args = ["0", paths["config"], paths["video"], paths["background"], paths["model"], paths["calibration"], "R",
            str(tmp_path)]
    rc, out = _run([runtime.CLI_PATH, *args], env={"LM_BACKGROUND": spec})
    assert rc == 1, out
    assert "Invalid inputs: LM_BACKGROUND: " in out, out
    assert "Total Elapsed time:" in out
    assert not os.path.exists(tmp_path / "output_synth_R.yml")


def test_background_program_errors(tmp_path):
    exe = runtime.BKG_CLI_PATH
    for args in ([], ["only.avi"], ["a.avi", "b.png", "1", "500", "extra"]):
        rc, out = _run([exe, *args])
        assert rc == 1 and out.startswith("Usage: LocoMouseBackground video.avi out.png [stride [permille]]"), out
    missing = str(tmp_path / "none.avi")
    rc, out = _run([exe, missing, str(tmp_path / "out.png"), "1"])
    assert rc == 1 and f"Could not open the video file: {missing}." in out, out
    assert not os.path.exists(tmp_path / "out.png")
    rc, out = _run([exe, missing, str(tmp_path / "out.png"), "0"])  # a stride of 0 is no stride
    assert rc == 1 and out.startswith("Usage: "), out
