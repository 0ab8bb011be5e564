"""Histogram matching of the bottom crop (include/locomouse_match.h), the
parts that run without a GPU: the header and the exported names, NULL and bad
arguments, the reference CDF's validation, lm_match_cdf and the core's
histogram, CDF and table (csrc/lm_match_core.h) against the numpy restatement
tests/match_ref.py bit for bit, a stand-alone sanitizer run of the core
against a brute-force statement, and the batch plan of a matched context
(tests/cpp/match_plan_check.cpp), and the LocoMouse program's switch
LM_REFERENCE_BRIGHTNESS up to the point where a device would be touched.  Nothing here is loaded into Python under a
sanitizer."""
import ctypes as C
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_ref as MR  # noqa: E402
import media_writers as MW  # noqa: E402

from locomouse_cpp_amd import abi, runtime  # noqa: E402
from locomouse_cpp_amd import synthetic as S  # noqa: E402

ROOT = runtime.ROOT
HDR = os.path.join(ROOT, "include", "locomouse_match.h")
CSRC = os.path.join(ROOT, "locomouse_cpp_amd", "csrc")
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


def declared_functions(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"^[A-Za-z_][\w\s\*]*?\b(lm_\w+)\s*\(", text, flags=re.M)))


def _build(name, exe, flags):
    subprocess.check_call(["g++", *flags, "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I" + CSRC,
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", name), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def match_check(tmp_path_factory):
    return _build("match_check.cpp", str(tmp_path_factory.mktemp("match") / "match_check"), ["-O2"])


def test_header_and_exports():
    assert set(declared_functions(HDR)) == set(runtime.MATCH_EXPORTED)
    assert len(set(runtime.MATCH_EXPORTED)) == len(runtime.MATCH_EXPORTED)
    L = runtime.lib()
    for sym in runtime.MATCH_EXPORTED:
        assert getattr(L, sym) is not None
    for other in (runtime.EXPORTED, runtime.JPEG_EXPORTED, runtime.BKG_EXPORTED, runtime.ENC_EXPORTED, runtime.TRAIN_EXPORTED,
                  runtime.CALIB_EXPORTED):
        assert not set(runtime.MATCH_EXPORTED) & set(other)
    assert L.lm_abi_version() == 6


def test_null_and_bad_arguments_without_gpu():
    L = runtime.lib()
    E = abi.LM_ERR_INVALID_ARGUMENT
    img = np.zeros((4, 5), np.uint8)
    out = np.zeros(256, np.float32)
    assert L.lm_match_cdf(None, 4, 5, 5, out.ctypes.data) == E and b"null" in L.lm_last_error()
    assert L.lm_match_cdf(img.ctypes.data, 4, 5, 5, None) == E
    for rows, cols, pitch in ((0, 5, 5), (4, 0, 5), (-1, 5, 5), (4, 5, 4), (65536, 65536, 65536)):
        assert L.lm_match_cdf(img.ctypes.data, rows, cols, pitch, out.ctypes.data) == E, (rows, cols, pitch)
    h = C.c_void_p(1)
    cfg = S.SyntheticConfig()
    good = MR.cdf(np.arange(256, dtype=np.uint8).reshape(16, 16))
    args = (C.byref(cfg.setup), C.byref(cfg.params), C.byref(cfg.model))
    assert L.lm_ctx_create_matched(0, *args, good.ctypes.data, 4, None) == E and b"out is NULL" in L.lm_last_error()
    assert L.lm_ctx_create_matched(0, *args, None, 4, C.byref(h)) == E and not h.value
    assert b"reference_cdf is NULL" in L.lm_last_error()
    for fn in (L.lm_debug_match_hist, L.lm_debug_match_table):
        assert fn(None, 0, out.ctypes.data) == E
    assert L.lm_debug_match_crop(None, 0, 0, out.ctypes.data, 1, 1) == E
    with pytest.raises(ValueError):
        runtime.match_cdf(np.zeros((4, 4), np.float32))


def test_reference_cdf_validation_and_the_two_options():
    """256 finite, non-negative, non-decreasing floats; both options of
    lm_params must be 0.  Every refusal comes before a device is touched."""
    L = runtime.lib()
    E = abi.LM_ERR_INVALID_ARGUMENT
    cfg = S.SyntheticConfig()
    good = MR.cdf(np.arange(256, dtype=np.uint8).reshape(16, 16))
    h = C.c_void_p()

    def create(cdf, c=cfg):
        cdf = np.ascontiguousarray(cdf, np.float32)
        return L.lm_ctx_create_matched(0, C.byref(c.setup), C.byref(c.params), C.byref(c.model), cdf.ctypes.data, 4, C.byref(h))
    for i, v, word in ((0, np.nan, b"finite"), (255, np.inf, b"finite"), (7, -np.inf, b"finite"), (0, -1e-6, b"non-negative"),
                       (100, good[99] - 1e-3, b"non-decreasing"), (255, 0.5, b"non-decreasing")):
        bad = good.copy()
        bad[i] = v
        assert create(bad) == E and not h.value, (i, v)
        assert word in L.lm_last_error(), (i, v, L.lm_last_error())
    for field in ("use_reference_image_brightness", "transform_gray_values"):
        c = S.SyntheticConfig()
        setattr(c.params, field, 1)
        assert create(good, c) == E and not h.value and b"must be 0" in L.lm_last_error()
    with pytest.raises(ValueError):
        runtime.Context(cfg, reference_cdf=np.zeros(255, np.float32))


def _dump(exe, tmp_path, image, ref, pitch=None):
    image = np.ascontiguousarray(image, np.uint8)
    rows, cols = image.shape
    pitch = cols if pitch is None else pitch
    buf = np.zeros((rows, pitch), np.uint8)
    buf[:, :cols] = image
    buf[:, cols:] = 77  # the bytes between the rows are not pixels
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as fh:
        fh.write(struct.pack("<iii", rows, cols, pitch) + buf.tobytes() + np.ascontiguousarray(ref, np.float32).tobytes())
    subprocess.check_call([exe, "dump", fin, fout])
    raw = open(fout, "rb").read()
    assert len(raw) == 1024 + 1024 + 256 + 4
    return (np.frombuffer(raw, np.uint32, 256), np.frombuffer(raw, np.float32, 256, 1024), np.frombuffer(raw, np.uint8, 256, 2048),
            struct.unpack("<i", raw[2304:])[0])


def _images():
    rng = np.random.default_rng(20240611)
    out = {
        "random": rng.integers(0, 256, (61, 83), dtype=np.uint8),
        "random dark": (rng.integers(0, 256, (40, 57)) ** 2 // 700).astype(np.uint8),
        "single value": np.full((19, 23), 131, np.uint8),
        "prime n": rng.integers(0, 200, (1, 9973), dtype=np.uint8),  # n = 9973
        "one bin, n >= 65536": np.full((257, 256), 3, np.uint8),
        "397 x 139": rng.integers(0, 256, (139, 397), dtype=np.uint8),
    }
    return out


def _references():
    rng = np.random.default_rng(7)
    plateaus = np.repeat(np.array([0.1, 0.1, 0.55, 1.0], np.float32), 64)
    return {
        "an image's": MR.cdf(rng.integers(0, 256, (50, 50)).astype(np.uint8) // 2 + 100),
        "ends at 0.9": (np.float32(0.9) * np.arange(1, 257, dtype=np.float32) / np.float32(256)).astype(np.float32),
        "plateaus": plateaus,
        "zeros": np.zeros(256, np.float32),
    }


@pytest.mark.parametrize("iname", list(_images()))
def test_core_equals_the_restatement_bit_for_bit(iname, match_check, tmp_path):
    """lm_match_cdf and the core's histogram, CDF and table against
    tests/match_ref.py; a reference that ends below the image CDF's last value
    runs the second loop (asserted), one that covers it only the first."""
    img = _images()[iname]
    got_cdf = runtime.match_cdf(img)
    h = MR.hist(img)
    c = MR.cdf_of_hist(h, img.size)
    assert np.array_equal(got_cdf.view(np.uint32), c.view(np.uint32))
    ran = {}
    for rname, ref in _references().items():
        gh, gc, gt, gfb = _dump(match_check, tmp_path, img, ref, pitch=img.shape[1] + 3)
        T, fb = MR.table(c, ref)
        assert np.array_equal(gh, h.astype(np.uint32)), rname
        assert np.array_equal(gc.view(np.uint32), c.view(np.uint32)), rname
        assert np.array_equal(gt, T), rname
        assert gfb == fb, rname
        ran[rname] = fb
    assert ran["ends at 0.9"] > 0 and ran["zeros"] > 0  # the second loop ran
    assert all(fb < 256 for name, fb in ran.items() if name != "zeros")  # and the first


def test_cdf_of_one_bin_is_the_rounded_product():
    """n >= 65536 pixels in one bin: p = float(n) * float(1 / n), one product
    rounded once, and the CDF is flat from there."""
    img = np.full((300, 256), 9, np.uint8)
    c = runtime.match_cdf(img)
    want = np.float32(np.float32(img.size) * np.float32(1.0 / img.size))
    assert np.all(c[:9] == 0) and np.all(c[9:].view(np.uint32) == want.view(np.uint32))
    # a row pitch wider than the row: the bytes between rows are not counted
    wide = np.full((300, 300), 200, np.uint8)
    wide[:, :256] = 9
    out = np.zeros(256, np.float32)
    assert runtime.lib().lm_match_cdf(wide.ctypes.data, 300, 256, 300, out.ctypes.data) == 0
    assert np.array_equal(out.view(np.uint32), c.view(np.uint32))


def test_core_against_brute_force_under_the_sanitizers(tmp_path):
    """tests/cpp/match_check.cpp built with -fsanitize=address,undefined:
    seeded images and references, both loops of the table reached."""
    exe = _build("match_check.cpp", str(tmp_path / "match_check_san"), SAN)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    m = re.search(r"(\d+) cases, fallback in (\d+), first branch in (\d+), (\d+) failures", r.stdout)
    assert r.returncode == 0 and m, r.stdout[-2000:] + r.stderr[-2000:]
    cases, fb, first, failures = map(int, m.groups())
    assert cases > 1000 and fb > 100 and first > 100 and failures == 0


PLAN_LINE = re.compile(r"(\d+) batches, modes first (\d+) given (\d+) carry (\d+) handoff (\d+), refused match (\d+) roi (\d+), "
                       r"(\d+) checks, (\d+) failures")


@pytest.mark.parametrize("flags", [["-O2"], SAN], ids=["plain", "sanitizers"])
def test_batch_plan_of_a_matched_context(flags, tmp_path):
    """Which slots get a table, which slot's table each reader uses, and the
    refusal of a box that leaves the image, in every batch mode."""
    exe = _build("match_plan_check.cpp", str(tmp_path / "match_plan_check"), flags)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    m = PLAN_LINE.search(r.stdout)
    assert r.returncode == 0 and m, r.stdout[-2000:] + r.stderr[-2000:]
    n = list(map(int, m.groups()))
    assert all(v > 0 for v in n[:8]) and n[8] == 0, n


def test_planted_plan_errors_are_caught(tmp_path):
    """A copy of lm_batch_plan.h that skips the rule for the unprocessed slot 0,
    and one whose I_PREV_PAD reads the current slot's table."""
    text = open(os.path.join(CSRC, "lm_batch_plan.h")).read()
    for old, new in (("const int t = prev ? s - 1 : s;", "const int t = s;"),
                     ("  *s0 = s_lut0;\n  return n + 1 - s_lut0;", "  *s0 = 1;\n  return n;")):
        assert text.count(old) == 1, old
        inc = tmp_path / "inc"
        inc.mkdir(exist_ok=True)
        (inc / "lm_batch_plan.h").write_text(text.replace(old, new))
        exe = str(tmp_path / "planted")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + str(inc), "-I" + CSRC, "-I" + os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "cpp", "match_plan_check.cpp"), "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
        m = PLAN_LINE.search(r.stdout)
        assert r.returncode == 1 and m and int(m.group(9)) > 0, (old, r.stdout[-1000:])


# ------------------------------------------------- the program's switch (no GPU)

def _cli(args, env):
    e = dict(os.environ)
    e.pop("LM_REFERENCE_BRIGHTNESS", None)
    e.update(env)
    p = subprocess.run([runtime.CLI_PATH, *args], capture_output=True, text=True, env=e, timeout=300)
    return p.returncode, p.stdout


def _cli_inputs(tmp_path, overrides, ref=None, colour=False):
    cfg = S.SyntheticConfig()
    paths = MW.write_inputs(str(tmp_path), cfg, 2)
    MW.write_config(paths["config"], cfg, overrides=overrides)
    if ref is not None:
        MW.write_png(str(tmp_path / "ref.png"), np.stack([ref, ref // 2, ref // 3], 2) if colour else ref)
    return [
        "0", paths["config"], paths["video"], paths["background"], paths["model"], paths["calibration"], "R", str(tmp_path)]


@pytest.mark.parametrize("value", ["yes", "1", "Intended", "intended "])
def test_cli_refuses_other_values_before_a_device_is_touched(value, tmp_path):
    """Any value but `intended` (or nothing) is an Invalid inputs error, raised
    once the argument list is parsed -- even with a config file that does not
    exist, so before the config is read, a video opened or a device touched."""
    args = _cli_inputs(tmp_path, {})
    args[1] = str(tmp_path / "none.yml")
    rc, out = _cli(args, {"LM_REFERENCE_BRIGHTNESS": value})
    assert rc == 1 and f"Invalid inputs: LM_REFERENCE_BRIGHTNESS: must be intended, not {value}." in out, out
    assert "Failed to read config file" not in out


def test_cli_inputs_carry_the_reference_image(tmp_path):
    """load_config keeps the PNG's pixels (a path relative to the reference
    path, as :172), a colour file converted to grey; set but empty means unset."""
    ref = (np.arange(40 * 50).reshape(40, 50) % 200).astype(np.uint8)
    args = _cli_inputs(tmp_path, {"use_reference_image_brightness": 1, "reference_image_path": '"' + str(tmp_path / "ref.png") + '"'}, ref)
    for env, word in (({"LM_REFERENCE_BRIGHTNESS": "intended"}, "intended"), ({}, "as_executed"),
                      ({"LM_REFERENCE_BRIGHTNESS": ""}, "as_executed")):
        rc, out = _cli(args, dict(env, LM_PRINT_INPUTS="1"))
        assert rc == 0 and f"reference {word} 40 50 {int(ref.sum())}" in out.splitlines(), out
    args = _cli_inputs(tmp_path, {"use_reference_image_brightness": 1, "reference_image_path": '"' + str(tmp_path / "ref.png") + '"'},
                       ref, colour=True)
    rc, out = _cli(args, {"LM_REFERENCE_BRIGHTNESS": "intended", "LM_PRINT_INPUTS": "1"})
    line = [x for x in out.splitlines() if x.startswith("reference ")]
    assert rc == 0 and line and line[0].split()[:4] == ["reference", "intended", "40", "50"], out
    grey = int(line[0].split()[4])
    assert int((ref // 3).sum()) < grey < int(ref.sum())  # a grey conversion of the three channels, not channel 0
    # without the option the program says nothing about a reference
    rc, out = _cli(_cli_inputs(tmp_path, {}), {"LM_REFERENCE_BRIGHTNESS": "intended", "LM_PRINT_INPUTS": "1"})
    assert rc == 0 and "reference " not in out, out


@pytest.mark.parametrize("intended", [False, True])
def test_cli_reference_image_errors_are_the_reference_s(intended, tmp_path):
    """:152-190 with and without the switch: a missing image is an error with
    the option alone, and falls back to the table with both options set."""
    env = {"LM_REFERENCE_BRIGHTNESS": "intended"} if intended else {}
    args = _cli_inputs(tmp_path, {"use_reference_image_brightness": 1, "reference_image_path": '"none.png"'})
    rc, out = _cli(args, env)
    assert rc == 1 and "Invalid inputs: Invalid configuration parameter: Failed to open reference image: none.png." in out, out
    args = _cli_inputs(tmp_path, {"use_reference_image_brightness": 1, "transform_gray_values": 1,
                                  "reference_image_path": '"none.png"'})
    rc, out = _cli(args, env)
    assert rc == 1 and "Only one of 'use_reference_image_brightness' or 'transform_gray_values' should be true." in out
    assert "Could not open the reference image. Applying the provided transformation on the gray levels..." in out
    assert "Could not load the gray level transformation from the config file." in out, out
