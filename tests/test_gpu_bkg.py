"""The background estimate on the GPU (include/locomouse_bkg.h,
csrc/lm_bkg.hip): every result is compared exactly with the numpy statement
np.sort(stack, axis=0)[(permille * (K - 1)) // 1000]."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bkg_harness as BH  # noqa: E402
import media_writers as MW  # noqa: E402

from locomouse_cpp_amd import abi, runtime  # noqa: E402
from locomouse_cpp_amd import synthetic as S  # noqa: E402

pytestmark = pytest.mark.gpu


def push_all(est, buf, pitch, k):
    """The k frames of `buf`, `pitch` bytes apart, in pushes of the context's max_batch (lm_bkg_push)."""
    for s in range(0, k, est.max_batch):
        n = min(est.max_batch, k - s)
        rc = runtime.lib().lm_bkg_push(est._h, buf[s * pitch:].ctypes.data, pitch, n)
        assert rc == abi.LM_OK, runtime.lib().lm_last_error()


@pytest.mark.parametrize("shape", BH.SHAPES, ids=[s[0] for s in BH.SHAPES])
def test_shapes_and_patterns_equal_numpy(shape):
    name, rows, cols, pad, k, max_batch = shape
    stack = BH.shape_stack(name)
    buf, pitch = BH.padded(stack, pad)
    est = runtime.BackgroundEstimator(rows, cols, max_batch=max_batch)
    push_all(est, buf, pitch, k)
    assert est.samples == k
    for pm in BH.PERMILLES:
        assert np.array_equal(est.finish(pm), BH.numpy_median(stack, pm)), (name, pm)
    est.close()


def test_workload_frame_size():
    cfg = S.SyntheticConfig()
    stack = cfg.frames(0, 20)
    est = runtime.BackgroundEstimator(cfg.rows, cfg.cols, max_batch=20)
    est.push(stack)
    ordered = np.sort(stack, axis=0)
    for pm in BH.PERMILLES:
        assert np.array_equal(est.finish(pm), ordered[(pm * 19) // 1000]), pm
    est.close()


def test_state_finish_push_reset():
    rows, cols = 8, 64
    a, b = BH.patterned(5, rows, cols, seed=1), BH.patterned(6, rows, cols, seed=2)
    est = runtime.BackgroundEstimator(rows, cols, max_batch=6)
    with pytest.raises(runtime.LMError) as e:  # nothing pushed yet
        est.finish()
    assert e.value.code == abi.LM_ERR_INVALID_ARGUMENT
    est.push(a)
    first, second = est.finish(500), est.finish(500)
    assert np.array_equal(first, second) and np.array_equal(first, BH.numpy_median(a, 500))
    est.push(b)  # a push after a finish keeps accumulating
    assert est.samples == 11
    both = np.concatenate([a, b])
    for pm in BH.PERMILLES:
        assert np.array_equal(est.finish(pm), BH.numpy_median(both, pm)), pm
    est.reset()
    assert est.samples == 0
    with pytest.raises(runtime.LMError):
        est.finish()
    est.push(b)
    assert est.samples == 6 and np.array_equal(est.finish(250), BH.numpy_median(b, 250))
    for pm in (-1, 1001):
        with pytest.raises(runtime.LMError) as e:
            est.finish(pm)
        assert e.value.code == abi.LM_ERR_INVALID_ARGUMENT
    with pytest.raises(runtime.LMError) as e:  # more than max_batch
        est.push(np.zeros((7, rows, cols), np.uint8))
    assert e.value.code == abi.LM_ERR_INVALID_ARGUMENT and est.samples == 6
    rc = runtime.lib().lm_bkg_push(est._h, b.ctypes.data, rows * cols - 1, 2)  # a pitch below the frame size
    assert rc == abi.LM_ERR_INVALID_ARGUMENT and b"pitch" in runtime.lib().lm_last_error() and est.samples == 6
    assert np.array_equal(est.finish(250), BH.numpy_median(b, 250))
    est.close()


def test_counters_hold_300_equal_samples():
    """One pixel constant over 300 frames: an 8-bit counter would wrap."""
    stack = BH.patterned(300, 8, 8, seed=300)
    stack[:, 0, 0] = 9
    est = runtime.BackgroundEstimator(8, 8, max_batch=64)
    for s in range(0, 300, 64):
        est.push(stack[s:s + 64])
    assert est.samples == 300
    for pm in BH.PERMILLES:
        got = est.finish(pm)
        assert got[0, 0] == 9 and np.array_equal(got, BH.numpy_median(stack, pm)), pm
    est.close()


def test_sample_cap_is_refused_whole():
    """LM_BKG_MAX_SAMPLES is below 2^20: constant frames up to the cap exactly,
    then a push that would pass it is refused and changes nothing."""
    cap = abi.LM_BKG_MAX_SAMPLES
    assert cap < 1 << 20
    rng = np.random.default_rng(8)
    image = rng.integers(0, 256, size=(8, 8), dtype=np.uint8)
    batch = np.ascontiguousarray(np.broadcast_to(image, (4096, 8, 8)))
    est = runtime.BackgroundEstimator(8, 8, max_batch=4096)
    while est.samples + 4096 < cap:
        est.push(batch)
    est.push(batch[:cap - 1 - est.samples])
    assert est.samples == cap - 1
    other = np.ascontiguousarray(np.broadcast_to(255 - image, (2, 8, 8)))
    with pytest.raises(runtime.LMError) as e:  # 2 frames with room for 1: none of them counts
        est.push(other)
    assert e.value.code == abi.LM_ERR_INVALID_ARGUMENT and est.samples == cap - 1
    est.push(batch[:1])
    assert est.samples == cap
    at_cap = [est.finish(pm) for pm in BH.PERMILLES]
    assert all(np.array_equal(g, image) for g in at_cap)
    with pytest.raises(runtime.LMError) as e:
        est.push(other[:1])
    assert e.value.code == abi.LM_ERR_INVALID_ARGUMENT and b"LM_BKG_MAX_SAMPLES" in runtime.lib().lm_last_error()
    assert est.samples == cap
    assert all(np.array_equal(est.finish(pm), image) for pm in BH.PERMILLES)
    est.close()


def test_push_device_equals_push():
    import torch
    rows, cols, k = 16, 130, 9
    stack = BH.patterned(k, rows, cols, seed=77)
    host = runtime.BackgroundEstimator(rows, cols, max_batch=k)
    host.push(stack)
    for pad in (0, 3, 4):  # tight, unaligned and aligned pitch
        buf, pitch = BH.padded(stack, pad)
        d = torch.from_numpy(buf).cuda()
        torch.cuda.synchronize()
        dev = runtime.BackgroundEstimator(rows, cols, max_batch=k)
        dev.push_device(d.data_ptr(), pitch, 4)
        dev.push_device(d.data_ptr() + 4 * pitch, pitch, k - 4)
        for pm in BH.PERMILLES:
            got = dev.finish(pm)  # (waits for the pushes: d may go after it)
            assert np.array_equal(got, host.finish(pm)) and np.array_equal(got, BH.numpy_median(stack, pm)), (pad, pm)
        dev.close()
    host.close()


def test_push_device_of_a_jpeg_decoders_output():
    import torch
    import jpeg_harness as JH
    rows, cols = 34, 50
    jpegs = MW.jpeg_frames(JH.frames(4, rows, cols, 5), mode="RGB", quality=90, subsampling=2)  # 4:2:0
    dec = runtime.JpegDecoder(rows, cols, max_batch=4)
    d, status = dec.decode(jpegs)
    assert (status == abi.LM_JPEG_OK).all()
    decoded = d.cpu().numpy()
    dev = runtime.BackgroundEstimator(rows, cols, max_batch=4)
    dev.push_device(d.data_ptr(), rows * cols, 4)
    host = runtime.BackgroundEstimator(rows, cols, max_batch=4)
    host.push(decoded)
    for pm in BH.PERMILLES:
        got = dev.finish(pm)
        assert np.array_equal(got, host.finish(pm)) and np.array_equal(got, BH.numpy_median(decoded, pm)), pm
    torch.cuda.synchronize()
    for c in (dev, host, dec):
        c.close()


# ---- the programs end to end, on a 40-frame synthetic video

N_VIDEO = 40
JPEG = dict(mode="RGB", quality=92, subsampling=2)


def _run(cmd, env=None, timeout=300):
    e = dict(os.environ)
    e.update(env or {})
    p = subprocess.run(cmd, capture_output=True, text=True, env=e, timeout=timeout)
    return p.returncode, p.stdout


def _inputs(tmp_path, kind):
    cfg = S.SyntheticConfig()
    paths = MW.write_inputs(str(tmp_path), cfg, N_VIDEO, stem="mouse_R", bits=24, jpeg=JPEG if kind == "mjpeg" else None)
    frames = paths["decoded"] if kind == "mjpeg" else cfg.frames(0, N_VIDEO)
    return cfg, paths, frames


@pytest.mark.parametrize("kind", ["avi", "mjpeg"])
def test_background_program_writes_the_median(tmp_path, kind):
    from PIL import Image
    cfg, paths, frames = _inputs(tmp_path, kind)
    out = str(tmp_path / "bkg.png")
    rc, text = _run([runtime.BKG_CLI_PATH, paths["video"], out, "1"])
    assert rc == 0, text
    with Image.open(out) as im:
        assert np.array_equal(np.asarray(im), BH.numpy_median(frames, 500))
    rc, text = _run([runtime.BKG_CLI_PATH, paths["video"], out, "3", "900"], env={"LM_READ_THREADS": "2"})
    assert rc == 0, text
    with Image.open(out) as im:
        assert np.array_equal(np.asarray(im), BH.numpy_median(frames[::3], 900))


@pytest.mark.parametrize("spec,stride,permille", [("median", 1, 500), ("median:4:250", 4, 250)])
@pytest.mark.parametrize("kind", ["avi", "mjpeg"])
def test_cli_background_knob_equals_a_run_on_the_numpy_median(tmp_path, kind, spec, stride, permille):
    from PIL import Image
    cfg, paths, frames = _inputs(tmp_path, kind)
    want = BH.numpy_median(frames[::stride], permille)
    out_a, out_b = tmp_path / "a", tmp_path / "b"
    out_a.mkdir()
    out_b.mkdir()

    def args(background, outdir):
        return ["0", paths["config"], paths["video"], background, paths["model"], paths["calibration"], "R", str(outdir)]

    saved = str(tmp_path / "saved.png")
    rc, text = _run([runtime.CLI_PATH, *args(str(tmp_path / "no_such_background.png"), out_a)],
                    env={"LM_BACKGROUND": spec, "LM_BACKGROUND_SAVE": saved, "LM_BATCH": "16", "LM_TIMING": "1"})
    assert rc == 0, text
    with Image.open(saved) as im:
        assert np.array_equal(np.asarray(im), want)
    timing = [ln for ln in text.splitlines() if ln.startswith("LM_TIMING ")][0].split()
    assert float(timing[timing.index("background_ms") + 1]) > 0
    MW.write_png(paths["background"], want)
    rc, text = _run([runtime.CLI_PATH, *args(paths["background"], out_b)], env={"LM_BATCH": "16"})
    assert rc == 0, text
    a = (out_a / "output_mouse_R.yml").read_bytes()
    assert len(a) > 1000 and a == (out_b / "output_mouse_R.yml").read_bytes()


def test_cli_print_inputs_sums_the_estimated_background(tmp_path):
    cfg, paths, frames = _inputs(tmp_path, "avi")
    args = ["0", paths["config"], paths["video"], str(tmp_path / "none.png"), paths["model"], paths["calibration"], "R",
            str(tmp_path)]
    rc, text = _run([runtime.CLI_PATH, *args], env={"LM_BACKGROUND": "median:2", "LM_PRINT_INPUTS": "1"})
    assert rc == 0, text
    d = dict(line.split(" ", 1) for line in text.splitlines() if " " in line)
    assert int(d["background_sum"]) == int(BH.numpy_median(frames[::2], 500).astype(np.int64).sum())
