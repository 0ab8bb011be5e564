"""bench.py's command line on the GPU: a plain run only times the steps,
`--full` adds the oracle check and the CPU baselines, and `--dump-outputs`
writes the results of the last timed step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from locomouse_cpp_amd import synthetic as S
from locomouse_cpp_amd.results import slice_results

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = ["--gpus", "1", "--streams", "2", "--batch", "16", "--resident", "100", "--steps", "2", "--warmup", "1"]


def _bench(args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *SHAPE, *args], env=env, capture_output=True,
                       text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    from oracle import oracle as O
    line = _bench(["--dump-outputs", str(tmp_path)])
    assert line["steps"] == 2 and line["unit"] == "frames/s" and line["higher_is_better"] is True
    # two contexts x 16 frames per step
    assert line["value"] == pytest.approx(32 / (line["ms_per_step"] * 1e-3), rel=1e-3)
    for k in ("parity_sample", "cpu_baseline", "cpu_baseline_threads", "cpu_baseline_node"):
        assert k not in line
    # context k cycles frames [400 k, 400 k + 400); its last timed batch is its
    # third, frames 400 k + 32 .. 400 k + 47, with frame 400 k + 31 before it
    cfg = S.SyntheticConfig()
    for k in range(2):
        first = 400 * k + 32
        ref = slice_results(O.OracleRun(cfg, bench._scene_frames(cfg, range(first - 1, first + 16))).result, 1)
        for name, a in bench.result_arrays(f"ctx{k}.", ref):
            got = np.load(tmp_path / (name + ".npy"))
            assert got.dtype == np.float64 and got.shape == a.shape and np.array_equal(got, a), name


def test_full_run_checks_the_timed_batches_and_measures_the_cpu():
    line = _bench(["--full", "--cpu-seconds", "0.1"])
    assert line["parity_sample"]["bit_exact"] and line["parity_sample"]["frames"] == 32
    for k in ("cpu_baseline", "cpu_baseline_threads", "cpu_baseline_node"):
        assert line[k]["value"] > 0
