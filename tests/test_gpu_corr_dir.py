"""The ring correlation's wave directory on the GPU (LM_CORR_DIR, default 1:
k_corr_dir writes the cumulative waves of each launch group's detectors once
per batch, and a wave of k_corr_rw / k_corr_rw_all finds its detector, or that
it has none, from that record; csrc/lm_corr_dir.h).  Every case runs one batch
of the C3 geometry with the directory and once more with LM_CORR_DIR=0 (the
waves walk their group's detectors as before): every result array must be
bit-identical between the two and to the oracle.  A batch that sets the
lane's error word (a group whose waves exceed its grid sets it) fails in
detect(), so a passing case also had a zero error word.  Batches of 3 frames
(one ingest group, few list segments in use) and 9 (two groups), each with the
per-width plan and the merged one (forced by the context's debug bits, which
choose as LM_CORR_PLAN does: the variable itself is read once per process, so
one pytest process could not run both); scenes with ordinary lists, with empty
lists (every workgroup returns), with long ones (a checkerboard), with each
kind of list taken away (the unlisted branch next to listed detectors) and a
flipped calibration."""
import functools

import numpy as np
import pytest

import edge_scenes as E
from locomouse_cpp_amd import runtime as rt
from locomouse_cpp_amd import synthetic as S
from test_gpu_parity import _oracle, assert_same
from test_gpu_tail_skip import _plan

pytestmark = pytest.mark.gpu

# scene -> (flip, switch that is set to 0 or None)
SCENES = {
    "default": (False, None),
    "blank": (False, None),
    "checker": (False, None),
    "dark_off": (False, "LM_CORR_DARK"),
    "tailskip_off": (False, "LM_CORR_TAILSKIP"),
    "pointskip_off": (False, "LM_CORR_POINTSKIP"),
    "flip": (True, None),
}


def _frames(cfg, scene, n):
    if scene == "blank":
        return np.stack([E.blank(cfg)] * n)
    if scene == "checker":
        return E.checker_frames(cfg, n)
    return cfg.frames(20, n)


@functools.lru_cache(maxsize=None)
def _case(scene, n):
    """The case's configuration, frames and oracle result (the oracle does not
    depend on the switches or the plan: computed once per scene and size)."""
    flip, _ = SCENES[scene]
    cfg = S.SyntheticConfig(flip=flip)
    frames = _frames(cfg, "default" if scene in ("dark_off", "tailskip_off", "pointskip_off", "flip") else scene, n)
    frames.setflags(write=False)
    return cfg, frames, _oracle(cfg, frames).result


@pytest.mark.parametrize("plan", [0, 1])
@pytest.mark.parametrize("n", [3, 9])
@pytest.mark.parametrize("scene", list(SCENES))
def test_directory_against_walk_and_oracle(scene, n, plan, monkeypatch):
    cfg, frames, ref = _case(scene, n)
    off = SCENES[scene][1]
    if off:
        monkeypatch.setenv(off, "0")
    got = {}
    for d in ("1", "0"):
        monkeypatch.setenv("LM_CORR_DIR", d)
        ctx = rt.Context(cfg, max_batch=n)
        ctx.set_debug(_plan(plan))
        got[d] = ctx.detect(frames, 0)  # (raises on a non-zero error word)
        ctx.close()
    label = f"{scene}, {n} frames, plan {plan}: "
    assert_same(got["1"], got["0"], label + "directory against walk: ")
    assert_same(got["1"], ref, label + "directory against the oracle: ")
    assert_same(got["0"], ref, label + "walk against the oracle: ")
