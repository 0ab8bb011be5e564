"""GPU parity of a batch that inherits its halo frame's crop corners: corners
(bb) given for one batch and omitted for the next.  Slot 0 of the second batch
is then cropped from the context's last_bb (lm_batch_plan.h) -- the one path of
the slot table that the pipelined tests (test_gpu_pipeline.py) do not reach."""
import numpy as np
import pytest

import edge_scenes as E
from locomouse_cpp_amd import synthetic as S
from locomouse_cpp_amd.results import concat_results
from test_gpu_parity import _oracle, assert_same
from test_gpu_pipeline import _pctx

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("lanes", [1, 2])
def test_corners_given_then_omitted(lanes):
    """Frames 0-3 with moving corners, frames 4-7 without bb: slot 0 of the
    second batch (frame 3) keeps the corners it had in its own batch -- carried
    on one lane, cropped again from them after the hand-off on two -- and
    frames 4-7 take the provided box's."""
    cfg = S.SyntheticConfig()
    frames = cfg.frames(0, 8)
    bb = E.moving_corners(cfg, 4)
    p = cfg.params
    box = [p.bounding_box_bottom.x + p.bounding_box_bottom.width, p.bounding_box_bottom.y + p.bounding_box_bottom.height,
           p.bounding_box_side.y + p.bounding_box_side.height]
    ref = _oracle(cfg, frames, bb=np.concatenate([bb, np.tile(np.array(box, np.int32), (4, 1))])).result
    ctx = _pctx(cfg, lanes, 4)
    ctx.submit(frames[0:4], 0, bb=bb)
    ctx.submit(frames[4:8], 4)
    parts = [ctx.collect(), ctx.collect()]
    assert_same(concat_results(parts), ref, f"corners then none, {lanes} lanes: ")
