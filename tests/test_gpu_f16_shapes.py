"""k_corr_f16<NCH> (lm_corr.hip), the MFMA correlation of LM_CORR_F16, bit
for bit against the CPU oracle at every chunk count NCH = 2..10 (widths 1 to
129), detector heights 1 to 7 (the row loop's groups of three, its kh % 3
remainder and the clamped prefetch of one- and two-row detectors), output
sizes on the residues of the 128 x 64 workgroup tile that switch a wave, one
of its two 32 x 32 accumulator tiles or a ballot word off, LDS windows above
64 KiB and at the 160 KiB cap, per-frame crops, flip and a batch seam.

The scenes are f16_scenes.py's: weights n / 4096 and u8 pixels, so every
partial sum is exact in fp32 and the f16 mode has nothing to round
(test_f16_scenes.py asserts that bound and that the lists, the accumulator
tiles and the last rows and columns hold candidates).  Pinned: the four
candidate lists with their scores and everything derived from them
(assert_same), the tail points, and TAIL_MASK -- with tail_sub_bounding_box =
1 and a half-positive tail_bottom map of essentially one component, the map
itself, ballot word by ballot word."""
import numpy as np
import pytest

import f16_scenes as F
from locomouse_cpp_amd.results import concat_results
from locomouse_cpp_amd.runtime import Context, LMError
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu


def _check_geometry(sc, g):
    """The output sizes are the intended residues of the workgroup tile."""
    box = F.BOXES[sc.case.boxes]
    ow_r, ohb_r, ohs_r = F.BOX_RESIDUES[sc.case.boxes]
    assert (g.bb_bottom_mouse.width, g.bb_bottom_mouse.height) == box["bottom"][2:]
    assert (g.bb_side_mouse.width, g.bb_side_mouse.height) == box["side"][2:]
    assert g.tail_box_width == g.bb_bottom_mouse.width == g.bb_side_mouse.width
    assert g.bb_bottom_mouse.width % 128 == ow_r
    assert g.bb_bottom_mouse.height % 64 == ohb_r and g.bb_side_mouse.height % 64 == ohs_r


def _compare(name):
    sc = F.scene(name)
    case = sc.case
    ctx = Context(F.gpu_config(sc), max_batch=4)
    try:
        ctx.set_debug(1)
        g = ctx.geometry()
        _check_geometry(sc, g)
        shape = (g.bb_bottom_mouse.height, g.tail_box_width)
        parts, masks = [], []
        if case.seam:  # frames 1.. in batches of two after the halo frame 0
            for lo in range(1, len(sc.frames), 2):
                fr = sc.frames[lo:lo + 2]
                parts.append(ctx.detect(fr, lo, prev_frame=sc.frames[0] if lo == 1 else None))
                masks += [ctx.debug_tail_mask(f) for f in range(len(fr))]
        else:
            parts.append(ctx.detect(sc.frames, 0, bb=sc.bb))
            masks = [ctx.debug_tail_mask(f) for f in range(len(sc.frames))]
        got = concat_results(parts) if len(parts) > 1 else parts[0]
        ref = sc.result
        assert int(ref["n_frames"]) == case.n == len(masks)
        assert_same(got, ref, f"f16 {name} (NCH {case.classes}): ")
        for f, m in enumerate(masks):
            exp = sc.ref.tail_mask(sc.drop + f, shape)
            assert np.array_equal(m, exp), f"f16 {name}: TAIL_MASK of frame {f} differs at {np.argwhere(m != exp)[:8].tolist()}"
        return masks
    finally:
        ctx.close()


@pytest.mark.parametrize("nch", range(2, 11))
def test_f16_every_chunk_count(nch):
    """Six detectors of one class (one launch group of k_corr_f16<nch>):
    5 x kw_max, 7 x kw_min, 4 x (kw_max - 1), 2 x kw_max, 1 x kw_min and 3 x a
    width between; odd classes on 161 x 97 / 161 x 90 outputs, even ones on
    225 x 129 / 225 x 65."""
    assert F.CASES[f"nch{nch}"].classes == [nch]
    _compare(f"nch{nch}")


def test_f16_six_classes_in_one_context():
    assert F.CASES["mixed"].classes == [3, 4, 6, 7, 9, 10]
    _compare("mixed")


@pytest.mark.parametrize("name", ["ow128_oh64", "ow160_oh96", "ow193"])
def test_f16_tile_edges(name):
    """Outputs that are exact multiples of the 128 x 64 tile; 160 x 96 and
    160 x 32 (a wave's second accumulator tile and the second wave row exactly
    off); 193 columns (one column into the second wave)."""
    _compare(name)


@pytest.mark.parametrize("name", ["moving", "flip", "seam"])
def test_f16_crops_flip_and_seam(name):
    """Per-frame corners (window loads at any alignment), flipped frames, and
    five frames in batches of two after a halo frame."""
    assert F.CASES[name].classes[0] >= 7
    _compare(name)


def test_f16_dense_tail_map():
    """Every tail_bottom score positive: every ballot word of the box, the
    partial last one included, all ones."""
    for m in _compare("dense_tail"):
        assert m.all()


@pytest.mark.parametrize("name", ["tall64", "tall247"])
def test_f16_tall_detectors(name):
    """64 x 129: a 67,056-byte window, the first above 64 KiB; 247 x 129:
    163,680 bytes, the largest the runtime accepts."""
    _compare(name)


def test_f16_acceptance_boundary():
    Context(F.boundary_config(1, 129), max_batch=4).close()
    for kh, kw in ((1, 130), (248, 129)):
        with pytest.raises(LMError, match="too large for the f16"):
            Context(F.boundary_config(kh, kw), max_batch=4)
