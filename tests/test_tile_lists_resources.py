"""Register budget of the tile-bound pre-pass with the narrow class on
(k_tile_bound<false, true> and k_tile_bound<true, true>), read from the code
objects' metadata (no GPU needed): at most 64 VGPRs, so that eight workgroups
of four waves share a compute unit (amdgpu_waves_per_eu(8, 8)), no scratch and
no VGPR spill.  Step 5w keeps a chunk of 64 entries in registers between its
two passes; a variant of the earlier tail that carried more across its passes
spilled six VGPRs (profiles/narrow/README.md)."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
LIB = os.path.join(ROOT, "locomouse_cpp_amd", "liblocomouse_hip.so")


@pytest.fixture(scope="module")
def tile_bound():
    if not os.path.exists(LIB):
        pytest.skip("liblocomouse_hip.so not built")
    import kernel_resources
    ks = kernel_resources.kernels(LIB)
    # k_tile_bound<ROWS, NARROW>: _Z12k_tile_boundILb<ROWS>ELb<NARROW>EE...
    out = {}
    for name, r in ks.items():
        m = re.match(r"_Z12k_tile_boundILb([01])ELb([01])EE", name)
        if m:
            out[(int(m.group(1)), int(m.group(2)))] = r
    return out


def test_all_four_instantiations_are_built(tile_bound):
    assert sorted(tile_bound) == [(0, 0), (0, 1), (1, 0), (1, 1)], sorted(tile_bound)


@pytest.mark.parametrize("rows", [0, 1])
def test_narrow_instantiation_budget(tile_bound, rows):
    r = tile_bound[(rows, 1)]
    print(rows, r)
    assert r["vgpr_count"] <= 64, r
    assert r.get("agpr_count", 0) == 0, r
    assert r["private_segment_fixed_size"] == 0, r
    assert r["vgpr_spill_count"] == 0, r
