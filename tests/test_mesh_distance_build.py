"""Compile-time properties of csrc/mf_mesh_distance.hip: every kernel of the unit holds its working set in registers -- no
scratch memory, no VGPR or SGPR spills -- and the number of kernels is pinned: the four of mf_surface_records, the closest-point
search, the weights, the sampler, the statistics and their finish.  Checked by compiling the unit
for gfx950 with hipcc's resource-usage remarks, as tests/test_distance_build.py does (no GPU needed)."""
import os

import pytest

from test_build_properties import HIPCC, _compile, _unit_flags

KERNELS = ("md_fill_kernel", "md_claim_kernel", "md_build_kernel", "md_unplaced_kernel", "md_closest_kernel",
           "md_weights_kernel", "md_sample_kernel", "md_stats_kernel", "md_stats_finish_kernel")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_mesh_distance_kernels_have_no_scratch_and_no_spills():
    usage, asm = _compile("mf_mesh_distance", _unit_flags("mf_mesh_distance"))
    for kernel in KERNELS:
        assert any(kernel in name for name in usage), (kernel, sorted(usage))
    assert len(usage) == len(KERNELS) == 9, sorted(usage)
    for name, u in usage.items():
        assert any(kernel in name for kernel in KERNELS), name
        assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
    # the search keeps eight waves per SIMD: nothing but other waves hides the latency of a tile's records
    for name, u in usage.items():
        if "md_closest_kernel" in name:
            assert u["Occupancy"] == 8, (name, u)
