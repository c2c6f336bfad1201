"""Compile-time properties of csrc/mf_mesh_smooth.hip: every kernel of the unit holds its working set in registers -- no scratch
memory, no VGPR or SGPR spills (the lane-per-vertex sort works in a column of LDS, not in a private array) -- and the
number of kernels is pinned.  Checked by compiling the unit for gfx950 with hipcc's resource-usage remarks, as
tests/test_regions_build.py does (no GPU needed)."""
import os

import pytest

from test_build_properties import HIPCC, _compile, _unit_flags

KERNELS = ("ring_count_kernel", "ring_sum_kernel", "ring_top_kernel", "ring_prefix_kernel", "ring_fill_kernel", "ring_short_kernel",
           "ring_long_kernel", "ring_emit_kernel", "ring_emit_long_kernel", "smooth_pack_kernel", "smooth_step_kernel",
           "smooth_unpack_kernel")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_mesh_smooth_kernels_have_no_scratch_and_no_spills():
    usage, _ = _compile("mf_mesh_smooth", _unit_flags("mf_mesh_smooth"))
    for kernel in KERNELS:
        assert any(kernel in name for name in usage), (kernel, sorted(usage))
    assert len(usage) == len(KERNELS) == 12, sorted(usage)
    for name, u in usage.items():
        assert any(kernel in name for kernel in KERNELS), name
        assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
