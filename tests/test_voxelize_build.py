"""Compile-time properties of csrc/mf_voxelize.hip: every kernel of the unit holds its working set in registers -- no scratch
memory, no VGPR or SGPR spills (the surface pass keeps a triangle's nine edge functions and its plane in registers; the walk of
large boxes is a kernel of its own for that reason) -- and the number of kernels is pinned.  Checked by compiling the unit for
gfx950 with hipcc's resource-usage remarks, as tests/test_mesh_smooth_build.py does (no GPU needed)."""
import os

import pytest

from test_build_properties import HIPCC, _compile, _unit_flags

KERNELS = ("voxel_clear_kernel", "voxel_surface_kernel", "voxel_surface_big_kernel", "voxel_fill_init_kernel",
           "voxel_fill_union_kernel", "voxel_fill_emit_kernel", "voxel_dilate_z_kernel", "voxel_dilate_rows_kernel",
           "voxel_count_finish_kernel")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_voxelize_kernels_have_no_scratch_and_no_spills():
    usage, _ = _compile("mf_voxelize", _unit_flags("mf_voxelize"))
    for kernel in KERNELS:
        assert any(kernel in name for name in usage), (kernel, sorted(usage))
    assert len(usage) == len(KERNELS) == 9, sorted(usage)
    for name, u in usage.items():
        assert any(kernel in name for kernel in KERNELS), name
        assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
