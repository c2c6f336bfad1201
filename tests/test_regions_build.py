"""Compile-time properties of csrc/mf_regions.hip: every kernel of the unit holds its working set in registers -- no scratch
memory, no VGPR or SGPR spills -- and the number of kernels is pinned.  Checked by compiling the
unit for gfx950 with hipcc's resource-usage remarks, as tests/test_frames_build.py does (no GPU needed)."""
import os

import pytest

from test_build_properties import HIPCC, _compile, _unit_flags

KERNELS = ("reg_tile_kernel", "reg_seam_kernel", "reg_flatten_kernel", "reg_best_kernel", "reg_select_kernel", "reg_hole_mark_kernel",
           "reg_hole_fill_kernel", "reg_table_count_kernel", "reg_table_area_kernel", "reg_table_rows_kernel", "reg_table_bbox_kernel")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_regions_kernels_have_no_scratch_and_no_spills():
    usage, _ = _compile("mf_regions", _unit_flags("mf_regions"))
    for kernel in KERNELS:
        assert any(kernel in name for name in usage), (kernel, sorted(usage))
    assert len(usage) == len(KERNELS) == 11, sorted(usage)
    for name, u in usage.items():
        assert any(kernel in name for kernel in KERNELS), name
        assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
