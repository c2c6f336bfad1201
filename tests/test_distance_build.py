"""Compile-time properties of csrc/mf_distance.hip: every kernel of the unit holds its working set in registers -- no scratch
memory, no VGPR or SGPR spills -- and the number of kernels is pinned: the three passes and the count's finish.  Checked by
compiling the unit for gfx950 with hipcc's resource-usage remarks, as tests/test_voxelize_build.py does (no GPU needed)."""
import os

import pytest

from test_build_properties import HIPCC, _compile, _unit_flags

KERNELS = ("edt_z_kernel", "edt_y_kernel", "edt_x_kernel", "edt_count_finish_kernel")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_distance_kernels_have_no_scratch_and_no_spills():
    usage, _ = _compile("mf_distance", _unit_flags("mf_distance"))
    for kernel in KERNELS:
        assert any(kernel in name for name in usage), (kernel, sorted(usage))
    assert len(usage) == len(KERNELS) == 4, sorted(usage)
    for name, u in usage.items():
        assert any(kernel in name for kernel in KERNELS), name
        assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
