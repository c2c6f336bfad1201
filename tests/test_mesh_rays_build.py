"""Compile-time properties of csrc/mf_mesh_rays.hip: every kernel of the unit holds its working set in registers -- no scratch
memory, no VGPR or SGPR spills -- and the number of kernels is pinned: the corner rows and the cast in its two modes.  The
lifted helpers (csrc/mf_f3.hpp) add no kernel to either unit that includes them.  Checked by compiling the unit for gfx950 with
hipcc's resource-usage remarks, as tests/test_mesh_distance_build.py does (no GPU needed)."""
import os

import pytest

from test_build_properties import HIPCC, _compile, _unit_flags

KERNELS = ("mr_corners_kernel", "mr_cast_kernelILi0EE", "mr_cast_kernelILi1EE")       # <MODE = 0 first | 1 any>


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_mesh_ray_kernels_have_no_scratch_and_no_spills():
    usage, asm = _compile("mf_mesh_rays", _unit_flags("mf_mesh_rays"))
    for kernel in KERNELS:
        assert sum(kernel in name for name in usage) == 1, (kernel, sorted(usage))
    assert len(usage) == len(KERNELS) == 3, sorted(usage)
    for name, u in usage.items():
        assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
    # the cast keeps eight waves per SIMD (what the compile reports): nothing but other waves hides the latency of a tile's rows
    for name, u in usage.items():
        if "mr_cast_kernel" in name:
            assert u["Occupancy"] == 8, (name, u)
    # a tile's corner rows come through the scalar cache, eight floats at a time
    assert "s_load_dwordx8" in asm
