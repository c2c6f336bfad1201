"""Compile-time properties of csrc/mf_frames.hip: every kernel of the unit holds its working set in registers -- no scratch, no
VGPR spills (a tap array indexed at run time, or a key tile that did not unroll, would show up here as scratch).  Checked by
compiling the unit for gfx950 with hipcc's resource-usage remarks, as tests/test_build_properties.py does (no GPU needed)."""
import os

import pytest

from test_build_properties import HIPCC, _compile, _unit_flags

KERNELS = ("resize_horizontal_kernel", "resize_vertical_kernel", "composite_rows_kernel", "plate_staged_kernel", "plate_streamed_kernel")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_frames_kernels_have_no_scratch_and_no_spills():
    usage, _ = _compile("mf_frames", _unit_flags("mf_frames"))
    for kernel in KERNELS:
        assert any(kernel in name for name in usage), (kernel, sorted(usage))
    # every instantiation the entries launch: 4 + 4 resize passes, 2 composites, 2 x 2 plates
    assert len(usage) == 14, sorted(usage)
    for name, u in usage.items():
        assert any(kernel in name for kernel in KERNELS), name
        assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
