"""The folded fp32 inference stream (mf_nerf_pack_fold, MF_F_FOLDED_FINAL) without a GPU: its sizes, its refusals on the host,
and the compile-time properties of the two kernels that read it (the way tests/test_build_properties.py checks the others)."""
import ctypes
import os
import re

import pytest

from test_build_properties import HIPCC, _compile

SCRATCH = (128 * 256 + 128) * 4          # W' ((W/2) x W) and b' (W/2) as fp32 ...
SCRATCH = (SCRATCH + 1023) // 1024 * 1024   # ... padded to a whole 1 KiB group (include/mocoflow_hip.h): 129 KiB


def _desc(L, extra, dim, W=256):
    d = L.mf_nerf_desc()
    d.D, d.W, d.in_channels_xyz, d.skip_mask = 8, W, 63, 1 << 4
    d.extra_feat_type, d.extra_feat_dim = extra, dim
    return d


def test_fold_packed_sizes():
    """The folded stream is the fp32 one minus xyz_encoding_final's 8 panels of 32 groups, plus the scratch area; the
    unfolded sizes are what they were."""
    import moco_flow_amd._lib as L
    lib = L.lib()
    assert SCRATCH == 129 * 1024
    for extra, dim, ge in ((L.MF_EXTRA_DIR, 27, 36), (L.MF_EXTRA_IND, 5, 34), (L.MF_EXTRA_NONE, 0, 32)):
        d = _desc(L, extra, dim)
        stream = 13 * 1024 + ((8 + 3 * 32 + 40 + 3 * 32) * 8 + ge * 4) * 1024
        got = lib.mf_nerf_fold_packed_bytes(ctypes.byref(d))
        assert got >= stream, (extra, got)
        assert got - stream == SCRATCH, (extra, got - stream)
        assert lib.mf_nerf_packed_bytes(ctypes.byref(d)) == stream + 32 * 8 * 1024          # unchanged
        assert lib.mf_nerf_packed_bytes_p(ctypes.byref(d), L.MF_PREC_F32) == stream + 32 * 8 * 1024
    assert lib.mf_version() == 16


def test_fold_refusals_on_the_host():
    import moco_flow_amd._lib as L
    lib = L.lib()
    d = _desc(L, L.MF_EXTRA_DIR, 27, W=128)
    assert lib.mf_nerf_packed_bytes(ctypes.byref(d)) > 0                   # the fp32 forward takes W = 128 ...
    assert lib.mf_nerf_fold_packed_bytes(ctypes.byref(d)) == 0             # ... the folded stream does not
    assert b"unsupported" in lib.mf_last_error()
    p = ctypes.c_void_p(4096)
    assert lib.mf_nerf_pack_fold(ctypes.byref(d), p, None) == -3
    assert lib.mf_nerf_fold_packed_bytes(None) == 0
    d = _desc(L, L.MF_EXTRA_DIR, 27)
    assert lib.mf_nerf_pack_fold(None, p, None) == -1
    assert lib.mf_nerf_pack_fold(ctypes.byref(d), None, None) == -1
    assert lib.mf_nerf_pack_fold(ctypes.byref(d), p, None) == -1 and b"missing" in lib.mf_last_error()    # no weight pointers
    assert L.MF_F_FOLDED_FINAL == 8


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_fold_kernels_have_no_spills_and_stream_weights_by_buffer_dma():
    """render_fold_kernel<MOCO>: no spilled VGPR, no scratch, <= 256 VGPRs (two waves per SIMD), weights by the buffer form
    of the LDS-DMA; and the unit still holds render_kernel<MOCO, DUMP> under their names."""
    usage, asm = _compile("mf_render", [])
    fold = {k: v for k, v in usage.items() if "render_fold_kernel" in k}
    assert len(fold) == 2, sorted(usage)                                   # <MOCO = false | true>
    for k, u in fold.items():
        assert u["VGPRs Spill"] == 0 and u["ScratchSize"] == 0, (k, u)
        assert u["VGPRs"] <= 256 and u["Occupancy"] == 2, (k, u)
    assert len([k for k in usage if re.search(r"render_kernelILb[01]ELb[01]EE", k)]) == 4
    assert "global_load_lds" not in asm
    for k in fold:                                                         # each kernel's own body streams by buffer DMA
        body = asm[asm.index(k + ":"):]
        body = body[:body.index("s_endpgm")]
        assert len(re.findall(r"buffer_load_dwordx4 .* lds", body)) > 10, k
        assert "scratch_" not in body, k
