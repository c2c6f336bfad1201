"""Validation metrics without a GPU: the restatement (tests/metrics_oracle.py) against closed forms that do not depend on
it, its reflect indexing, and the host-side argument validation of mf_ssim / mf_sqerr (include/mocoflow_hip.h)."""
import ctypes

import pytest
import torch

import metrics_oracle as O

C1, C2 = 1e-4, 9e-4


def closed_form(p, q):
    """Constant images a = p, b = q: every sigma is 0, the map is (2pq + C1) / (p^2 + q^2 + C1) (C2 cancels) up to the
    formula's eps = 1e-12, which lowers it by eps / ((p^2 + q^2 + C1) C2) relative: below 1e-8 where p^2 + q^2 >= 0.11, as in
    every case here (the black pair p = q = 0, where eps shows as 1.1e-5, is test_identical_images_map_is_one's)."""
    return (2 * p * q + C1) / (p * p + q * q + C1)


@pytest.mark.parametrize("ws", [3, 7, 11])
@pytest.mark.parametrize("p,q", [(0.0, 0.4), (1.0, 1.0), (0.3, 0.8), (1.0, 0.0), (0.5, 0.45)])
def test_constant_images_closed_form(ws, p, q):
    shape = (2, 3, 13, 17)
    for dtype, tol in ((torch.float64, 1e-8), (torch.float32, 1e-3)):
        # fp32: a few ulp of 0.5 on each sigma, divided by C2 = 9e-4
        a, b = torch.full(shape, p, dtype=dtype), torch.full(shape, q, dtype=dtype)
        m = O.ssim_map(a, b, ws)
        assert m.shape == shape and m.dtype == dtype
        err = (m.double() - closed_form(p, q)).abs().max().item()
        print(f"ws={ws} p={p} q={q} {dtype}: max err {err:.3e}")
        assert err <= tol


@pytest.mark.parametrize("ws", [3, 11])
def test_identical_images_map_is_one(ws):
    pred, gt = O.frame_pair((1, 3, 23, 31), seed=3)
    a = gt.double()
    a[:, :, 15:, 10:20] = 0.0                     # a black flat patch: where eps / (C1 C2) is the whole deviation
    m = O.ssim_map(a, a.clone(), ws)
    err = (m - 1).abs().max().item()
    print(f"ws={ws}: max |map - 1| = {err:.3e}")
    assert err <= 1.2e-5                           # eps / (C1 C2) = 1e-12 / 9e-8


def test_reflect_indexing_on_a_ramp():
    H, W = 4, 5
    ramp = torch.arange(H * W, dtype=torch.float64).view(1, 1, H, W)
    # F.pad(mode='reflect') by 2: rows -2..5 -> 2 1 0 1 2 3 2 1; columns -2..6 -> 2 1 0 1 2 3 4 3 2
    rows = [2, 1, 0, 1, 2, 3, 2, 1]
    cols = [2, 1, 0, 1, 2, 3, 4, 3, 2]
    assert [O.reflect_index(i, H) for i in range(-2, H + 2)] == rows
    assert [O.reflect_index(i, W) for i in range(-2, W + 2)] == cols
    padded = torch.nn.functional.pad(ramp, (2, 2, 2, 2), mode='reflect')[0, 0]
    want = torch.tensor([[r * W + c for c in cols] for r in rows], dtype=torch.float64)
    assert torch.equal(padded, want)
    # and through the restatement: mu of the ramp at the corner with a window of 5 is the windowed sum of that table
    g = O.gaussian_1d(5)
    mu00 = (g[:, None] * g[None, :] * want[:5, :5]).sum()
    a = ramp / (H * W)
    m = O.ssim_map(a, a, 5, eps=0.0)
    assert torch.allclose(m, torch.ones_like(m), atol=1e-12)
    k = (g[:, None] * g[None, :])[None, None]
    mu = torch.nn.functional.conv2d(padded[None, None], k)
    assert abs(mu[0, 0, 0, 0].item() - mu00.item()) < 1e-12


def test_oracle_mse_psnr():
    a = torch.tensor([[0.0, 0.5, 1.0], [0.25, 0.25, 0.25]])
    b = torch.tensor([[0.0, 0.0, 0.0], [0.25, 0.5, 0.0]])
    assert O.mse(a, b).item() == pytest.approx((0.25 + 1 + 0.0625 + 0.0625) / 6)
    mask = torch.tensor([False, True])
    assert O.mse(a, b, mask).item() == pytest.approx(0.125 / 3)
    assert O.psnr(a, b, mask).item() == pytest.approx(-10 * torch.log10(torch.tensor(0.125 / 3)).item())
    assert O.mse(a, b, reduction='none').shape == a.shape


def test_package_exports_metrics():
    import moco_flow_amd
    assert hasattr(moco_flow_amd, 'metrics')
    for name in ("mse", "psnr", "ssim", "image_metrics"):
        assert callable(getattr(moco_flow_amd.metrics, name))
    assert set(moco_flow_amd.metrics.__all__) == {"mse", "psnr", "ssim", "image_metrics"}


def _ssim_call(lib, B, C, H, W, ws, a=True, sums=True, scratch=True, strides=True):
    """mf_ssim with host placeholders for the device pointers: every call here must be refused before anything is launched."""
    buf = (ctypes.c_double * 8)()
    p = ctypes.addressof(buf)
    st = (ctypes.c_int64 * 4)(C * H * W, H * W, W, 1)
    return lib.mf_ssim(p if a else None, st if strides else None, p, st, B, C, H, W, ws, 1.0, 1e-12, None, p if sums else None,
                       p if scratch else None, None)


def test_ssim_abi_validates_on_the_host():
    import moco_flow_amd._lib as L
    lib = L.lib()
    assert lib.mf_ssim_scratch_bytes(1, 3, 540, 540) > 0
    assert lib.mf_ssim_scratch_bytes(0, 3, 540, 540) == 0          # empty sizes
    assert lib.mf_ssim_scratch_bytes(1, 3, 0, 540) == 0
    assert lib.mf_ssim_scratch_bytes(1, 3, -1, 540) == -1
    assert b"negative" in lib.mf_last_error()
    assert lib.mf_ssim_scratch_bytes(1 << 31, 1 << 31, 1 << 31, 1 << 31) == -1
    for ws in (4, 13, 1, 0, -3):
        assert _ssim_call(lib, 1, 3, 16, 16, ws) == -1, ws
        assert b"window_size" in lib.mf_last_error()
    assert _ssim_call(lib, 1, 3, 5, 16, 11) == -1                  # ws // 2 >= H
    assert b"window_size" in lib.mf_last_error() and b"H=5" in lib.mf_last_error()
    assert _ssim_call(lib, 1, 3, 16, 2, 5) == -1                   # ws // 2 >= W
    assert b"W=2" in lib.mf_last_error()
    assert _ssim_call(lib, 1, 3, -16, 16, 3) == -1
    assert b"negative" in lib.mf_last_error()
    assert _ssim_call(lib, 1, 3, 16, 16, 3, sums=False) == -1
    assert b"sums" in lib.mf_last_error()
    assert _ssim_call(lib, 1, 3, 16, 16, 3, a=False) == -1
    assert b"null" in lib.mf_last_error()
    assert _ssim_call(lib, 1, 3, 16, 16, 3, strides=False) == -1
    assert _ssim_call(lib, 1, 3, 16, 16, 3, scratch=False) == -1


def test_sqerr_abi_validates_on_the_host():
    import moco_flow_amd._lib as L
    lib = L.lib()
    buf = (ctypes.c_double * 8)()
    p = ctypes.addressof(buf)
    assert lib.mf_sqerr_scratch_bytes(0) == 0                      # empty
    assert lib.mf_sqerr_scratch_bytes(1) == 16
    assert lib.mf_sqerr_scratch_bytes(540 * 540 * 3) > 16
    assert lib.mf_sqerr_scratch_bytes(-1) == -1
    assert b"negative" in lib.mf_last_error()
    assert lib.mf_sqerr(p, p, -5, None, 1, p, p, None) == -1
    assert b"negative" in lib.mf_last_error()
    assert lib.mf_sqerr(p, p, 6, None, 1, None, p, None) == -1
    assert b"out2" in lib.mf_last_error()
    assert lib.mf_sqerr(p, p, 6, p, 0, p, p, None) == -1
    assert b"row_len" in lib.mf_last_error()
    assert lib.mf_sqerr(p, p, 7, p, 3, p, p, None) == -1           # row_len does not divide n
    assert b"row_len" in lib.mf_last_error()
    assert lib.mf_sqerr(None, p, 6, None, 1, p, p, None) == -1
    assert b"null" in lib.mf_last_error()
    assert lib.mf_sqerr(p, p, 6, None, 1, p, None, None) == -1
