"""Validation metrics on the device (reference: models/metrics.py:4-22, called per image by val_step,
trainer_moco_flow.py:453-473): ``mse``, ``psnr`` and ``ssim`` with the reference's signatures, and ``image_metrics``, which
scores a rendered frame -- all three numbers -- in one mf_ssim launch on the (H W, 3) rows render_image / render_rays
produced, without a permute copy and without a host sync.

The reference's ssim is kornia 0.6.5's ``kornia.metrics.ssim.ssim``.  KORNIA RESTATED: kornia is not available to this
project; mf_ssim (include/mocoflow_hip.h) restates the published algorithm and is unpinned against kornia itself.

No gradients: the reference evaluates these under no_grad; inputs that require grad are detached.  Everything runs on the
current stream of the inputs' device."""
import ctypes as C

import torch

from . import _lib as L

__all__ = ["mse", "psnr", "ssim", "image_metrics"]


def _pair(image_pred, image_gt, what):
    L.require_gpu(image_pred, what)
    L.require_gpu(image_gt, what)
    if image_pred.shape != image_gt.shape:
        raise RuntimeError(f"moco_flow_amd.{what}: shapes differ, {tuple(image_pred.shape)} and {tuple(image_gt.shape)}")
    if image_pred.device != image_gt.device:
        raise RuntimeError(f"moco_flow_amd.{what}: inputs on {image_pred.device} and {image_gt.device}")
    return image_pred.detach().float(), image_gt.detach().float()


def _row_len(value_shape, valid_mask, what):
    """Elements of the value per mask entry: the mask has the value's shape or its leading dimensions."""
    if valid_mask.dtype != torch.bool:
        raise RuntimeError(f"moco_flow_amd.{what}: valid_mask must be a bool tensor, got {valid_mask.dtype}")
    k = valid_mask.dim()
    if tuple(valid_mask.shape) != tuple(value_shape[:k]):
        raise RuntimeError(f"moco_flow_amd.{what}: valid_mask {tuple(valid_mask.shape)} is neither the value's shape "
                           f"{tuple(value_shape)} nor its leading dimensions")
    n = 1
    for s in value_shape[k:]:
        n *= s
    return n


def _sqerr(a, b, valid_mask, what):
    """Device double[2] = [sum of (a - b)^2 over the selected elements, their count] (mf_sqerr)."""
    a, b = a.contiguous(), b.contiguous()
    n = a.numel()
    mask, row_len = None, 1
    if valid_mask is not None:
        row_len = _row_len(a.shape, valid_mask, what)
        mask = valid_mask.to(a.device).contiguous().view(torch.uint8)
    out = torch.empty(2, dtype=torch.float64, device=a.device)
    scratch = L.scratch(a.device, "mf_sqerr_scratch_bytes", n)
    L.launch(a.device, "mf_sqerr", a.data_ptr(), b.data_ptr(), n, L.ptr(mask), max(row_len, 1), out.data_ptr(), scratch.data_ptr())
    return out


def mse(image_pred, image_gt, valid_mask=None, reduction='mean'):
    """metrics.py:4-10.  'mean': 0-dim fp32 device tensor, sum / count in float64 through mf_sqerr (nan when the mask selects
    nothing, as torch.mean of an empty tensor).  Any other reduction: the elementwise (pred - gt)^2, masked or not."""
    a, b = _pair(image_pred, image_gt, "mse")
    if reduction == 'mean':
        out = _sqerr(a, b, valid_mask, "mse")
        return (out[0] / out[1]).float()
    value = (a - b) ** 2
    if valid_mask is not None:
        value = value[valid_mask]
    return value


def psnr(image_pred, image_gt, valid_mask=None, reduction='mean'):
    """metrics.py:12-13."""
    return -10 * torch.log10(mse(image_pred, image_gt, valid_mask, reduction))


def _ssim_launch(a, a_strides, b, b_strides, shape, window_size, max_val, want_map):
    """mf_ssim on two strided fp32 images -> (map or None, device double[2] = [sum ssim, sum (a - b)^2])."""
    B, Cn, H, W = shape
    dev = a.device
    scratch = L.scratch(dev, "mf_ssim_scratch_bytes", B, Cn, H, W)
    sums = torch.empty(2, dtype=torch.float64, device=dev)
    out = torch.empty(shape, dtype=torch.float32, device=dev) if want_map else None
    L.launch(dev, "mf_ssim", a.data_ptr(), (C.c_int64 * 4)(*a_strides), b.data_ptr(), (C.c_int64 * 4)(*b_strides), B, Cn, H, W,
             int(window_size), float(max_val), 1e-12, L.ptr(out), sums.data_ptr(), scratch.data_ptr())
    return out, sums


def ssim(image_pred, image_gt, reduction='mean', *, window_size=3, max_val=1.0):
    """metrics.py:15-22: image_pred and image_gt (B, C, H, W) of any strides (neither is copied), Gaussian window 3 as the
    reference.  'mean': the mean of the SSIM map as a 0-dim fp32 device tensor; the map is not materialised.  Any other
    reduction: 1 - 2 map, the reference's line 22 as written."""
    a, b = _pair(image_pred, image_gt, "ssim")
    if a.dim() != 4:
        raise RuntimeError(f"moco_flow_amd.ssim: images must be (B, C, H, W), got shape {tuple(a.shape)}")
    want_map = reduction != 'mean'
    out, sums = _ssim_launch(a, a.stride(), b, b.stride(), tuple(a.shape), window_size, max_val, want_map)
    if want_map:
        return 1 - 2 * out
    return (sums[0] / a.numel()).float()


def image_metrics(pred_rows, gt_rows, H, W, window_size=3):
    """What val_step reports for one frame, from ONE mf_ssim launch: pred_rows, gt_rows (H W, 3) rows in the order
    render_image / render_rays produce them (pixel-major, channel last; any row / channel strides, not copied) ->
    {'mse', 'psnr', 'ssim'} as 0-dim fp32 device tensors, equal to mse / psnr on the rows and ssim on
    rows.view(H, W, 3).permute(2, 0, 1)[None].  No host sync."""
    a, b = _pair(pred_rows, gt_rows, "image_metrics")
    if a.dim() != 2 or a.shape[0] != H * W:
        raise RuntimeError(f"moco_flow_amd.image_metrics: rows must be (H*W, C) = ({H * W}, C), got {tuple(a.shape)}")
    Cn = a.shape[1]
    strides = lambda t: (0, t.stride(1), W * t.stride(0), t.stride(0))
    _, sums = _ssim_launch(a, strides(a), b, strides(b), (1, Cn, H, W), window_size, 1.0, False)
    mean = sums / a.numel()
    m = mean[1].float()
    return {'mse': m, 'psnr': -10 * torch.log10(m), 'ssim': mean[0].float()}
