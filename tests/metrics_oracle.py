"""TEST INFRASTRUCTURE ONLY -- torch-on-the-CPU restatement of the validation metrics (models/metrics.py:4-22).

KORNIA RESTATED: ``ssim_map`` restates kornia 0.6.5's kornia.metrics.ssim.ssim(img1, img2, window_size, max_val=1.0,
eps=1e-12) from its published algorithm (kornia itself is not available here; unpinned against it, as
oracle/kornia_restated.py is for the quaternion functions):

  window   g[i] = exp(-(i - ws//2)^2 / (2 1.5^2)) normalised to sum 1, 2-D window g x g
  border   F.pad(mode='reflect') by ws//2 (the edge pixel is not repeated: index -1 -> 1, H -> H - 2)
  f        grouped F.conv2d with the 2-D window
  mu1 = f(a), mu2 = f(b), s1 = f(a^2) - mu1^2, s2 = f(b^2) - mu2^2, s12 = f(ab) - mu1 mu2
  ssim = (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2) + eps),  C1 = (0.01 max_val)^2, C2 = (0.03 max_val)^2

dtype-generic: everything is computed in the dtype of ``img1``."""
import torch
import torch.nn.functional as F


def gaussian_1d(window_size, dtype=torch.float64, sigma=1.5):
    x = torch.arange(window_size, dtype=dtype) - window_size // 2
    g = torch.exp(-(x * x) / (2.0 * sigma * sigma))
    return g / g.sum()


def reflect_index(i, n):
    """Source index of padded position i (may be < 0 or >= n) under reflect padding without repeating the edge."""
    if i < 0:
        i = -i
    if i >= n:
        i = 2 * (n - 1) - i
    return i


def ssim_map(img1, img2, window_size, max_val=1.0, eps=1e-12):
    assert img1.shape == img2.shape and img1.dim() == 4
    dtype = img1.dtype
    img2 = img2.to(dtype)
    C = img1.shape[1]
    g = gaussian_1d(window_size, dtype)
    kernel = (g[:, None] * g[None, :])[None, None].expand(C, 1, window_size, window_size).contiguous()
    r = window_size // 2
    f = lambda x: F.conv2d(F.pad(x, (r, r, r, r), mode='reflect'), kernel, groups=C)
    C1, C2 = (0.01 * max_val) ** 2, (0.03 * max_val) ** 2
    mu1, mu2 = f(img1), f(img2)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 ** 2, mu2 ** 2, mu1 * mu2
    sigma1_sq = f(img1 ** 2) - mu1_sq
    sigma2_sq = f(img2 ** 2) - mu2_sq
    sigma12 = f(img1 * img2) - mu1_mu2
    num = (2.0 * mu1_mu2 + C1) * (2.0 * sigma12 + C2)
    den = (mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2)
    return num / (den + eps)


def mse(image_pred, image_gt, valid_mask=None, reduction='mean'):
    """metrics.py:4-10."""
    value = (image_pred - image_gt) ** 2
    if valid_mask is not None:
        value = value[valid_mask]
    if reduction == 'mean':
        return torch.mean(value)
    return value


def psnr(image_pred, image_gt, valid_mask=None, reduction='mean'):
    """metrics.py:12-13."""
    return -10 * torch.log10(mse(image_pred, image_gt, valid_mask, reduction))


def frame_pair(shape, seed):
    """The GPU tests' inputs: structure plus the flat regions real frames have.  gt = 0.5 + 0.5 sin(9x + 5y) on the unit
    square, its top third 1.0 and its left quarter 0.0; pred = clamp(gt + 0.05 randn), its top quarter back to 1.0.
    (B, C, H, W) fp32, seeded; channel / batch k shifts the phase by k."""
    B, C, H, W = shape
    gen = torch.Generator().manual_seed(seed)
    y = torch.linspace(0, 1, H, dtype=torch.float64)[:, None]
    x = torch.linspace(0, 1, W, dtype=torch.float64)[None, :]
    k = torch.arange(B * C, dtype=torch.float64).view(B, C, 1, 1)
    gt = (0.5 + 0.5 * torch.sin(9 * x + 5 * y + k)).float()
    gt[:, :, : H // 3, :] = 1.0
    gt[:, :, :, : W // 4] = 0.0
    pred = (gt + 0.05 * torch.randn(shape, generator=gen)).clamp(0, 1)
    pred[:, :, : H // 4, :] = 1.0
    return pred, gt
