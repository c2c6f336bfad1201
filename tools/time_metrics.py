#!/usr/bin/env python3
"""Frame scoring (val_step, trainer_moco_flow.py:453-473): moco_flow_amd.metrics.image_metrics on a 540 x 540 frame pair
held as (H W, 3) rows -- mse, psnr and ssim from one mf_ssim launch -- beside the same arithmetic as the eager op sequence
of the restated reference (models/metrics.py:4-22 with kornia 0.6.5's ssim restated: permute to (1, 3, H, W), reflect pad,
five grouped conv2d, the elementwise formula, two means) on the same GPU.

Per row: device time per call from HIP events around each call, 5 warm-up calls, median of 20.  The frame pair is 7 MB:
both sides are launch-bound, no fraction of any peak is meant.  Usage: time_metrics.py [H W]  (default 540 540)"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from moco_flow_amd import metrics

H, W = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (540, 540)
dev = torch.device("cuda")
gen = torch.Generator().manual_seed(0)
y = torch.linspace(0, 1, H)[:, None, None]
x = torch.linspace(0, 1, W)[None, :, None]
gt = (0.5 + 0.5 * torch.sin(9 * x + 5 * y + torch.arange(3.0))).reshape(H * W, 3)
pred = (gt + 0.05 * torch.randn(gt.shape, generator=gen)).clamp(0, 1)
gt, pred = gt.to(dev), pred.to(dev)


def eager(pred_rows, gt_rows, ws=3):
    a = pred_rows.view(H, W, 3).permute(2, 0, 1)[None]
    b = gt_rows.view(H, W, 3).permute(2, 0, 1)[None]
    g = torch.exp(-(torch.arange(ws, device=dev, dtype=torch.float32) - ws // 2) ** 2 / (2 * 1.5 ** 2))
    g = g / g.sum()
    k = (g[:, None] * g[None, :])[None, None].expand(3, 1, ws, ws).contiguous()
    f = lambda t: F.conv2d(F.pad(t, (ws // 2,) * 4, mode='reflect'), k, groups=3)
    mu1, mu2 = f(a), f(b)
    s1, s2, s12 = f(a * a) - mu1 ** 2, f(b * b) - mu2 ** 2, f(a * b) - mu1 * mu2
    m = ((2 * mu1 * mu2 + 1e-4) * (2 * s12 + 9e-4)) / ((mu1 ** 2 + mu2 ** 2 + 1e-4) * (s1 + s2 + 9e-4) + 1e-12)
    e = torch.mean((pred_rows - gt_rows) ** 2)
    return {'mse': e, 'psnr': -10 * torch.log10(e), 'ssim': torch.mean(m)}


def timeit(f, warm=5, n=20):
    for _ in range(warm):
        out = f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = f()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts), max(ts), out


print(f"frame pair {H} x {W} x 3 fp32 rows, window 3; ms per call (median of 20 / min / max)")
for name, f in (("image_metrics (one mf_ssim launch)", lambda: metrics.image_metrics(pred, gt, H, W)),
                ("eager restatement", lambda: eager(pred, gt))):
    med, lo, hi, out = timeit(f)
    print(f"  {name:36s} {med:8.4f} / {lo:8.4f} / {hi:8.4f}   mse {out['mse'].item():.6e} psnr {out['psnr'].item():.4f} "
          f"ssim {out['ssim'].item():.6f}", flush=True)
