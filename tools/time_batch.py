#!/usr/bin/env python3
"""The ray batch of a training step (train_step, trainer_moco_flow.py:407-417 over datasets/moco_flow_dataset.py:166-176,
190-196): moco_flow_amd.batch.FrameRays.sample -- torch.randperm and ONE mf_ray_batch launch from the camera, the compacted
hull mask and the 8-bit RGBA frame -- beside the eager device op sequence of the reference on the same GPU: the cached
(H W, 9) ray table, composited (H W, 3) image and (H W, 3) background, then torch.nonzero, torch.randperm and three gathers
per step.  Both draw their own permutation; with one passed in, the two batches are torch.equal (checked here once).

Per row: device time per call from HIP events around each call, 5 warm-up calls, median of 20.  A batch is tens of kilobytes:
both sides are launch-bound, no fraction of any peak is meant.  Also printed: the once-per-frame set-up of each side and the
bytes each keeps on the device per cached frame.  Usage: time_batch.py [H W]  (default 540 540)"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from moco_flow_amd import FrameRays, camera

H, W = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (540, 540)
dev = torch.device("cuda")
gen = torch.Generator().manual_seed(0)
focal, center = 1.2 * W, (0.5 * W, 0.5 * H)
c2w = np.array([[0.8, 0.0, 0.6, 0.3], [0.0, 1.0, 0.0, -0.2], [-0.6, 0.0, 0.8, 2.5]], dtype=np.float32)
near, far, idx = 1.5, 4.5, 0.25
y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
mask = ((((y - 0.5 * H) / (0.45 * H)) ** 2 + ((x - 0.5 * W) / (0.3 * W)) ** 2) < 1.0).reshape(-1).to(dev)     # a standing ellipse
rgba = torch.randint(0, 256, (H, W, 4), dtype=torch.uint8, generator=gen).to(dev)
colour = torch.rand(3, generator=gen).to(dev)
nbytes = lambda *ts: sum(t.numel() * t.element_size() for t in ts)


def eager_frame():
    """What the reference's dataset caches per frame, on the device."""
    rays = camera.make_rays(H, W, focal, center, c2w, near, far, idx)
    img = rgba.permute(2, 0, 1).float().div(255)
    bkgd = colour.view(3, 1, 1).repeat(1, H, W)
    img = img[:3] * img[-1:] + bkgd * (1 - img[-1:])
    return rays, mask, img.reshape(3, -1).permute(1, 0).contiguous(), bkgd.reshape(3, -1).permute(1, 0).contiguous()


def eager_step(cache, N_rand, perm=None):
    rays, msk, rgbs, background = cache
    val_inds = torch.nonzero(msk).squeeze(1)                                   # (synchronises: the length goes to the host)
    perm = torch.randperm(val_inds.shape[0], device=dev) if perm is None else perm
    sel = val_inds[perm[:N_rand]]
    return rays[sel], rgbs[sel], background[sel], sel


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


make_frame = lambda: FrameRays(H, W, focal, center, c2w, near, far, idx, rays_msk=mask)
frame, cache = make_frame(), eager_frame()
print(f"frame {H} x {W}, {frame.n_valid} valid pixels, RGBA input; ms per call (median of 20 / min / max)")
for name, f in (("FrameRays(...)   once per frame", make_frame), ("eager tables    once per frame", eager_frame)):
    med, lo, hi, _ = timeit(f)
    print(f"  {name:44s} {med:8.4f} / {lo:8.4f} / {hi:8.4f}", flush=True)
for N_rand in (1024, 5120):
    perm = torch.randperm(frame.n_valid, device=dev)
    for a, b in zip(frame.sample(N_rand, image=rgba, background=colour, perm=perm), eager_step(cache, N_rand, perm)):
        assert torch.equal(a, b)
    for name, f in ((f"FrameRays.sample N_rand={N_rand}", lambda: frame.sample(N_rand, image=rgba, background=colour)),
                    (f"  the launch alone (perm passed)", lambda: frame.sample(N_rand, image=rgba, background=colour, perm=perm)),
                    (f"eager sequence   N_rand={N_rand}", lambda: eager_step(cache, N_rand))):
        med, lo, hi, _ = timeit(f)
        print(f"  {name:44s} {med:8.4f} / {lo:8.4f} / {hi:8.4f}", flush=True)
print(f"resident per frame: FrameRays {frame.resident_bytes()} B of val_inds + the {nbytes(rgba)} B RGBA frame and 12 B colour = "
      f"{frame.resident_bytes() + nbytes(rgba, colour)} B; eager {nbytes(*cache)} B (rays {nbytes(cache[0])}, mask {nbytes(cache[1])}, "
      f"rgbs {nbytes(cache[2])}, background {nbytes(cache[3])})")
