#!/usr/bin/env python3
"""Occupancy grids at test time (moco_flow_amd.occupancy) on tools/time_image.py's 540 x 540 set-up: MoCo bw NoF -> NeRF,
64 + 128 samples, test_time=True, the camera at z = 4 looking at the AABB [-1, 1]^3, the hull of the projected AABB as
rays_msk (Camera.get_valid_rays_mask).

  build    OccupancyGrid.from_field at 128^3 in fp32 and bf16, split into the sigma query (query_sigma on the lattice) and
           the build (from_sigma: mf_occ_build with its count)
  clip     clip_rays and cull on the hull rays of the frame (mf_ray_clip; cull adds the copy of the table)
  frame    image.render_image without a grid and with one, fp32 and bf16

The random test networks have no body-shaped field, so the grid of the frame rows comes from from_sigma of a synthetic
capsule that fills about 10 % of the box; the kept-ray fraction is printed beside the times, since the saving is that
fraction of the render and belongs to the scene.  Device time per call from HIP events around each call, 5 warm-up calls,
median of 20, one process.  Usage: time_occupancy.py [H W]  (default 540 540)"""
import functools
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import moco_flow_amd as M
from moco_flow_amd import camera, image, rendering, synth

rendering.STRICT_RNG = False
H, W = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (540, 540)
N_GRID = 128
dev = torch.device("cuda")


def load(m, sd):
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(dev)


def timeit(f, warm=5, n=20):
    for _ in range(warm):
        f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


focal = 1.2 * W
c2w = np.array([[1, 0, 0, 0.0], [0, 1, 0, 0.0], [0, 0, 1, 4.0], [0, 0, 0, 1.0]], dtype=np.float64)
K = np.array([[focal, 0, W / 2], [0, focal, H / 2], [0, 0, 1]], dtype=np.float64)
aabb = np.array([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]])
corners = np.array([[x, y, z] for x in aabb[:, 0] for y in aabb[:, 1] for z in aabb[:, 2]], dtype=np.float32)
rays = camera.make_rays(H, W, focal, (W / 2, H / 2), c2w[:3], 2.0, 6.0, -0.25)
bg = torch.ones(H * W, 3, device=dev)
msk = camera.valid_rays_mask(corners, c2w, K, (H, W))
hull = rays[msk]
n_hull = hull.shape[0]

nerfs = [load(M.NeRF(8, 256, 63, [4], "ind", 5), synth.nerf_state(0, extra_feat_type="ind", extra_feat_dim=5, regime="dense", tag=t))
         for t in ("coarse", "fine")]
nof = load(M.NoF(4, 128, 33, [2], "ind", 33, True), synth.nof_state(0, use_quat=True, tag="bw", head_scale=0.25))
nerf_embs, nof_embs = [M.Embedding(3, 10), M.Embedding(1, 2), None], [M.Embedding(3, 5), M.Embedding(1, 16)]
fwd = functools.partial(M.render_rays, nerf_embeddings=nerf_embs, nerf_models=nerfs, nof_embeddings=nof_embs, nof_models=[nof],
                        N_samples=64, N_importance=128, perturb=0, noise_std=0, test_time=True)
render = lambda r, b: fwd(r, b)

print(f"{H} x {W} frame: {n_hull} hull rays of {H * W} ({n_hull / (H * W):.3f}), lattice {N_GRID}^3, MoCo bw NoF -> NeRF, 64 + 128 samples")

# ---- build
xyz, n = M.OccupancyGrid.lattice(N_GRID, aabb, dev)
with torch.no_grad():
    for prec in ("f32", "bf16"):
        flow = dict(bw_nof=nof, nof_embeddings=nof_embs, ind=-0.25, precision=prec)
        sigma = M.query_sigma(xyz, nerfs[1], nerf_embs[0], **flow)
        t_query = timeit(lambda: M.query_sigma(xyz, nerfs[1], nerf_embs[0], **flow))
        t_build = timeit(lambda: M.OccupancyGrid.from_sigma(sigma.view(*n), aabb[0], aabb[1], 1.0, "softplus", 1))
        t_field = timeit(lambda: M.OccupancyGrid.from_field(nerfs[1], nerf_embs[0], aabb, N_GRID, 1.0, "softplus", 1, **flow))
        frac = M.OccupancyGrid.from_sigma(sigma.view(*n), aabb[0], aabb[1], 1.0, "softplus", 1).occupied_fraction()
        print(f"  build {prec:5s}: query_sigma {t_query:8.3f} ms + mf_occ_build {t_build:7.3f} ms; from_field {t_field:8.3f} ms "
              f"(random network at tau = 1: {frac:.3f} of the cells occupied)")

# ---- the capsule: a standing segment of length 1.2 and radius 0.38, 9.7 % of the box's volume
ax = [torch.linspace(-1, 1, N_GRID, device=dev, dtype=torch.float64) for _ in range(3)]
X, Y, Z = torch.meshgrid(*ax, indexing="ij")
dist = torch.sqrt(X ** 2 + (Y.abs() - 0.6).clamp_min(0) ** 2 + Z ** 2)
capsule = torch.where(dist <= 0.38, 5.0, -5.0).float()
grid = M.OccupancyGrid.from_sigma(capsule, aabb[0], aabb[1], 1.0, "softplus", 1)
print(f"  capsule grid: {grid.occupied_fraction():.3f} of the cells occupied after dilation by 1 ({float((dist <= 0.38).double().mean()):.3f} of the lattice points inside)")

# ---- clip
t_clip = timeit(lambda: grid.clip_rays(hull))
t_cull = timeit(lambda: grid.cull(hull, "both"))
hit = grid.clip_rays(hull)[2]
kept = int(hit.sum())
print(f"  clip  : clip_rays {t_clip:7.3f} ms, cull {t_cull:7.3f} ms on {n_hull} hull rays; kept {kept} = {kept / n_hull:.3f} of the hull rays")

# ---- frame
with torch.no_grad():
    for prec in ("f32", "bf16"):
        rendering.set_precision(prec)
        t_plain = timeit(lambda: image.render_image(rays, bg, render, 65536, msk))
        row = f"  frame {prec:5s}: no grid {t_plain:8.2f} ms"
        for tighten in ("none", "near", "both"):
            t_grid = timeit(lambda: image.render_image(rays, bg, render, 65536, msk, occupancy=grid, tighten=tighten))
            row += f"; grid, tighten={tighten} {t_grid:8.2f} ms ({t_grid / t_plain:.3f} x)"
        print(row + f"; kept-ray fraction {kept / n_hull:.3f}; cull (clip_rays + the table copy) = {t_cull / t_plain:.4f} of the frame without a grid")
rendering.set_precision("f32")
