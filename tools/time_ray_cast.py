#!/usr/bin/env python3
"""Ray casts against a mesh (MeshIndex.corners, cast_rays: csrc/mf_mesh_rays.hip) on the smooth analytic field's marching-cubes
mesh of tools/time_mesh.py at N^3 (scaled into [-0.5, 0.5]^3 and seen by tools/time_raster.py's camera) and on the 6 890-vertex
synthetic SMPL body with its 13 776 synthetic triangles (tools/time_voxelize.py's camera: 4 in front of the box centre).

Per mesh: MeshIndex and mf_surface_corners alone; then on two ray sets -- the hull rays of one 540 x 540 camera (the filled
convex hull of the projected mesh box) and 100 000 random rays (origins uniform in the box grown by a half, directions normal) --
cast_rays in mode "first" and "any" with the cull, the share of rays that hit, the mean number of 64-triangle tiles a wave
evaluated out of the tiles there are, the full sweep where T x Q stays under 3e11 pairs (and whether it equals the cull bit for
bit), and what the time is made of: the same call on dead rays (the host plumbing alone: the Morton sort of the rays, the start
tiles, one launch that leaves at once) and on live rays whose range [t_min, t_max] no tile meets (plumbing + the scan of every
tile box, nothing evaluated).  Beside it raster.render_mesh on the same camera, whose ray_t plane is the same quantity for a
pinhole frame, and how far the two agree on the whole frame.

The times are information: nothing did this job before, and no share of a peak is claimed.  Device time per call from HIP
events around each call, 5 warm-up calls, median of 20, one process.
Usage: time_ray_cast.py [N]   (default 512; a smaller N for a quick look)"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import moco_flow_amd as M
from moco_flow_amd import _lib as L, camera, smpl as S, synth

N = int(sys.argv[1]) if len(sys.argv) > 1 else 512
H = W = 540
Q_RANDOM = 100_000
SWEEP_PAIRS = 3e11
dev = torch.device("cuda")


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


def smooth_field(n):
    ax = torch.linspace(0, 1, n, device=dev)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    vol = (torch.sin(6.0 * x + 2.0 * y * y) + torch.sin(5.0 * y + 3.0 * z) + torch.sin(7.0 * z + 4.0 * x * y)).contiguous()
    del x, y, z
    verts, tris = M.marching_cubes(vol, 0.3)
    return (verts / (n - 1) - 0.5).contiguous(), tris


def corners_alone(index):
    L.launch(dev, "mf_surface_corners", L.ptr0(index.verts), index.V, L.ptr0(index.tris), index.T, L.ptr0(index.slot_tri), L.ptr0(index.corners))


def ray_set(what, index, rays):
    Q, T = rays.shape[0], index.T
    row = f"    {what}, Q {Q}: "
    for mode in ("first", "any"):
        t = timeit(lambda: M.cast_rays(index, rays=rays, mode=mode))
        out = M.cast_rays(index, rays=rays, mode=mode, return_visited=True)
        visited = out[-1].float()
        hit = torch.isfinite(out[0]) if mode == "first" else out[0].bool()
        row += (f"{mode} {t:8.3f} ms ({float(visited.mean()):.1f} tiles evaluated per wave of 64 rays, largest {int(visited.max())}, of {index.n_tiles}; "
                f"{float(hit.float().mean()):.3f} of the rays hit); ")
    dead = rays.clone()
    dead[:, 3:6] = 0
    t_dead = timeit(lambda: M.cast_rays(index, rays=dead))
    unmet = rays.clone()
    unmet[:, 6:8] = -1e30
    t_scan = timeit(lambda: M.cast_rays(index, rays=unmet))
    assert not torch.isfinite(M.cast_rays(index, rays=unmet)[0]).any()
    row += f"dead rays {t_dead:7.3f} ms (the plumbing), a range no tile meets {t_scan:8.3f} ms (plumbing + the scan of {index.n_tiles} tile boxes); "
    if T * Q <= SWEEP_PAIRS:
        t = timeit(lambda: M.cast_rays(index, rays=rays, cull=False), warm=1, n=3)
        same = all(torch.equal(a, b) for a, b in zip(M.cast_rays(index, rays=rays, cull=False), M.cast_rays(index, rays=rays)))
        row += f"sweep {t:9.3f} ms ({T * Q / t / 1e6:.0f} G ray-triangle tests / s, median of 3; {'equal to the cull bit for bit' if same else 'DIFFERS'})"
    else:
        row += f"sweep not run ({T * Q:.2e} pairs)"
    print(row, flush=True)


def legs(what, verts, tris, pose, focal):
    t_index = timeit(lambda: M.MeshIndex(verts, tris))
    index = M.MeshIndex(verts, tris)
    index.corners
    t_corners = timeit(lambda: corners_alone(index))
    print(f"  {what}: V {len(verts)} T {len(tris)} ({index.n_tiles} tiles, {int(index.dropped_count)} dropped): MeshIndex {t_index:9.3f} ms, "
          f"mf_surface_corners {t_corners:7.3f} ms ({64 * index.n_tiles * 64 / 1e6:.1f} MB of corner rows)", flush=True)
    lo, hi = verts.amin(0).cpu().numpy().astype(np.float64), verts.amax(0).cpu().numpy().astype(np.float64)
    box = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])], dtype=np.float32)
    K = np.array([[focal, 0, W / 2], [0, focal, H / 2], [0, 0, 1]], dtype=np.float64)
    frame = camera.make_rays(H, W, focal, (W / 2, H / 2), pose[:3], 0.0, 100.0, 0.0)
    hull = frame[camera.valid_rays_mask(box, pose, K, (H, W))].contiguous()
    ray_set(f"hull rays of a {H} x {W} camera", index, hull)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    lo_t, hi_t = verts.amin(0), verts.amax(0)
    rnd = torch.empty((Q_RANDOM, 8), device=dev)
    rnd[:, 0:3] = (lo_t + hi_t) / 2 + (torch.rand((Q_RANDOM, 3), device=dev, generator=g) - 0.5) * 1.5 * (hi_t - lo_t)
    rnd[:, 3:6] = torch.randn((Q_RANDOM, 3), device=dev, generator=g)
    rnd[:, 6], rnd[:, 7] = 0.0, float("inf")
    ray_set("random rays", index, rnd)
    # the neighbour: the rasterizer on the same camera, and the whole frame cast
    white = torch.ones((len(verts), 3), device=dev)
    t_raster = timeit(lambda: M.render_mesh(verts, tris, white, H, W, focal, (W / 2, H / 2), pose))
    t_frame = timeit(lambda: M.cast_rays(index, rays=frame))
    ray_t = M.render_mesh(verts, tris, white, H, W, focal, (W / 2, H / 2), pose)["ray_t"].reshape(-1)
    t = M.cast_rays(index, rays=frame)[0]
    both = torch.isfinite(ray_t) & torch.isfinite(t)
    agree = float((torch.isfinite(ray_t) == torch.isfinite(t)).float().mean())
    diff = (ray_t - t)[both].abs()
    print(f"    the whole {H} x {W} frame: cast_rays first {t_frame:8.3f} ms, raster.render_mesh (all five planes) {t_raster:8.3f} ms; covered / hit agree on "
          f"{agree:.5f} of the pixels, |ray_t - t| median {float(diff.median()):.2e} largest {float(diff.max()):.2e} where both are finite "
          f"(the rasterizer samples a snapped 1/256-pixel projection, the cast the ray itself)", flush=True)


print(f"ray casts against a mesh: the smooth field at {N}^3 and the synthetic SMPL body; {H} x {W} camera, {Q_RANDOM} random rays", flush=True)
verts, tris = smooth_field(N)
legs(f"smooth field {N}^3", verts, tris, camera.look_at_pose([0.9, 0.7, 1.4], [0.0, 0.0, 0.0]), 600.0)
del verts, tris
torch.cuda.empty_cache()

body = S.SMPL(model=synth.smpl_model(1, 6890)).cuda()
pose, betas = synth.smpl_pose(5, batch=1, scale=0.3)
with torch.no_grad():
    verts = body(torch.from_numpy(pose).cuda(), torch.from_numpy(betas).cuda())[0].contiguous()
v = verts.cpu().numpy()
tris = torch.from_numpy(synth.smpl_faces(v)).cuda()
centre = (v.min(0) + v.max(0)) / 2
c2w = np.array([[1, 0, 0, centre[0]], [0, 1, 0, centre[1]], [0, 0, 1, centre[2] + 4.0], [0, 0, 0, 1.0]], dtype=np.float64)
legs("synthetic SMPL body", verts, tris, c2w, 1.2 * W)
