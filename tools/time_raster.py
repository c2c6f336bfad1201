#!/usr/bin/env python3
"""The rasterizer (moco_flow_amd.raster; scripts/data_utils.py:23-86, 273-336 without pyrender): raster.render_mesh -- projection,
mf_rasterize and one fused resolve -- on
    a closed 6 890-vertex / 13 776-triangle mesh (SMPL's counts: a body-sized ellipsoid of 82 rings x 84 segments) at 540 x 540
    and 1080 x 1080, vertex-coloured, white background, as a stage-1 view is drawn;
    a marching_cubes mesh of about 1.8 M triangles (the smooth field of tools/time_mesh.py at 512^3) at 540 x 540, headlight-shaded,
beside (a) the bytes it must move -- vertices and colours read once, triangles read once, the key plane cleared, written at least
once and read once, the five planes written once -- over the HBM copy rate measured here (a 1 GiB device-to-device copy), and (b)
the same five planes composed from eager device ops out of rasterize's face / bary planes (gathers, the weighted sum, quantise,
where, cat; nothing at the parent commit rasterizes, so that part has no eager counterpart and is timed on its own).

Per row: device time per call from HIP events around each call, 5 warm-up calls, median of 20.  No pass / fail on time.
Usage: time_raster.py [--small]   (--small: a 96^3 field instead of 512^3, for a quick look)"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import moco_flow_amd as M
from moco_flow_amd import camera, raster

dev = torch.device("cuda")


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


def body_mesh(rings=82, segs=84):
    """A closed ellipsoid with SMPL's counts: 2 + rings segs vertices, 2 rings segs triangles."""
    th = np.pi * (np.arange(rings) + 1) / (rings + 1)
    ph = 2 * np.pi * np.arange(segs) / segs
    unit = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.cos(th), np.ones(segs)), np.outer(np.sin(th), np.sin(ph))], -1)
    v = np.concatenate([[[0, 1, 0]], unit.reshape(-1, 3), [[0, -1, 0]]]) * [0.3, 0.9, 0.2]
    idx = lambda r, s: 1 + r * segs + s % segs
    t = [(0, idx(0, s + 1), idx(0, s)) for s in range(segs)]
    for r in range(rings - 1):
        for s in range(segs):
            t += [(idx(r, s), idx(r, s + 1), idx(r + 1, s)), (idx(r, s + 1), idx(r + 1, s + 1), idx(r + 1, s))]
    last = 1 + rings * segs
    t += [(last, idx(rings - 1, s), idx(rings - 1, s + 1)) for s in range(segs)]
    return torch.tensor(v, dtype=torch.float32, device=dev), torch.tensor(t, dtype=torch.int64, device=dev)


def eager_compose(face, depth, bary, tris, colors, H, W, f, c, white):
    hit = face >= 0
    vi = tris[face.clamp(min=0).long()]                                         # (H, W, 3)
    col = (bary[..., 0:1] * colors[vi[..., 0]] + bary[..., 1:2] * colors[vi[..., 1]]) + bary[..., 2:3] * colors[vi[..., 2]]
    rgb = torch.where(hit[..., None], col.mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8), white)
    rgba = torch.cat([rgb, (hit.to(torch.uint8) * 255)[..., None]], dim=-1)
    i = torch.arange(W, device=dev, dtype=torch.float32)[None, :]
    j = torch.arange(H, device=dev, dtype=torch.float32)[:, None]
    ray_t = depth * torch.sqrt(((i - c[0]) / f) ** 2 + ((j - c[1]) / f) ** 2 + 1)
    return {"rgba": rgba, "mask": hit.reshape(-1), "depth": depth, "ray_t": ray_t, "face": face}


copy_src = torch.empty(1 << 28, dtype=torch.float32, device=dev)
copy_dst = torch.empty_like(copy_src)
copy_ms = timeit(lambda: copy_dst.copy_(copy_src))[0]
rate = 2 * copy_src.numel() * 4 / (copy_ms * 1e-3)
del copy_src, copy_dst
print(f"HBM copy rate {rate / 1e12:.2f} TB/s (1 GiB device-to-device, read + write counted); ms per call: median of 20 / min / max")


def leg(name, verts, tris, colors, H, W, f, c, c2w, shading):
    V, T = verts.shape[0], tris.shape[0]
    white = torch.full((3,), 255, dtype=torch.uint8, device=dev)
    kw = dict(background=(1.0, 1.0, 1.0), shading=shading)
    med, lo, hi, out = timeit(lambda: raster.render_mesh(verts, tris, colors, H, W, f, c, c2w, **kw))
    covered = int(out["mask"].sum())
    print(f"{name}: V = {V}, T = {T}, {H} x {W}, shading {shading}; {covered} covered pixels ({covered / (H * W):.1%})")
    print(f"  render_mesh (project + mf_rasterize + mf_raster_shade)   {med:8.4f} / {lo:8.4f} / {hi:8.4f}")
    moved = V * 12 * 2 + V * 12 + T * 24 + H * W * 8 * 3 + H * W * (4 + 1 + 4 + 4 + 4)
    print(f"  bytes it must move: {moved / 1e6:.1f} MB = {moved / rate * 1e3:.4f} ms at the copy rate, {moved / rate * 1e3 / med:.3f} of the measured time")
    screen, inv_z = raster.project_vertices(verts, c2w, f, c)
    p = timeit(lambda: raster.project_vertices(verts, c2w, f, c))
    r = timeit(lambda: raster.rasterize(screen, inv_z, tris, H, W))
    print(f"  project_vertices alone                                   {p[0]:8.4f} / {p[1]:8.4f} / {p[2]:8.4f}")
    print(f"  rasterize alone (mf_rasterize + mf_raster_resolve)       {r[0]:8.4f} / {r[1]:8.4f} / {r[2]:8.4f}")
    if shading == "none":
        face, depth, bary = r[3]
        e = timeit(lambda: eager_compose(face, depth, bary, tris, colors, H, W, f, c, white))
        print(f"  the five planes from face / bary by eager device ops      {e[0]:8.4f} / {e[1]:8.4f} / {e[2]:8.4f}   (after rasterize; "
              f"with it {e[0] + r[0] + p[0]:.4f})")
        same = torch.equal(e[3]["rgba"], out["rgba"]) and torch.equal(e[3]["mask"], out["mask"])
        print(f"  eager rgba and mask equal render_mesh's: {same}")


verts, tris = body_mesh()
lo, hi = verts.min(0).values, verts.max(0).values
colors = (verts - lo) / (hi - lo)
pose = camera.look_at_pose([1.5, 0.6, 2.0], [0.0, 0.0, 0.0])
for side in (540, 1080):
    leg("SMPL-sized mesh", verts, tris, colors, side, side, 1.1 * side, (side / 2, side / 2), pose, "none")

N = 96 if "--small" in sys.argv else 512
ax = torch.linspace(0, 1, N, device=dev)
x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
vol = (torch.sin(6.0 * x + 2.0 * y * y) + torch.sin(5.0 * y + 3.0 * z) + torch.sin(7.0 * z + 4.0 * x * y)).contiguous()
del x, y, z
mv, mt = M.marching_cubes(vol, 0.3)
del vol
mv = mv / (N - 1) - 0.5
lo, hi = mv.min(0).values, mv.max(0).values
pose = camera.look_at_pose([0.9, 0.7, 1.4], [0.0, 0.0, 0.0])
leg(f"marching_cubes mesh ({N}^3 smooth field)", mv, mt, (mv - lo) / (hi - lo), 540, 540, 600.0, (270, 270), pose, "headlight")
leg(f"marching_cubes mesh ({N}^3 smooth field)", mv, mt, (mv - lo) / (hi - lo), 540, 540, 600.0, (270, 270), pose, "none")
