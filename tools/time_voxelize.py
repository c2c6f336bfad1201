#!/usr/bin/env python3
"""Occupancy grids from a mesh (OccupancyGrid.from_mesh: mf_voxel_mesh, mf_voxel_fill, mf_voxel_dilate) on the 6 890-vertex
synthetic SMPL body: posed on the device (smpl.SMPL), 13 776 synthetic triangles between neighbouring posed vertices
(synth.smpl_faces: local like a body's, NOT a closed surface -- the fill does all its work and finds nothing to fill), the box
0.25 around the vertices, thickness 0.2 as the reference's.

  mesh     at 128^3 and 256^3 cells: the surface pass, the fill, the dilation by the thickness's radii, from_mesh end to end
  field    beside it, in the same process: OccupancyGrid.from_field on a 128^3 lattice in fp32 and bf16 (MoCo bw NoF -> NeRF),
           and from_field(within=from_mesh(...)) behind a 32^3 mesh grid
  rays     the kept-ray fraction of a 540 x 540 frame's hull rays under either grid

The times are information: nothing did this job before.  The surface pass is integer atomics and the fill chases parents; neither
is held against a peak.  Device time per call from HIP events around each call, 5 warm-up calls, median of 20, one process."""
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import moco_flow_amd as M
from moco_flow_amd import _lib as L, camera, smpl as S, synth

H = W = 540
N_GRID = 128
THICKNESS = 0.2
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


def f3(v):
    return (ctypes.c_float * 3)(*[float(x) for x in v])


body = S.SMPL(model=synth.smpl_model(1, 6890)).cuda()
pose, betas = synth.smpl_pose(5, batch=1, scale=0.3)
with torch.no_grad():
    verts = body(torch.from_numpy(pose).cuda(), torch.from_numpy(betas).cuda())[0].contiguous()
v = verts.cpu().numpy()
faces = synth.smpl_faces(v)
tris = torch.from_numpy(faces).cuda()
aabb = np.stack([v.min(0) - 0.25, v.max(0) + 0.25]).astype(np.float64)
edge = np.linalg.norm(v[faces[:, 0]] - v[faces[:, 1]], axis=1)
print(f"synthetic SMPL: {len(v)} vertices, {len(tris)} triangles (mean edge {edge.mean():.4f}, longest {edge.max():.4f}), box "
      f"{np.round(aabb[1] - aabb[0], 3).tolist()}, thickness {THICKNESS}")

lib = L.lib()
for dims in (128, 256):
    g3 = (dims,) * 3
    surface = M.OccupancyGrid.from_mesh(verts, tris, aabb, dims, dilate=0, thickness=0.0, solid=False)
    radii = tuple(1 + int(np.ceil(THICKNESS / c)) for c in surface.cell)
    bits = torch.empty_like(surface.bits)
    stream = L.current_stream(dev)
    t_surface = timeit(lambda: lib.mf_voxel_mesh(verts.data_ptr(), len(v), tris.data_ptr(), len(tris), *g3, f3(surface.lo), f3(surface.hi),
                                                 f3(surface.inv_cell), bits.data_ptr(), None, stream))
    assert torch.equal(bits, surface.bits)
    t_fill = timeit(lambda: surface.filled())
    t_dilate = timeit(lambda: surface.dilated(radii))
    t_all = timeit(lambda: M.OccupancyGrid.from_mesh(verts, tris, aabb, dims, dilate=1, thickness=THICKNESS))
    grid = M.OccupancyGrid.from_mesh(verts, tris, aabb, dims, dilate=1, thickness=THICKNESS)
    print(f"  mesh {dims}^3: surface {t_surface:7.3f} ms ({surface.occupied_fraction():.4f} of the cells), fill {t_fill:7.3f} ms, dilation by "
          f"{radii} {t_dilate:7.3f} ms, from_mesh {t_all:7.3f} ms ({grid.occupied_fraction():.3f} of the cells)")
    if dims == N_GRID:
        mesh_grid = grid

nerf = load(M.NeRF(8, 256, 63, [4], "ind", 5), synth.nerf_state(0, extra_feat_type="ind", extra_feat_dim=5, regime="dense", tag="fine"))
nof = load(M.NoF(4, 128, 33, [2], "ind", 33, True), synth.nof_state(0, use_quat=True, tag="bw", head_scale=0.25))
nerf_emb, nof_embs = M.Embedding(3, 10), [M.Embedding(3, 5), M.Embedding(1, 16)]
coarse = M.OccupancyGrid.from_mesh(verts, tris, aabb, 32, dilate=1, thickness=THICKNESS)
with torch.no_grad():
    for prec in ("f32", "bf16"):
        kw = dict(N_grid=N_GRID, sigma_threshold=1.0, bw_nof=nof, nof_embeddings=nof_embs, ind=-0.25, precision=prec)
        t_field = timeit(lambda: M.OccupancyGrid.from_field(nerf, nerf_emb, aabb, **kw))
        t_within = timeit(lambda: M.OccupancyGrid.from_field(nerf, nerf_emb, aabb, within=coarse, **kw))
        field_grid = M.OccupancyGrid.from_field(nerf, nerf_emb, aabb, **kw)
        print(f"  field {prec:5s}: from_field {t_field:8.3f} ms; from_field(within=from_mesh at 32^3, {coarse.occupied_fraction():.3f} of its cells) "
              f"{t_within:8.3f} ms (random network at tau = 1: {field_grid.occupied_fraction():.3f} of the cells occupied)")

centre = aabb.mean(0)
focal = 1.2 * W
c2w = np.array([[1, 0, 0, centre[0]], [0, 1, 0, centre[1]], [0, 0, 1, centre[2] + 4.0], [0, 0, 0, 1.0]], dtype=np.float64)
K = np.array([[focal, 0, W / 2], [0, focal, H / 2], [0, 0, 1]], dtype=np.float64)
corners = np.array([[x, y, z] for x in aabb[:, 0] for y in aabb[:, 1] for z in aabb[:, 2]], dtype=np.float32)
rays = camera.make_rays(H, W, focal, (W / 2, H / 2), c2w[:3], 2.0, 6.0, -0.25)
hull = rays[camera.valid_rays_mask(corners, c2w, K, (H, W))]
for name, grid in (("from_mesh", mesh_grid), ("from_field", field_grid)):
    t_clip = timeit(lambda: grid.clip_rays(hull))
    kept = int(grid.clip_rays(hull)[2].sum())
    print(f"  rays  : {name:10s} at {grid.dims[0]}^3: kept {kept} of {hull.shape[0]} hull rays of the {H} x {W} frame = {kept / hull.shape[0]:.3f} "
          f"(clip_rays {t_clip:6.3f} ms)")
