#!/usr/bin/env python3
"""Occupancy grids from a mesh (OccupancyGrid.from_mesh: mf_voxel_mesh, mf_voxel_fill, mf_voxel_dilate) on the 6 890-vertex
synthetic SMPL body: posed on the device (smpl.SMPL), 13 776 synthetic triangles between neighbouring posed vertices
(synth.smpl_faces: local like a body's, NOT a closed surface -- the fill does all its work and finds nothing to fill), the box
0.25 around the vertices, thickness 0.2 as the reference's.

  mesh     at 128^3 and 256^3 cells: the surface pass, the fill, the dilation by the thickness's radii, from_mesh end to end
  field    beside it, in the same process: OccupancyGrid.from_field on a 128^3 lattice in fp32 and bf16 (MoCo bw NoF -> NeRF),
           and from_field(within=from_mesh(...)) behind a 32^3 mesh grid
  rays     the kept-ray fraction of a 540 x 540 frame's hull rays under either grid
  euclid   the exact Euclidean shell and the distance field (mf_grid_edt: squared_distance, dilated_euclidean, the three passes one
           by one from the profiler's kernel records) and from_mesh(shell="euclidean") beside the box shell at 128^3 and 256^3:
           occupied and kept-ray fractions of both shells, one frame of render_image behind each

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

# ---- the Euclidean shell and the distance field (csrc/mf_distance.hip), beside the box shell in this process
COPY_RATE = 4.69e12                                  # bytes / s of a device copy, measured (profiles/README.md)
EDT_KERNELS = ("edt_z_kernel", "edt_y_kernel", "edt_x_kernel", "edt_count_finish_kernel")


def kernel_times(f, warm=5, n=20):
    """Median device time (ms) per kernel of EDT_KERNELS over n calls of f, from the profiler's kernel records."""
    from torch.profiler import ProfilerActivity, profile
    for _ in range(warm):
        f()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(n):
            f()
        torch.cuda.synchronize()
    seen = {k: [] for k in EDT_KERNELS}
    for ev in prof.events():
        for k in EDT_KERNELS:
            if k in ev.name:
                seen[k].append(ev.device_time / 1e3)
    return {k: statistics.median(v) for k, v in seen.items() if v}


def kept_fraction(grid):
    return int(grid.clip_rays(hull)[2].sum()) / hull.shape[0]


shells = {}
for dims in (128, 256):
    body = M.OccupancyGrid.from_mesh(verts, tris, aabb, dims, dilate=0, thickness=0.0, solid=True)       # surface + fill
    w, R, r = M.OccupancyGrid.euclid_metric(body.cell, THICKNESS)
    cells = dims ** 3
    t_d2 = timeit(lambda: body.squared_distance(THICKNESS))
    t_shell = timeit(lambda: body.dilated_euclidean(THICKNESS))
    print(f"  euclid {dims}^3: w {w}, R {R}, reach {r} cells; squared_distance {t_d2:7.3f} ms, dilated_euclidean {t_shell:7.3f} ms")
    try:
        per = kernel_times(lambda: body.dilated_euclidean(THICKNESS))
        bytes_of = {"edt_z_kernel": cells / 8 + 2 * cells, "edt_y_kernel": 2 * cells + 4 * cells, "edt_x_kernel": 4 * cells + cells / 8}
        print("           passes of dilated_euclidean: " + "; ".join(
            f"{k} {per[k]:.4f} ms" + (f" ({bytes_of[k] / 1e6:.1f} MB algorithmic = {bytes_of[k] / COPY_RATE * 1e3:.4f} ms at the copy rate; "
                                      f"the windows are cache traffic)" if k in bytes_of else "") for k in EDT_KERNELS if k in per))
    except Exception as e:                           # the profiler is a measuring aid: without it the passes are not split
        print(f"           passes of dilated_euclidean: not measured ({type(e).__name__}: {e})")
    kw = dict(dims=dims, dilate=1, thickness=THICKNESS)
    t_box = timeit(lambda: M.OccupancyGrid.from_mesh(verts, tris, aabb, **kw))
    t_euc = timeit(lambda: M.OccupancyGrid.from_mesh(verts, tris, aabb, shell="euclidean", **kw))
    box = M.OccupancyGrid.from_mesh(verts, tris, aabb, **kw)
    euc = M.OccupancyGrid.from_mesh(verts, tris, aabb, shell="euclidean", **kw)
    inside_box = bool(((euc.bits & ~box.bits) == 0).all())
    print(f"           from_mesh box {t_box:7.3f} ms, euclidean {t_euc:7.3f} ms; occupied {box.occupied_fraction():.4f} / {euc.occupied_fraction():.4f} "
          f"of the cells (euclidean / box = {euc.occupied_fraction() / box.occupied_fraction():.3f}; inside the box shell: {inside_box}); kept hull rays "
          f"{kept_fraction(box):.3f} / {kept_fraction(euc):.3f}")
    shells[dims] = (box, euc)

from moco_flow_amd import image
coarse_nerf = load(M.NeRF(8, 256, 63, [4], "ind", 5), synth.nerf_state(0, extra_feat_type="ind", extra_feat_dim=5, regime="dense", tag="coarse"))
render = lambda r, b: M.render_rays(r, b, nerf_embeddings=[nerf_emb, M.Embedding(1, 2), None], nerf_models=[coarse_nerf, nerf], nof_embeddings=nof_embs,
                                    nof_models=[nof], N_samples=64, N_importance=128, perturb=0, noise_std=0, test_time=True)
bg = torch.ones(H * W, 3, device=dev)
msk = camera.valid_rays_mask(corners, c2w, K, (H, W))
with torch.no_grad():
    t_plain = timeit(lambda: image.render_image(rays, bg, render, 65536, msk), warm=2, n=5)
    row = f"  frame f32, MoCo bw NoF -> NeRF, 64 + 128 samples: no grid {t_plain:8.2f} ms"
    for name, grid in zip(("box", "euclidean"), shells[N_GRID]):
        t_grid = timeit(lambda: image.render_image(rays, bg, render, 65536, msk, occupancy=grid), warm=2, n=5)
        row += f"; behind the {name} shell at {N_GRID}^3 {t_grid:8.2f} ms ({t_grid / t_plain:.3f} x, kept {kept_fraction(grid):.3f})"
    print(row + " (median of 5 after 2 warm-ups)")
