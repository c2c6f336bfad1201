#!/usr/bin/env python3
"""Mesh-to-mesh distances (MeshIndex, closest_point, sample_surface, surface_distance: csrc/mf_mesh_distance.hip) on the two
marching-cubes meshes of tools/time_mesh.py at N^3 (the f32 sigma lattice of the test NeRF at threshold 10; the smooth analytic
field at 0.3) and on the 6 890-vertex synthetic SMPL body with its 13 776 synthetic triangles (tools/time_voxelize.py).

Per mesh: MeshIndex (the Morton sort, mf_surface_records, the weights and their running sum) and mf_surface_records alone;
closest_point on Q = 100 000 queries (surface samples displaced by a normal draw of one lattice step) in mode "cull", the mean
number of 64-triangle tiles a wave evaluated out of the tiles there are, and mode "sweep" where T x Q stays under 3e11 pairs; sample_surface;
surface_distance beside mf_knn1 (point-to-vertex, brute force) on the same counts; and the deviation that simplify_mesh (cell = 4
lattice steps) and smooth_mesh (10 Taubin iterations) introduce, as surface_distance between the mesh and its edit (mean, rms and
the largest sampled distance in both directions, in lattice steps).  On the SMPL body: the same legs, and the share of a
synthetic surface (the smooth field's mesh at 128^3, scaled into the body's box) within thickness 0.05 / 0.1 / 0.2 of the body --
synthetic fields, not a trained checkpoint: the figures show the measurement, they validate no thickness.

The times are information: nothing did this job before, and no share of a peak is claimed.  Device time per call from HIP
events around each call, 5 warm-up calls, median of 20, one process.
Usage: time_mesh_distance.py [N]   (default 512; a smaller N for a quick look)"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import moco_flow_amd as M
from moco_flow_amd import _lib as L, smpl as S, synth

N = int(sys.argv[1]) if len(sys.argv) > 1 else 512
Q = 100_000
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


def field_meshes(n):
    sd = synth.nerf_state(0, regime="dense")
    sd["sigma.weight"] = sd["sigma.weight"] * np.float32(3.0)
    nerf = M.NeRF(8, 256, 63, [4], "dir", 27)
    nerf.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    nerf = nerf.to(dev)
    with torch.no_grad():
        xyz = M.mesh.lattice(n, dev)
        vol = M.query_sigma(xyz, nerf, M.Embedding(3, 10)).view(n, n, n)
        del xyz
    yield ("test NeRF sigma at 10",) + M.marching_cubes(vol, 10.0, clamp_zero=True)
    del vol
    torch.cuda.empty_cache()
    yield ("smooth field",) + smooth_field(n)


def smooth_field(n):
    ax = torch.linspace(0, 1, n, device=dev)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    vol = (torch.sin(6.0 * x + 2.0 * y * y) + torch.sin(5.0 * y + 3.0 * z) + torch.sin(7.0 * z + 4.0 * x * y)).contiguous()
    return M.marching_cubes(vol, 0.3)


def records_alone(index):
    L.launch(dev, "mf_surface_records", L.ptr0(index.verts), index.V, L.ptr0(index.tris), index.T, L.ptr0(index.order), L.ptr0(index.records),
             L.ptr0(index.edges), L.ptr0(index.slot_tri), L.ptr0(index.tile_box), L.ptr0(index.tri_slot), L.ptr0(index.area2),
             L.ptr0(index.normal), L.ptr0(index.dropped), index.dropped_count.data_ptr())


def deviation(what, a, b, unit):
    out = M.surface_distance(a, b, n=Q)
    print(f"    {what}: " + "; ".join(f"{k} mean {float(out[k]['mean']):.4f} rms {float(out[k]['rms']):.4f} max {float(out[k]['max']):.4f}"
                                     for k in ("a2b", "b2a")) + f"; chamfer {float(out['chamfer']):.4f} ({unit}; a = the mesh, b = its edit; "
          f"{Q} samples each way; normal consistency {float(out['a2b']['normal_consistency']):.4f} / {float(out['b2a']['normal_consistency']):.4f})", flush=True)


def legs(what, verts, tris, step, unit, edits=True):
    V, T = len(verts), len(tris)
    t_index = timeit(lambda: M.MeshIndex(verts, tris))
    index = M.MeshIndex(verts, tris)
    t_records = timeit(lambda: records_alone(index))
    print(f"  {what}: V {V} T {T} ({index.n_tiles} tiles, {int(index.dropped_count)} dropped): MeshIndex {t_index:9.3f} ms, mf_surface_records alone "
          f"{t_records:9.3f} ms ({112 * index.n_tiles * 64 / 1e6:.1f} MB of records and edge rows)", flush=True)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    t_sample = timeit(lambda: M.sample_surface(index, Q, generator=g))
    points, _ = M.sample_surface(index, Q, generator=g)
    q = (points + torch.randn(points.shape, device=dev, generator=g) * step).contiguous()
    row = f"    closest_point, Q {Q}: "
    t = timeit(lambda: M.closest_point(q, index))
    row += f"cull {t:9.3f} ms, "
    visited = M.closest_point(q, index, return_visited=True)[3].float()
    row += f"{float(visited.mean()):.1f} tiles evaluated per wave of 64 queries (largest {int(visited.max())}) of {index.n_tiles}; "
    if T * Q <= SWEEP_PAIRS:
        t = timeit(lambda: M.closest_point(q, index, mode="sweep"), warm=2, n=5)
        same = all(torch.equal(a, b) for a, b in zip(M.closest_point(q, index, mode="sweep"), M.closest_point(q, index)))
        row += f"sweep {t:9.3f} ms ({T * Q / t / 1e6:.0f} G point-triangle values / s, median of 5; {'equal to the cull bit for bit' if same else 'DIFFERS'})"
    else:
        row += f"sweep not run ({T * Q:.2e} pairs)"
    print(row + f"; sample_surface({Q}) {t_sample:7.3f} ms", flush=True)
    t_sd = timeit(lambda: M.surface_distance(index, index, n=Q), warm=2, n=5)
    d, i = torch.empty((Q, 1), device=dev), torch.empty((Q, 1), dtype=torch.int64, device=dev)
    t_knn = timeit(lambda: L.launch(dev, "mf_knn1", verts.data_ptr(), V, q.data_ptr(), Q, d.data_ptr(), i.data_ptr()), warm=2, n=5)
    print(f"    surface_distance(mesh, itself, n = {Q}): {t_sd:9.3f} ms (two directions: samples, search, statistics; median of 5); mf_knn1 on "
          f"{Q} queries against the {V} vertices {t_knn:9.3f} ms (one direction, point-to-vertex, brute force)", flush=True)
    if edits:
        sv, st = M.simplify_mesh(verts, tris, 4.0)
        deviation(f"simplify_mesh(cell = 4 steps): V {V} -> {len(sv)}, T {T} -> {len(st)}", index, (sv, st), unit)
        del sv, st
        deviation("smooth_mesh(10 Taubin iterations)", index, (M.smooth_mesh(verts, tris, iterations=10), tris), unit)
    return index


print(f"mesh distances at {N}^3 (coordinates in lattice steps) and on the synthetic SMPL body; Q = {Q}", flush=True)
for what, verts, tris in field_meshes(N):
    if len(tris) > 40_000_000:
        print(f"  {what}: V {len(verts)} T {len(tris)}: not measured (above 4e7 triangles: the random network's sigma is noise at this size)", flush=True)
    else:
        legs(f"{what} {N}^3", verts, tris, 1.0, "lattice steps")
    del verts, tris
    torch.cuda.empty_cache()

body = S.SMPL(model=synth.smpl_model(1, 6890)).cuda()
pose, betas = synth.smpl_pose(5, batch=1, scale=0.3)
with torch.no_grad():
    verts = body(torch.from_numpy(pose).cuda(), torch.from_numpy(betas).cuda())[0].contiguous()
v = verts.cpu().numpy()
tris = torch.from_numpy(synth.smpl_faces(v)).cuda()
smpl_index = legs("synthetic SMPL body", verts, tris, 0.01, "world units", edits=False)
sv, st = smooth_field(128)
lo, hi = verts.amin(0) - 0.1, verts.amax(0) + 0.1
sv = (lo + sv / 127.0 * (hi - lo)).contiguous()
tau = (0.05, 0.1, 0.2)
out = M.surface_distance((sv, st), smpl_index, n=Q, thresholds=tau)
share = (out["a2b"]["within"].double() / out["a2b"]["finite"]).tolist()
print(f"  thickness: the smooth field's mesh at 128^3 (V {len(sv)} T {len(st)}) scaled into the body's box grown by 0.1: the share of its surface "
      f"within {tau} of the body = " + " / ".join(f"{s:.4f}" for s in share) + f" (mean distance {float(out['a2b']['mean']):.4f}; F-scores "
      + " / ".join(f"{s:.4f}" for s in out["fscore"].tolist()) + "; SYNTHETIC fields, not a trained checkpoint: no thickness is validated by this)")
