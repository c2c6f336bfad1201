#!/usr/bin/env python3
"""Mesh extraction (visualize_mesh, trainer_moco_flow.py:485-548): marching_cubes alone at 256^3 and 512^3 on the raw
sigma lattice of synth.nerf_state(0, regime="dense") at threshold 10 (sigma head x 3: unscaled, that NeRF's sigma stays
below 10 and the mesh is empty -- tests/golden/gen_mesh_golden.py), and extract_mesh end to end per precision.

Per row: wall time per call (host clock around calls that end in a device synchronise, 2 warm-up calls, median of 5),
V and T, the mesh bytes written (12 V + 24 T), and the volume bytes read (4 B x N^3, the two passes counted once: what
any isosurface step must read) over that time, as a fraction of the 6.29 TB/s measured HBM copy rate
(MI355X_MICROARCH.md).  marching_cubes includes its one device -> host read of the counts and the scratch / output
allocations.  A smooth analytic field at each size shows the cost of the volume read when the mesh is small (the random
NeRF's sigma makes ~10^8 triangles at 512^3).

The components leg (mesh_components / filter_components: what follows an isosurface at a fixed threshold), on both fields of
each size: the labelling (mf_mesh_label), the table (mf_mesh_table_count, its read, mf_mesh_table_emit) and the filter to the
largest component (mf_mesh_filter_plan, its read, mf_mesh_filter_emit, the vertex gather) timed separately, then
filter_components end to end, beside marching_cubes on the same volume and, for the NeRF, the sigma query.  Algorithmic
bytes: 24 B per triangle read + 4 B per vertex of labels (the labelling), the compacted outputs 12 B per kept vertex + 24 B
per kept triangle (the filter), each over its time as a fraction of the 4.69 TB/s device-to-device copy rate -- information
only: the accesses to the parents are random and no share of a peak is claimed.  The host path these replace, in the same
process where scipy is importable: the device -> host copy of the mesh, scipy.sparse.csgraph.connected_components, a numpy
re-index to the largest component (once each; --no-host skips it).  --sparse: only extract_mesh end to end, without and behind
an occupancy grid (query_sigma_lattice; the timings beside tools/time_lattice.py --sparse).  Usage: time_mesh.py [--no-host]
[--components-only] [--sparse] [N ...]  (default 256 512)"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import moco_flow_amd as M
from moco_flow_amd import synth

COPY_RATE = 6.29e12
D2D_COPY_RATE = 4.69e12
HOST = "--no-host" not in sys.argv
COMPONENTS_ONLY = "--components-only" in sys.argv
Ns = [int(a) for a in sys.argv[1:] if not a.startswith("--")] or [256, 512]
dev = torch.device("cuda")
sd = synth.nerf_state(0, regime="dense")
sd["sigma.weight"] = sd["sigma.weight"] * np.float32(3.0)
nerf = M.NeRF(8, 256, 63, [4], "dir", 27)
nerf.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
nerf = nerf.to(dev)
emb = M.Embedding(3, 10)


def timeit(f, warm=2, n=5):
    for _ in range(warm):
        out = f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        t = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    return statistics.median(ts) * 1e3, out


def row(what, N, ms, out):
    v, t = out
    gbs = 4 * N ** 3 / (ms * 1e-3)
    out_gb = (12 * len(v) + 24 * len(t)) / 1e9
    print(f"  {what:34s} {N:4d}^3: {ms:9.3f} ms  V {len(v):10d}  T {len(t):10d}  volume {gbs / 1e9:8.1f} GB/s "
          f"= {gbs / COPY_RATE:.3f} of the copy rate; mesh written {out_gb:.2f} GB", flush=True)


def host_path(verts, tris):
    """The host round trip: copy, scipy's connected components, numpy re-index to the largest; each timed once."""
    try:
        from scipy import sparse
        from scipy.sparse import csgraph
    except ImportError:
        print("    host path: scipy is not importable here, no comparison", flush=True)
        return
    t0 = time.perf_counter()
    v, t = verts.cpu().numpy(), tris.cpu().numpy()
    t1 = time.perf_counter()
    V = len(v)
    e0, e1 = np.concatenate([t[:, 0], t[:, 1]]).astype(np.int32), np.concatenate([t[:, 1], t[:, 2]]).astype(np.int32)
    graph = sparse.coo_matrix((np.ones(len(e0), np.int8), (e0, e1)), shape=(V, V)).tocsr()
    n, lab = csgraph.connected_components(graph, directed=False)
    t2 = time.perf_counter()
    del graph, e0, e1
    big = np.bincount(lab[t[:, 0]], minlength=n).argmax()
    vkeep = lab == big
    remap = np.cumsum(vkeep) - 1
    kv, kt = v[vkeep], remap[t[vkeep[t[:, 0]]]]
    t3 = time.perf_counter()
    print(f"    host path: device -> host copy {1e3 * (t1 - t0):10.1f} ms, scipy connected_components (graph build included) "
          f"{1e3 * (t2 - t1):10.1f} ms, numpy re-index {1e3 * (t3 - t2):10.1f} ms: {n} components, kept V {len(kv)} T {len(kt)}",
          flush=True)


def components_leg(what, N, verts, tris, mc_ms, sigma_ms=None):
    V, T = len(verts), len(tris)
    counts = torch.empty(3, dtype=torch.int64, device=dev)
    ms_label, labels = timeit(lambda: M.mesh._label(tris, V, counts))
    ms_table, (ids, tri_counts, vert_counts) = timeit(lambda: M.mesh._table(tris, V, labels, counts, "time_mesh"))
    keep = M.mesh._keep(ids, tri_counts, V, T, 1, None)
    ms_filter, (kv, kt) = timeit(lambda: M.mesh._filter(verts, tris, labels, ids, keep))
    ms_all, _ = timeit(lambda: M.filter_components(verts, tris, keep_largest=1))
    b_label, b_out = 24 * T + 4 * V, 12 * len(kv) + 24 * len(kt)
    frac = lambda b, ms: b / (ms * 1e-3) / D2D_COPY_RATE
    beside = f"marching_cubes {mc_ms:.3f} ms" + (f", sigma query {sigma_ms:.1f} ms" if sigma_ms is not None else "")
    print(f"  components, {what} {N}^3: V {V} T {T}, {len(ids)} components, largest {int(tri_counts.max()) if len(ids) else 0} "
          f"triangles  ({beside})")
    print(f"    labelling {ms_label:9.3f} ms  ({b_label / 1e9:.3f} GB algorithmic = {frac(b_label, ms_label):.3f} of the copy rate)")
    print(f"    table     {ms_table:9.3f} ms  (with its read of the component count)")
    print(f"    filter    {ms_filter:9.3f} ms  (keep_largest=1 -> V {len(kv)} T {len(kt)}; {b_out / 1e9:.3f} GB of compacted output = "
          f"{frac(b_out, ms_filter):.3f} of the copy rate; with its read of the kept counts)")
    print(f"    filter_components end to end {ms_all:9.3f} ms", flush=True)
    del labels, kv, kt
    if HOST:
        host_path(verts, tris)


if "--sparse" in sys.argv:
    # extract_mesh end to end without and behind a grid: tools/time_occupancy.py's capsule scaled to the mesh lattice's box
    # [-1.5, 1.5]^3 (about 10 % of it), as a 128^3 grid dilated by 1.  The random NeRF crosses the threshold wherever it is
    # evaluated, so the sparse mesh is the part of the dense one inside the active bricks: V and T are printed per row.
    ax = [torch.linspace(-1, 1, 128, device=dev, dtype=torch.float64) for _ in range(3)]
    X, Y, Z = torch.meshgrid(*ax, indexing="ij")
    dist = torch.sqrt(X ** 2 + (Y.abs() - 0.6).clamp_min(0) ** 2 + Z ** 2)
    grid = M.OccupancyGrid.from_sigma(torch.where(dist <= 0.38, 5.0, -5.0).float(), (-1.5,) * 3, (1.5,) * 3, 1.0, "softplus", 1)
    del X, Y, Z, dist
    print(f"extract_mesh end to end, dense and behind the capsule grid ({grid.occupied_fraction():.3f} of its 127^3 cells occupied)")
    for N in Ns:
        for prec in ("f32", "bf16"):
            kw = dict(N_grid=N, sigma_threshold=10, precision=prec)
            ms, out = timeit(lambda: M.extract_mesh(nerf, emb, **kw), warm=1, n=3)
            row(f"extract_mesh {prec}", N, ms, out)
            ms_s, out = timeit(lambda: M.extract_mesh(nerf, emb, occupancy=grid, **kw), warm=1, n=3)
            row(f"extract_mesh {prec}, occupancy=grid", N, ms_s, out)
            a = np.linspace(-1.5, 1.5, N).astype(np.float32)
            _, (K, bricks) = M.query_sigma_lattice((a, a, a), nerf, emb, grid, world_of_axis=(1, 0, 2), fill=0.0, precision=prec,
                                                   return_stats=True)
            print(f"    {ms_s / ms:.3f} x; active bricks {K} of {bricks} = {K / bricks:.3f}", flush=True)
            del out
            torch.cuda.empty_cache()
    sys.exit(0)
print("marching_cubes (clamp_zero, threshold 10) on the f32 sigma lattice; the components leg on each mesh")
for N in Ns:
    with torch.no_grad():
        xyz = M.mesh.lattice(N, dev)
        sigma_ms, sig = timeit(lambda: M.query_sigma(xyz, nerf, emb), warm=1, n=3)
        vol = sig.view(N, N, N)
        del xyz, sig
    ms, out = timeit(lambda: M.marching_cubes(vol, 10.0, clamp_zero=True))
    row("marching_cubes", N, ms, out)
    del vol
    components_leg("test NeRF sigma at 10", N, out[0], out[1], ms, sigma_ms)
    del out
    # a smooth field with a far smaller surface than the random NeRF's: what reading the volume itself costs
    ax = torch.linspace(0, 1, N, device=dev)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    vol = (torch.sin(6.0 * x + 2.0 * y * y) + torch.sin(5.0 * y + 3.0 * z) + torch.sin(7.0 * z + 4.0 * x * y)).contiguous()
    del x, y, z
    ms, out = timeit(lambda: M.marching_cubes(vol, 0.3))
    row("marching_cubes, smooth field", N, ms, out)
    del vol
    components_leg("smooth field", N, out[0], out[1], ms)
    del out
    torch.cuda.empty_cache()
if COMPONENTS_ONLY:
    sys.exit(0)
print("extract_mesh end to end (lattice + query_sigma + marching_cubes + post-processing)")
for N in Ns:
    for prec in ("f32", "bf16", "bf16x3"):
        ms, out = timeit(lambda: M.extract_mesh(nerf, emb, N_grid=N, sigma_threshold=10, precision=prec), warm=1, n=3)
        row(f"extract_mesh {prec}", N, ms, out)
        del out
        torch.cuda.empty_cache()
