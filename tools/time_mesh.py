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
an occupancy grid (query_sigma_lattice; the timings beside tools/time_lattice.py --sparse).

--simplify CELL: only the simplification leg (simplify_mesh, vertex clustering with a cell of CELL lattice steps) on both
meshes of each size (default 512): its two steps by HIP events on the stream, median of 20 after 5 warm-ups -- the plan (cell
ids, the duplicate table, survivors, the ranks of the used cells; scratch allocation included) and the emit (members' sums and
minima, the mean positions, the re-indexed triangles; output allocation included) -- and simplify_mesh end to end with its
read of the counts, both placements.  Beside each time the algorithmic bytes (plan: 12 B per vertex + 24 B per triangle read;
emit: the same read, 20 B per new vertex + 24 B per kept triangle + 8 B per vertex of cluster written) over the 4.69 TB/s
device-to-device copy rate -- information only: the table probes and the per-cell atomics are random accesses and no share
of a peak is claimed.  The numpy oracle (tests/mesh_simplify_oracle.py) on the same mesh in the same process, once, where
the mesh has at most 8 M triangles (--no-host skips it); it also checks the device's result bit for bit.

--smooth K: only the smoothing leg (vertex_rings, smooth_mesh) on both meshes of each size (default 512), device times by HIP
events on the stream, median of 20 after 5 warm-ups: vertex_rings (with its read of [bad, over_cap, R] and its allocations); one
smoothing step (the difference between 21 and 1 Laplacian steps over given rings, divided by 20: the packing and unpacking
cancel); smooth_mesh(iterations=K) end to end, building its rings, with its read.  Beside each time the algorithmic bytes
(rings: 24 B per triangle read + 8 B per ring entry and per offset + 1 B per vertex written; a step: 24 V + 4 R + 4 (V + 1), every
position read once and written once and the 32-bit private indices read once) over the 4.69 TB/s device-to-device copy rate
-- information only: the neighbour gathers are cache traffic and no share of a peak is claimed.  The host path it replaces in
the same process, once: the device -> host copy and the numpy oracle (tests/mesh_smooth_oracle.py), where the mesh has at most
8 M triangles (--no-host skips it); it also checks the device's result bit for bit.
Usage: time_mesh.py [--no-host] [--components-only] [--sparse] [--simplify CELL] [--smooth K] [N ...]  (default 256 512)"""
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
SIMPLIFY = float(sys.argv[sys.argv.index("--simplify") + 1]) if "--simplify" in sys.argv else None
SMOOTH = int(sys.argv[sys.argv.index("--smooth") + 1]) if "--smooth" in sys.argv else None
_args = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith("--") and sys.argv[i - 1] not in ("--simplify", "--smooth")]
Ns = [int(a) for a in _args] or ([512] if SIMPLIFY is not None or SMOOTH is not None else [256, 512])
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


def time_events(f, warm=5, n=20):
    """Median of n device times of f() in ms, by HIP events on the current stream, after `warm` calls."""
    for _ in range(warm):
        out = f()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = f()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), out


def simplify_leg(what, N, verts, tris, cell):
    import ctypes
    V, T = len(verts), len(tris)
    d3 = ctypes.c_double * 3
    grid = (d3(0, 0, 0), d3(N - 1, N - 1, N - 1), float(cell), *M.mesh._simplify_grid(np.zeros(3), np.full(3, N - 1.0), cell))
    slots = 1 << (2 * T).bit_length()
    ms_plan, (scratch, counts) = time_events(lambda: M.mesh._simplify_plan(verts, tris, grid, slots))
    Vk, Tk, bad = counts.tolist()
    ms_emit, _ = time_events(lambda: M.mesh._simplify_emit(verts, tris, grid, scratch, Vk, Tk, True))
    kw = dict(lo=(0,) * 3, hi=(N - 1,) * 3)
    ms_mean, out = time_events(lambda: M.simplify_mesh(verts, tris, cell, placement="mean", return_map=True, **kw))
    ms_first, _ = time_events(lambda: M.simplify_mesh(verts, tris, cell, placement="first", **kw))
    b_plan, b_emit = 12 * V + 24 * T, 12 * V + 24 * T + 20 * Vk + 24 * Tk + 8 * V
    frac = lambda b, ms: b / (ms * 1e-3) / D2D_COPY_RATE
    print(f"  simplify, {what} {N}^3, cell {cell}: V {V} -> {Vk}, T {T} -> {Tk} ({bad} bad), table of {slots} slots")
    print(f"    plan  {ms_plan:9.3f} ms  ({b_plan / 1e9:.3f} GB algorithmic = {frac(b_plan, ms_plan):.3f} of the copy rate)")
    print(f"    emit  {ms_emit:9.3f} ms  ({b_emit / 1e9:.3f} GB algorithmic = {frac(b_emit, ms_emit):.3f} of the copy rate)")
    print(f"    simplify_mesh end to end, with its read of the counts: mean {ms_mean:9.3f} ms, first {ms_first:9.3f} ms", flush=True)
    if not HOST:
        return
    if T > 8_000_000:
        print(f"    numpy oracle: not measured ({T} triangles: np.unique on the cell triples needs tens of GB and minutes)", flush=True)
        return
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import mesh_simplify_oracle as S
    t0 = time.perf_counter()
    v, t = verts.cpu().numpy(), tris.cpu().numpy()
    t1 = time.perf_counter()
    want = S.simplify(v, t, cell, (0,) * 3, (N - 1,) * 3)
    t2 = time.perf_counter()
    same = all(torch.equal(g.cpu(), torch.from_numpy(w)) for g, w in zip(out, want))
    print(f"    numpy oracle: device -> host copy {1e3 * (t1 - t0):8.1f} ms, simplify {1e3 * (t2 - t1):10.1f} ms; the device's result "
          f"{'equals it bit for bit' if same else 'DIFFERS'}", flush=True)


def smooth_leg(what, N, verts, tris, K):
    V, T = len(verts), len(tris)
    ms_rings, rings = time_events(lambda: M.vertex_rings(tris, V))
    R = len(rings[1])
    ms_1, _ = time_events(lambda: M.smooth_mesh(verts, tris, iterations=1, mu=None, rings=rings))
    ms_21, _ = time_events(lambda: M.smooth_mesh(verts, tris, iterations=21, mu=None, rings=rings))
    ms_step = (ms_21 - ms_1) / 20.0
    ms_all, out = time_events(lambda: M.smooth_mesh(verts, tris, iterations=K))
    b_rings, b_step = 24 * T + 8 * R + 8 * (V + 1) + V, 24 * V + 4 * R + 4 * (V + 1)
    frac = lambda b, ms: b / (ms * 1e-3) / D2D_COPY_RATE
    print(f"  smooth, {what} {N}^3: V {V} T {T}, R {R} ring entries, {int(rings[2].sum())} boundary vertices")
    print(f"    vertex_rings  {ms_rings:9.3f} ms  ({b_rings / 1e9:.3f} GB algorithmic = {frac(b_rings, ms_rings):.3f} of the copy rate; with its read)")
    print(f"    one step      {ms_step:9.3f} ms  ({b_step / 1e9:.3f} GB algorithmic = {frac(b_step, ms_step):.3f} of the copy rate; "
          f"21 steps {ms_21:.3f} ms, 1 step {ms_1:.3f} ms, packing and unpacking included in both)")
    print(f"    smooth_mesh(iterations={K}) end to end, rings built inside, with its read: {ms_all:9.3f} ms", flush=True)
    if not HOST:
        return
    if T > 8_000_000:
        print(f"    host path: not measured ({T} triangles: np.unique on the {6 * T} ring keys needs tens of GB and minutes)", flush=True)
        return
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import mesh_smooth_oracle as O
    t0 = time.perf_counter()
    v, t = verts.cpu().numpy(), tris.cpu().numpy()
    t1 = time.perf_counter()
    want_rings = O.rings(t, V)
    t2 = time.perf_counter()
    want = O.smooth(v, t, K, rings_=want_rings)
    t3 = time.perf_counter()
    same = all(torch.equal(g.cpu(), torch.from_numpy(w)) for g, w in zip(rings, want_rings)) and torch.equal(out.cpu(), torch.from_numpy(want))
    print(f"    host path: device -> host copy {1e3 * (t1 - t0):8.1f} ms, numpy rings {1e3 * (t2 - t1):10.1f} ms, numpy smooth "
          f"({K} iterations) {1e3 * (t3 - t2):10.1f} ms; the device's result {'equals it bit for bit' if same else 'DIFFERS'}", flush=True)


def both_meshes(N):
    """(what, verts, tris) of the two meshes of a size, one at a time."""
    with torch.no_grad():
        xyz = M.mesh.lattice(N, dev)
        vol = M.query_sigma(xyz, nerf, emb).view(N, N, N)
        del xyz
    yield ("test NeRF sigma at 10",) + M.marching_cubes(vol, 10.0, clamp_zero=True)
    del vol
    torch.cuda.empty_cache()
    ax = torch.linspace(0, 1, N, device=dev)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    vol = (torch.sin(6.0 * x + 2.0 * y * y) + torch.sin(5.0 * y + 3.0 * z) + torch.sin(7.0 * z + 4.0 * x * y)).contiguous()
    del x, y, z
    yield ("smooth field",) + M.marching_cubes(vol, 0.3)


if SMOOTH is not None:
    print(f"vertex_rings and smooth_mesh ({SMOOTH} Taubin iterations, lam 0.5, mu -0.53, boundary fixed) on the marching-cubes meshes "
          "of the f32 sigma lattice (threshold 10) and of the smooth field (0.3)")
    for N in Ns:
        for what, verts, tris in both_meshes(N):
            smooth_leg(what, N, verts, tris, SMOOTH)
            del verts, tris
            torch.cuda.empty_cache()
    sys.exit(0)
if SIMPLIFY is not None:
    print(f"simplify_mesh (vertex clustering, cell {SIMPLIFY} lattice steps) on the marching-cubes meshes of the f32 sigma lattice "
          "(threshold 10) and of the smooth field (0.3)")
    for N in Ns:
        with torch.no_grad():
            xyz = M.mesh.lattice(N, dev)
            vol = M.query_sigma(xyz, nerf, emb).view(N, N, N)
            del xyz
        verts, tris = M.marching_cubes(vol, 10.0, clamp_zero=True)
        del vol
        simplify_leg("test NeRF sigma at 10", N, verts, tris, SIMPLIFY)
        del verts, tris
        torch.cuda.empty_cache()
        ax = torch.linspace(0, 1, N, device=dev)
        x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
        vol = (torch.sin(6.0 * x + 2.0 * y * y) + torch.sin(5.0 * y + 3.0 * z) + torch.sin(7.0 * z + 4.0 * x * y)).contiguous()
        del x, y, z
        verts, tris = M.marching_cubes(vol, 0.3)
        del vol
        simplify_leg("smooth field", N, verts, tris, SIMPLIFY)
        del verts, tris
        torch.cuda.empty_cache()
    sys.exit(0)
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
