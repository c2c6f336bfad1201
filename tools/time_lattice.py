#!/usr/bin/env python3
"""Mesh-extraction lattice query (visualize_mesh, trainer_moco_flow.py:485-548 / trainer_nerf.py:215-245: N_grid^3
points through [bw NoF ->] embed -> NeRF(sigma_only) in 10 000-point chunks in the reference) as ONE fused launch
per lattice (mf_points_sigma).  Usage: time_lattice.py [N_grid]

time_lattice.py --sparse [N ...] (default 256 512): the dense query_sigma against query_sigma_lattice on the N^3 lattice over
[-1, 1]^3 behind tools/time_occupancy.py's capsule as a 128^3 grid (dilate 1), canonical space, fp32 and bf16, margin 1; then
OccupancyGrid.from_field at 128^3 dense and within a 32^3 grid of the same capsule.  Device time per call from HIP events
around each call (the sparse call's one count read-back lies inside its pair), 5 warm-up calls, median of 20, one process.
Beside the times: the active brick fraction -- the saving is that fraction and belongs to the scene -- and what the sparse
call costs beyond (active fraction x the dense time): the algorithmic bytes of the three small kernels at the 4.69 TB/s
device-to-device copy rate (select: 8 B per brick; points: 12 B per active point written; scatter: 4 B per active point read
and 4 B per lattice point written), and what is left for the read-back, the launches and the allocations."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import moco_flow_amd as M
from moco_flow_amd import synth
SPARSE = "--sparse" in sys.argv
_args = [a for a in sys.argv[1:] if not a.startswith("--")]
N = int(_args[0]) if _args else 256
dev = torch.device("cuda")


def sparse_report(Ns):
    import statistics
    import numpy as np
    D2D_COPY_RATE = 4.69e12
    load = lambda m, sd: (m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}), m.to(dev))[1]
    nerf = load(M.NeRF(8, 256, 63, [4], "ind", 5), synth.nerf_state(0, extra_feat_type="ind", extra_feat_dim=5, regime="dense"))
    emb = M.Embedding(3, 10)
    aabb = np.array([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]])

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

    def capsule_grid(G):
        """time_occupancy.py's capsule (a standing segment of length 1.2, radius 0.38) on a G^3 lattice, dilated by 1."""
        ax = [torch.linspace(-1, 1, G, device=dev, dtype=torch.float64) for _ in range(3)]
        X, Y, Z = torch.meshgrid(*ax, indexing="ij")
        dist = torch.sqrt(X ** 2 + (Y.abs() - 0.6).clamp_min(0) ** 2 + Z ** 2)
        return M.OccupancyGrid.from_sigma(torch.where(dist <= 0.38, 5.0, -5.0).float(), aabb[0], aabb[1], 1.0, "softplus", 1)

    grid = capsule_grid(128)
    print(f"sparse lattice queries behind the capsule grid (128^3 lattice, {grid.occupied_fraction():.3f} of the cells occupied), "
          "canonical space, margin 1")
    with torch.no_grad():
        for n in Ns:
            ax = np.linspace(-1.0, 1.0, n).astype(np.float32)
            xyz = M.OccupancyGrid.lattice(n, aabb, dev)[0]
            for prec in ("f32", "bf16"):
                dense = timeit(lambda: M.query_sigma(xyz, nerf, emb, precision=prec))
                sparse = timeit(lambda: M.query_sigma_lattice((ax, ax, ax), nerf, emb, grid, precision=prec))
                _, (K, bricks) = M.query_sigma_lattice((ax, ax, ax), nerf, emb, grid, precision=prec, return_stats=True)
                frac = K / bricks
                extra = sparse - frac * dense
                small = (8 * bricks + (12 + 4) * 512 * K + 4 * n ** 3) / D2D_COPY_RATE * 1e3
                print(f"  {n:4d}^3 {prec:5s}: dense {dense:9.3f} ms, sparse {sparse:9.3f} ms ({sparse / dense:.3f} x); active bricks {K} of "
                      f"{bricks} = {frac:.3f}; sparse - fraction x dense = {extra:8.3f} ms, of which {small:.3f} ms are the small "
                      f"kernels' bytes at the copy rate and {extra - small:8.3f} ms the read-back, launches and allocations", flush=True)
            del xyz
            torch.cuda.empty_cache()
        coarse = capsule_grid(32)
        for prec in ("f32", "bf16"):
            kw = dict(N_grid=128, sigma_threshold=1.0, activate_type="softplus", dilate=1, precision=prec)
            dense = timeit(lambda: M.OccupancyGrid.from_field(nerf, emb, aabb, **kw))
            within = timeit(lambda: M.OccupancyGrid.from_field(nerf, emb, aabb, within=coarse, **kw))
            ax = np.linspace(-1.0, 1.0, 128).astype(np.float32)
            _, (K, bricks) = M.query_sigma_lattice((ax, ax, ax), nerf, emb, coarse, precision=prec, return_stats=True)
            print(f"  from_field 128^3 {prec:5s}: dense {dense:8.3f} ms, within the 32^3 capsule grid {within:8.3f} ms "
                  f"({within / dense:.3f} x); active bricks {K} of {bricks} = {K / bricks:.3f}", flush=True)


if SPARSE:
    sparse_report([int(a) for a in _args] or [256, 512])
    sys.exit(0)
load = lambda m, sd: (m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}), m.to(dev))[1]
nerf = load(M.NeRF(8, 256, 63, [4], "ind", 5), synth.nerf_state(0, extra_feat_type="ind", extra_feat_dim=5, regime="dense"))
nof = load(M.NoF(4, 128, 33, [2], "ind", 33, True), synth.nof_state(0, use_quat=True, tag="bw", head_scale=0.25))
ax = torch.linspace(-1.2, 1.2, N, device=dev)
xyz = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3).contiguous()
emb = M.Embedding(3, 10)
nof_embs = [M.Embedding(3, 5), M.Embedding(1, 16)]


def timeit(f, n=3):
    f(); torch.cuda.synchronize(); t = time.perf_counter()
    for _ in range(n):
        f()
    torch.cuda.synchronize(); return (time.perf_counter() - t) / n * 1e3


print(f"{N}^3 = {xyz.shape[0] / 1e6:.1f} M lattice points")
for prec in ("f32", "bf16", "bf16x3"):
    ms = timeit(lambda: M.query_sigma(xyz, nerf, emb, precision=prec))
    print(f"  {prec:4s} canonical space (NeRF sigma)        : {ms:8.1f} ms  {xyz.shape[0] / (ms * 1e-3):.3e} points/s")
    ms = timeit(lambda: M.query_sigma(xyz, nerf, emb, nof, nof_embs, 0.25, precision=prec))
    print(f"  {prec:4s} observation space (bw NoF -> sigma) : {ms:8.1f} ms  {xyz.shape[0] / (ms * 1e-3):.3e} points/s")
