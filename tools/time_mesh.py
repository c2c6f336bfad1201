#!/usr/bin/env python3
"""Mesh extraction (visualize_mesh, trainer_moco_flow.py:485-548): marching_cubes alone at 256^3 and 512^3 on the raw
sigma lattice of synth.nerf_state(0, regime="dense") at threshold 10 (sigma head x 3: unscaled, that NeRF's sigma stays
below 10 and the mesh is empty -- tests/golden/gen_mesh_golden.py), and extract_mesh end to end per precision.

Per row: wall time per call (host clock around calls that end in a device synchronise, 2 warm-up calls, median of 5),
V and T, the mesh bytes written (12 V + 24 T), and the volume bytes read (4 B x N^3, the two passes counted once: what
any isosurface step must read) over that time, as a fraction of the 6.29 TB/s measured HBM copy rate
(MI355X_MICROARCH.md).  marching_cubes includes its one device -> host read of the counts and the scratch / output
allocations.  A smooth analytic field at each size shows the cost of the volume read when the mesh is small (the random
NeRF's sigma makes ~10^8 triangles at 512^3).  Usage: time_mesh.py [N ...]  (default 256 512)"""
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
Ns = [int(a) for a in sys.argv[1:]] or [256, 512]
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


print("marching_cubes (clamp_zero, threshold 10) on the f32 sigma lattice")
for N in Ns:
    with torch.no_grad():
        vol = M.query_sigma(M.mesh.lattice(N, dev), nerf, emb).view(N, N, N)
    ms, out = timeit(lambda: M.marching_cubes(vol, 10.0, clamp_zero=True))
    row("marching_cubes", N, ms, out)
    del vol, out
    # a smooth field with a far smaller surface than the random NeRF's: what reading the volume itself costs
    ax = torch.linspace(0, 1, N, device=dev)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    vol = (torch.sin(6.0 * x + 2.0 * y * y) + torch.sin(5.0 * y + 3.0 * z) + torch.sin(7.0 * z + 4.0 * x * y)).contiguous()
    del x, y, z
    ms, out = timeit(lambda: M.marching_cubes(vol, 0.3))
    row("marching_cubes, smooth field", N, ms, out)
    del vol, out
    torch.cuda.empty_cache()
print("extract_mesh end to end (lattice + query_sigma + marching_cubes + post-processing)")
for N in Ns:
    for prec in ("f32", "bf16", "bf16x3"):
        ms, out = timeit(lambda: M.extract_mesh(nerf, emb, N_grid=N, sigma_threshold=10, precision=prec), warm=1, n=3)
        row(f"extract_mesh {prec}", N, ms, out)
        del out
        torch.cuda.empty_cache()
