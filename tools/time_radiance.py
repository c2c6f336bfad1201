#!/usr/bin/env python3
"""Point radiance query on a lattice (an RGBA volume of the canonical body; the colours of a mesh's vertices are the same
query on fewer points): moco_flow_amd.query_radiance (mf_points_radiance, one launch), query_sigma (fp32) on the same
points, and what the query replaces -- the module calls [NoF ->] Embedding -> zero-pad -> Embedding of the extra block ->
NeRF.forward of this package on the same GPU, with their padded (B, 66) / (B, 68) rows in HBM.  Two modes, as
tools/time_lattice.py: canonical space, and through the backward NoF.  NeRF "ind"/5, dense synthetic weights.

Per row: device time per call from HIP events around each call, 5 warm-up calls, median of 20; points/s; for
query_radiance the fraction of the 157.3 TFLOP/s fp32 matrix peak at SURVEY.md §8d's algorithmic FLOPs per point (NeRF
full (ind/5) 1 181 184, + NoF quat 134 400 through the flow; query_sigma: NeRF sigma_only 982 528).
Usage: time_radiance.py [N_grid]  (default 256)"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import moco_flow_amd as M
from moco_flow_amd import synth

PEAK = 157.3e12
F_FULL, F_SIGMA, F_NOF = 1181184, 982528, 134400
N = int(sys.argv[1]) if len(sys.argv) > 1 else 256
IND = 0.25
dev = torch.device("cuda")
load = lambda m, sd: (m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}), m.to(dev))[1]
nerf = load(M.NeRF(8, 256, 63, [4], "ind", 5), synth.nerf_state(0, extra_feat_type="ind", extra_feat_dim=5, regime="dense"))
nof = load(M.NoF(4, 128, 33, [2], "ind", 33, True), synth.nof_state(0, use_quat=True, tag="bw", head_scale=0.25))
ax = torch.linspace(-1.2, 1.2, N, device=dev)
xyz = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3).contiguous()
B = xyz.shape[0]
embs = [M.Embedding(3, 10), M.Embedding(1, 2), None]
nof_embs = [M.Embedding(3, 5), M.Embedding(1, 16)]
ind_col = torch.full((B, 1), IND, device=dev)


def module_calls(through_nof):
    pts = xyz
    if through_nof:
        inp = torch.cat([nof_embs[0](xyz), nof_embs[1](ind_col)], -1)          # (B, 33 + 33)
        pts = nof(inp, xyz)
    e = embs[1](ind_col)                                                       # (B, 5): as wide as the block, no pad needed
    pad = torch.zeros((B, nerf.extra_feat_dim), device=dev)
    pad[:, :e.shape[1]] = e
    return nerf(torch.cat([embs[0](pts), pad], -1))                            # (B, 63 + 5) -> (B, 4)


def timeit(f, warm=5, n=20):
    for _ in range(warm):
        f()
    torch.cuda.synchronize()
    ms = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


print(f"{N}^3 = {B / 1e6:.1f} M lattice points, fp32, HIP events, median of 20 after 5 warm-ups")
with torch.no_grad():
    for through_nof in (False, True):
        kw = dict(bw_nof=nof, nof_embeddings=nof_embs) if through_nof else {}
        extra = F_NOF if through_nof else 0
        t_rad = timeit(lambda: M.query_radiance(xyz, nerf, embs, ind=IND, **kw))
        t_sig = timeit(lambda: M.query_sigma(xyz, nerf, embs[0], ind=IND, precision="f32", **kw))
        t_mod = timeit(lambda: module_calls(through_nof))
        print(f"  {'observation space (bw NoF ->)' if through_nof else 'canonical space'}:")
        print(f"    query_radiance : {t_rad:8.2f} ms  {B / (t_rad * 1e-3):.3e} points/s  {B * (F_FULL + extra) / (t_rad * 1e-3) / PEAK:.3f} of the fp32 matrix peak")
        print(f"    query_sigma    : {t_sig:8.2f} ms  {B / (t_sig * 1e-3):.3e} points/s  {B * (F_SIGMA + extra) / (t_sig * 1e-3) / PEAK:.3f} of the fp32 matrix peak")
        print(f"    module calls   : {t_mod:8.2f} ms  {B / (t_mod * 1e-3):.3e} points/s")
        print(f"    query_radiance / query_sigma = {t_rad / t_sig:.3f} (FLOP ratio {(F_FULL + extra) / (F_SIGMA + extra):.3f}); module calls / query_radiance = {t_mod / t_rad:.2f}")
