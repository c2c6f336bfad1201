"""CPU oracle of the fused point queries (query_sigma: xyz -> [bw NoF(ind)] -> encode -> NeRF trunk -> raw sigma) in any
arithmetic of oracle/bf16_ref.py, and the inputs tests/test_gpu_point_queries.py launches.  No GPU, no package code beyond
the synthetic weight draws: tests/test_points_oracle_cpu.py holds what is here to the preconditions the GPU bars need.

``point_query(B.F32, ..)`` is the trainer's spelling (trainer_moco_flow.py:146-187) that tests/test_gpu_parity.py::
test_fused_point_query restates with oracle/cpu_ref.py; with ``B.BF16`` / ``B.BF16X3`` every operand is rounded where
points_kernel_bf16 rounds it (the networks, embeddings and the per-point index bias are the render pass's own)."""
import numpy as np
import torch

from moco_flow_amd import synth
from oracle import bf16_ref as B
from oracle import cpu_ref as R

TILE = {"f32": 128, "bf16": 256, "bf16x3": 128}      # points per workgroup trip (kTile; 8 / 4 waves x 32 in the bf16 kernels)
MI355X_CUS = 256                                      # what the CPU preconditions assume for the device's launch shape
# five distinct image indices in [-1, 1); the first is the scalar of the existing point-query tests (frame 17 of 300)
IND_VALUES = tuple(float(np.float32(v)) for v in (17 * 2 / 300 - 1.0, -0.45, 0.05, 0.4, 0.85))


def states():
    """(NeRF(ind) state, NoF state): the draws of the existing point-query tests."""
    return (synth.nerf_state(41, extra_feat_type="ind", extra_feat_dim=5, regime="dense", tag="pts"),
            synth.nof_state(42, use_quat=True, tag="pts", head_scale=0.25))


def second_trip(tile, cus=MI355X_CUS):
    """Smallest point count at which a workgroup of the persistent launch (at most one per CU) takes a second trip and the
    last tile is ragged: one tile more than the grid has workgroups, and one point into the tile after it."""
    return (cus + 1) * tile + 1


def inputs(n, seed=0):
    """(xyz (n, 3) in [-1.5, 1.5), ind (n,)): ind = IND_VALUES[i % 5], so neighbouring lanes differ and every tile holds all
    five values."""
    xyz = torch.rand(n, 3, generator=torch.Generator().manual_seed(1000 + seed)) * 3 - 1.5
    ind = torch.tensor(IND_VALUES, dtype=torch.float32)[torch.arange(n) % len(IND_VALUES)]
    return xyz, ind


def subset(n, tile, seed=0):
    """Sorted indices of the points an oracle evaluates of a launch over n: every point of the first tile, every point of the
    last two tiles (at second_trip: the second trip of workgroups 0 and 1, the last one ragged) and 256 seeded draws from the
    points between them.  Points are independent of their batch, so an oracle of xyz[idx] checks a launch over all n."""
    ntiles = (n + tile - 1) // tile
    lo, hi = tile, (ntiles - 2) * tile
    if hi - lo <= 256:
        return torch.arange(n)
    mid = torch.randperm(hi - lo, generator=torch.Generator().manual_seed(seed))[:256] + lo
    return torch.cat([torch.arange(lo), mid.sort().values, torch.arange(hi, n)])


def point_query(arith, sd_nerf, sd_nof, xyz, ind):
    """(canonical point (n, 3), raw sigma through the NoF (n, 1), raw sigma of xyz taken as canonical (n, 1)) in ``arith``.
    xyz (n, 3), ind (n,) per-point image indices; sd_nof / ind None: no NoF, the first two are None."""
    be = B.Backend(arith)
    nerf = be.NeRF(8, 256, 63, [4], "ind", 5)
    nerf.load_state_dict(sd_nerf)
    ex = be.Embedding(3, 10)
    with torch.no_grad():
        canon = s_nof = None
        if sd_nof is not None and ind is not None:
            nof = be.NoF(4, 128, 33, [2], "ind", 33, True)
            nof.load_state_dict(sd_nof)
            inp = torch.cat([R._embed_padded(be.Embedding(3, 5), xyz, 33),
                             R._embed_padded(be.Embedding(1, 16), ind.reshape(-1, 1), 33)], -1)
            canon = nof(inp, xyz)
            s_nof = nerf(R._embed_padded(ex, canon, 63), sigma_only=True)
        s_can = nerf(R._embed_padded(ex, xyz, 63), sigma_only=True)
    return canon, s_nof, s_can
