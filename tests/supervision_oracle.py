"""Torch-CPU restatement of the reference's SMPL point supervision, for tests/test_supervision_cpu.py and
tests/test_gpu_supervision.py: the query sampling, nearest-vertex search, transform and split of ``get_frame_correspondence``
(datasets/moco_flow_dataset.py:101-132), ``forwarf_nerf``'s alphas (trainer/trainer_moco_flow.py:146-157) and the three point
losses of ``_shared_step`` (:330-363; trainer/trainer_nof.py:115-125 with all_points).  fp32 like the reference; the losses are
taken on the COMPACTED sets, as the reference takes them."""
import torch
from torch import nn

from oracle import smpl_ref


def sample_queries(verts, u, pick, noise, thickness, extent=3.0):
    """:103-112 for given draws: u (n, 3) uniform -> the cube of side `extent` about the origin (what trimesh's Box.sample_volume
    returns for a uniform draw); near-surface points verts[pick] + noise * thickness; cube points first."""
    box = (u - 0.5) * extent
    near = verts[pick]
    near = near + noise * thickness
    return torch.cat([box, near], dim=0)


def nearest(verts, query):
    """:120-121, knn_cuda.KNN(k = 1): (dist (Q,), ind (Q,)) of the nearest vertex, the lowest index among equal minima.  The
    squared distance is fma(az, az, fma(ay, ay, ax ax)) on fp32 differences ref - query, evaluated here in float64 and rounded
    to fp32 after each step."""
    a = (verts[None, :, :] - query[:, None, :]).double()                       # fp32 differences
    d = (a[..., 0] * a[..., 0]).float().double()
    d = (a[..., 1] * a[..., 1] + d).float().double()
    d = (a[..., 2] * a[..., 2] + d).float()
    best = d.min(dim=1).values
    ind = (d == best[:, None]).to(torch.int64).argmax(dim=1)                    # argmax returns the FIRST maximal entry
    return torch.sqrt(best), ind


def correspondence(verts, trans, query, thickness):
    """:120-132 without the compaction: (pairs (Q, 6), inside (Q,) bool, dist, ind)."""
    dist, ind = nearest(verts, query)
    cano = smpl_ref.apply_vertex_transforms(trans, ind, query)
    return torch.cat([query, cano], dim=-1), dist < thickness, dist, ind


def split(pairs, inside):
    """:131-132."""
    return pairs[inside], pairs[~inside]


def alphas(sigma, delta):
    """trainer_moco_flow.py:154."""
    return 1 - torch.exp(-delta * nn.Softplus()(sigma))


def bce_rows(sigma, delta):
    """nn.BCELoss(reduction='none') of alphas against zeros, :362."""
    a = alphas(sigma, delta)
    return nn.BCELoss(reduction="none")(a, torch.zeros_like(a))


def point_losses(pairs, inside, pred_bw=None, pred_fw=None, sigmas=(), deltas=(), all_points=False):
    """:330-363 on given network outputs (all full length, compacted here): {term: (mean, count)}; an empty set gives
    (0, 0) where the reference's mean is NaN."""
    inside = inside.bool()
    rows = torch.ones_like(inside) if all_points else inside
    query, cano = pairs[:, :3], pairs[:, 3:]
    out = {}
    for key, pred, target in (("nof_bw", pred_bw, cano), ("nof_fw", pred_fw, query)):
        if pred is None:
            continue
        n = int(rows.sum()) * 3
        out[key] = (nn.L1Loss()(pred[rows], target[rows]) if n else pred.sum() * 0, n)
    if len(sigmas):
        outside = torch.cat([alphas(s.reshape(-1)[~inside], d) for s, d in zip(sigmas, deltas)], dim=0)      # :356-361
        n = outside.numel()
        out["alphas_mask"] = (nn.BCELoss()(outside, torch.zeros_like(outside)) if n else outside.sum() * 0, n)
    return out
