#!/usr/bin/env python3
"""The SMPL point supervision of a training step (get_frame_correspondence, datasets/moco_flow_dataset.py:87-142, and the point
losses of _shared_step, trainer/trainer_moco_flow.py:330-363): moco_flow_amd.supervision -- correspondence + point_losses +
backward(), full-length tensors and a mask, no host read -- beside today's path on the same GPU: device draws,
smpl.frame_correspondence (three LBS calls, mf_knn1, the transform, two boolean-index compactions), the module calls on the
compacted sets, nn.L1Loss / nn.BCELoss, backward().  Both sides get the same draws.  Also: the mf_point_correspond launch alone
beside mf_knn1 + mf_apply_vertex_transforms.

At 2 x 1000 points (c2f.yaml's N_sampled) and 2 x 100 000 on the 6890-vertex synthetic model, c2f's networks (two NoFs
4 x 128, one NeRF 8 x 256).  Per row: device time per call from HIP events around each call, 5 warm-up calls, median of 20.  Both
sides are launch-bound at the small size; no fraction of any peak is meant.  Usage: time_supervision.py"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from torch import nn

import moco_flow_amd as M
from moco_flow_amd import smpl as S, supervision, synth
from moco_flow_amd.knn import KNN

dev = torch.device("cuda")
load = lambda m, sd: (m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}), m.to(dev))[1]
bw = load(M.NoF(4, 128, 33, [2], "ind", 33, True), synth.nof_state(3, use_quat=True, tag="bw", head_scale=0.25))
fw = load(M.NoF(4, 128, 33, [2], "ind", 33, True), synth.nof_state(4, use_quat=True, tag="fw", head_scale=0.25))
nerf = load(M.NeRF(8, 256, 63, [4], "ind", 5), synth.nerf_state(3, extra_feat_type="ind", extra_feat_dim=5, regime="dense"))
exyz, eind, nxyz = M.Embedding(3, 5), M.Embedding(1, 16), M.Embedding(3, 10)
model = S.SMPL(model=synth.smpl_model(1, 6890)).to(dev)
pose, betas = (torch.from_numpy(a).to(dev) for a in synth.smpl_pose(5, batch=2, scale=0.6))
IND, DELTA, THICKNESS = 0.1, 1 / 128, 0.2
knn = KNN(k=1, transpose_mode=True)


def zero():
    for m in (bw, fw, nerf):
        m.zero_grad(set_to_none=True)


def fused_step(draws):
    zero()
    n = draws[0].shape[0]
    corr = supervision.correspondence(model, pose[:1], betas[:1], pose[1:], betas[1:], n, THICKNESS, draws=draws)
    t = supervision.point_losses(corr, IND, bw, fw, (exyz, eind), nerfs=(nerf,), nerf_embedding_xyz=nxyz, deltas=(DELTA,))
    (t["nof_bw"] + t["nof_fw"] + t["alphas_mask"]).backward()
    return t


def nof(m, xyz):
    ind = torch.full((xyz.shape[0], 1), IND, device=dev)
    return m(torch.cat([exyz(xyz), eind(ind)], -1), xyz)


def parent_step(draws):
    zero()
    u, pick, noise = draws
    verts = model(pose[:1], betas[:1])[0]
    near = verts[pick]
    near += noise * THICKNESS
    query = torch.cat([(u - 0.5) * 3.0, near], 0)
    ins, outs = S.frame_correspondence(model, pose[:1], betas[:1], pose[1:], betas[1:], query, THICKNESS, knn=knn)   # synchronises twice
    q, cn = ins[:, :3].contiguous(), ins[:, 3:].contiguous()
    t = {"nof_bw": nn.L1Loss()(nof(bw, q), cn), "nof_fw": nn.L1Loss()(nof(fw, cn), q)}
    emb = nxyz(nof(bw, outs[:, :3].contiguous()))
    sig = nerf(F.pad(emb, (0, nerf.in_channels_xyz - emb.shape[1])), sigma_only=True)
    alphas = 1 - torch.exp(-DELTA * nn.Softplus()(sig))
    t["alphas_mask"] = nn.BCELoss()(alphas, torch.zeros_like(alphas))
    (t["nof_bw"] + t["nof_fw"] + t["alphas_mask"]).backward()
    return t


def timeit(f, warm=5, n=20):
    for _ in range(warm):
        out = f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = f()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts), max(ts), out


print("6890 vertices, NoF 4 x 128 (both directions), NeRF 8 x 256; ms per call (median of 20 / min / max)")
for n in (1000, 100000):
    g = torch.Generator(device=dev).manual_seed(n)
    draws = (torch.rand((n, 3), device=dev, generator=g), torch.randint(6890, (n,), device=dev, generator=g),
             torch.randn((n, 3), device=dev, generator=g))
    a, b = fused_step(draws), parent_step(draws)
    for k in a:
        assert abs(float(a[k]) - float(b[k])) <= 1e-5 * abs(float(b[k])), (k, float(a[k]), float(b[k]))
    verts = model(pose[:1], betas[:1])[0]
    T = model.get_vertex_transformation(pose, betas)
    trans = S.frame_transforms(T[0], T[1])
    query = supervision.correspondence(model, pose[:1], betas[:1], pose[1:], betas[1:], n, THICKNESS, draws=draws).pairs[:, :3].contiguous()

    def two_kernels():
        d, i = knn(verts[None], query[None])
        return S.apply_vertex_transforms(trans, i[0], query)

    for name, f in ((f"correspondence + point_losses + backward  2 x {n}", lambda: fused_step(draws)),
                    (f"frame_correspondence + modules + backward 2 x {n}", lambda: parent_step(draws)),
                    (f"  mf_point_correspond alone                Q = {2 * n}", lambda: supervision.point_correspond(verts, trans, query, THICKNESS)),
                    (f"  mf_knn1 + mf_apply_vertex_transforms     Q = {2 * n}", two_kernels)):
        med, lo, hi, _ = timeit(f)
        print(f"  {name:58s} {med:9.4f} / {lo:9.4f} / {hi:9.4f}", flush=True)
