"""SMPL point supervision of a training step on the device (reference: ``get_frame_correspondence``,
datasets/moco_flow_dataset.py:87-142, called at trainer/trainer_moco_flow.py:419-438 and trainer/trainer_nof.py:127-131; the
point losses of ``_shared_step``, trainer_moco_flow.py:330-363 and trainer_nof.py:115-125).

The reference samples query points, finds each point's nearest SMPL vertex, moves the point with that vertex's transform,
COMPACTS the points into an inside and an outside set (two host reads of data-dependent lengths) and takes three losses of
the two sets.  Here every tensor keeps all Q rows in the queries' order and the split is a byte mask:

    correspondence   the draws (torch, on the device), two mf_smpl_lbs calls, mf_smpl_frame_transforms and ONE
                     mf_point_correspond launch (search, transform and flag; near-surface queries generated in the launch)
    point_losses     the existing HIP module calls on all Q rows, then ONE autograd node around mf_point_loss_partials /
                     mf_point_loss_partials_backward: three (sum, count) pairs reduced on the device

Neither reads anything back to the host; ``Correspondence.split()`` (the reference's two compacted sets) is the only call
that synchronises.  The price of the mask: the forward NoF and the NeRFs also run on the rows the mask then drops."""
import ctypes as C

import torch
import torch.nn.functional as F

from . import _lib as L
from .smpl import frame_transforms

__all__ = ["Correspondence", "correspondence", "point_correspond", "point_losses"]

TERMS = ("nof_bw", "nof_fw", "alphas_mask")


class Correspondence:
    """pairs (Q, 6) fp32 = [query | canonical]; inside (Q,) uint8 = dist < thickness; dist (Q,) fp32 and ind (Q,) int64 of the
    nearest source-pose vertex.  Full length, in the queries' order."""
    __slots__ = ("pairs", "inside", "dist", "ind")

    def __init__(self, pairs, inside, dist, ind):
        self.pairs, self.inside, self.dist, self.ind = pairs, inside, dist, ind

    def split(self):
        """The reference's (inside_xyzs, outside_xyzs), moco_flow_dataset.py:131-132, by compaction: SYNCHRONISES."""
        m = self.inside.bool()
        return self.pairs[m], self.pairs[~m]


def point_correspond(verts, trans, queries, thickness, pick=None, noise=None, lanes_per_query=0):
    """mf_point_correspond: verts (V, 3), trans (V, 4, 4), queries (Q0, 3) or None, and optionally pick (Q1,) int64 with
    noise (Q1, 3) for Q1 further queries verts[pick] + noise * thickness made in the launch -> Correspondence of Q0 + Q1 rows."""
    L.require_gpu(verts, "supervision.point_correspond")
    dev = verts.device
    v = verts.detach().float().contiguous()
    t = trans.detach().float().contiguous()
    if v.dim() != 2 or v.shape[1] != 3 or tuple(t.shape) != (v.shape[0], 4, 4):
        raise RuntimeError(f"supervision.point_correspond: verts (V, 3) and trans (V, 4, 4), got {tuple(v.shape)} and {tuple(t.shape)}")
    q = None
    if queries is not None:
        L.require_gpu(queries, "supervision.point_correspond")
        q = queries.detach().float().contiguous()
        if q.dim() != 2 or q.shape[1] != 3:
            raise RuntimeError(f"supervision.point_correspond: queries must be (Q, 3), got {tuple(q.shape)}")
    if (pick is None) != (noise is None):
        raise RuntimeError("supervision.point_correspond: pick and noise come together")
    if pick is not None:
        L.require_gpu(pick, "supervision.point_correspond")
        L.require_gpu(noise, "supervision.point_correspond")
        if pick.dtype != torch.int64 or pick.dim() != 1 or tuple(noise.shape) != (pick.shape[0], 3):
            raise RuntimeError(f"supervision.point_correspond: pick (Q,) int64 and noise (Q, 3), got {tuple(pick.shape)} {pick.dtype} "
                               f"and {tuple(noise.shape)}")
        pick, noise = pick.contiguous(), noise.detach().float().contiguous()
    q0 = 0 if q is None else q.shape[0]
    q1 = 0 if pick is None else pick.shape[0]
    Q = q0 + q1
    pairs = torch.empty((Q, 6), device=dev, dtype=torch.float32)
    inside = torch.empty((Q,), device=dev, dtype=torch.uint8)
    dist = torch.empty((Q,), device=dev, dtype=torch.float32)
    ind = torch.empty((Q,), device=dev, dtype=torch.int64)
    L.launch(dev, "mf_point_correspond", v.data_ptr(), t.data_ptr(), v.shape[0], L.ptr(q), q0, L.ptr(pick), L.ptr(noise), q1,
             float(thickness), int(lanes_per_query), pairs.data_ptr(), inside.data_ptr(), dist.data_ptr(), ind.data_ptr())
    return Correspondence(pairs, inside, dist, ind)


def correspondence(smpl, src_pose, src_betas, tgt_pose, tgt_betas, num_sampled, thickness=0.2, *, extent=3.0, generator=None,
                   draws=None, queries=None):
    """``get_frame_correspondence`` (moco_flow_dataset.py:87-142) without its compaction -> Correspondence of 2 num_sampled rows:
    num_sampled points of the cube of side `extent` about the origin (:103-107), then num_sampled near-surface points
    src_verts[randint] + randn * thickness (:109-111).  The draws are torch's, on the device, in the reference's order --
    rand(num_sampled, 3), randint(V, (num_sampled,)), randn(num_sampled, 3) -- or given as draws=(u, pick, noise); the cube
    points are (u - 0.5) * extent (trimesh's sample_volume restated).  queries= (Q, 3) skips the sampling and takes the points
    as given.  No host read."""
    L.require_gpu(src_pose, "supervision.correspondence")
    dev = src_pose.device
    verts, T_src = smpl._lbs(src_pose, src_betas, True, True)
    _, T_tgt = smpl._lbs(tgt_pose, tgt_betas, False, True)
    trans = frame_transforms(T_src[0], T_tgt[0])                                             # :96-100
    verts = verts[0]
    if queries is not None:
        return point_correspond(verts, trans, queries, thickness)
    n = int(num_sampled)
    if n < 0:
        raise RuntimeError(f"supervision.correspondence: num_sampled={n}")
    if draws is None:
        u = torch.rand((n, 3), device=dev, generator=generator)
        pick = torch.randint(verts.shape[0], (n,), device=dev, generator=generator)
        noise = torch.randn((n, 3), device=dev, generator=generator)
    else:
        u, pick, noise = draws
        L.require_gpu(u, "supervision.correspondence")
        if tuple(u.shape) != (n, 3) or tuple(pick.shape) != (n,) or tuple(noise.shape) != (n, 3):
            raise RuntimeError(f"supervision.correspondence: draws must be (u ({n}, 3), pick ({n},), noise ({n}, 3)), got "
                               f"{tuple(u.shape)}, {tuple(pick.shape)}, {tuple(noise.shape)}")
    return point_correspond(verts, trans, (u.float() - 0.5) * float(extent), thickness, pick=pick, noise=noise)


def _loss_args(pairs, inside, use_all, pred_bw, pred_fw, sigmas, deltas):
    a = L.mf_point_loss_args()
    a.Q, a.pairs, a.inside, a.use_all = pairs.shape[0], L.ptr(pairs), L.ptr(inside), int(use_all)
    a.pred_bw, a.pred_fw, a.n_nerfs = L.ptr(pred_bw), L.ptr(pred_fw), len(sigmas)
    for k, (s, d) in enumerate(zip(sigmas, deltas)):
        a.sigma[k], a.delta[k] = s.data_ptr(), float(d)
    return a


class _PointLossMeans(torch.autograd.Function):
    """(3,) fp32 = the means of nof_bw, nof_fw, alphas_mask (0 where a term is empty) of mf_point_loss_partials; backward
    mf_point_loss_partials_backward with the counts read on the device.  ``partials`` (6,) float64 is kept on the node."""

    @staticmethod
    def forward(ctx, pairs, inside, use_all, deltas, pred_bw, pred_fw, *sigmas):
        dev = pairs.device
        c = lambda t: None if t is None else t.detach().float().contiguous()
        pred_bw, pred_fw = c(pred_bw), c(pred_fw)
        ctx.sigma_shapes = [tuple(s.shape) for s in sigmas]
        sigmas = [c(s).reshape(-1) for s in sigmas]
        out6 = torch.empty(6, device=dev, dtype=torch.float64)
        means = torch.empty(3, device=dev, dtype=torch.float32)
        scratch = L.scratch(dev, "mf_point_loss_partials_scratch_bytes", pairs.shape[0])
        a = _loss_args(pairs, inside, use_all, pred_bw, pred_fw, sigmas, deltas)
        L.launch(dev, "mf_point_loss_partials", C.byref(a), out6.data_ptr(), means.data_ptr(), scratch.data_ptr())
        ctx.use_all, ctx.deltas, ctx.has = use_all, deltas, (pred_bw is not None, pred_fw is not None)
        keep = [pairs, out6] + ([inside] if inside is not None else []) + [t for t in (pred_bw, pred_fw) if t is not None] + sigmas
        ctx.has_inside = inside is not None
        ctx.save_for_backward(*keep)
        ctx.partials = out6
        return means

    @staticmethod
    def backward(ctx, g):
        saved = list(ctx.saved_tensors)
        pairs, out6 = saved[0], saved[1]
        k = 2
        inside = None
        if ctx.has_inside:
            inside, k = saved[k], k + 1
        pred_bw = pred_fw = None
        if ctx.has[0]:
            pred_bw, k = saved[k], k + 1
        if ctx.has[1]:
            pred_fw, k = saved[k], k + 1
        sigmas = saved[k:]
        dev, Q = pairs.device, pairs.shape[0]
        need = ctx.needs_input_grad
        seeds = g.detach().float().contiguous()
        g_bw = torch.empty((Q, 3), device=dev, dtype=torch.float32) if pred_bw is not None and need[4] else None
        g_fw = torch.empty((Q, 3), device=dev, dtype=torch.float32) if pred_fw is not None and need[5] else None
        g_sig = [torch.empty(ctx.sigma_shapes[i], device=dev, dtype=torch.float32) if need[6 + i] else None for i in range(len(sigmas))]
        a = _loss_args(pairs, inside, ctx.use_all, pred_bw, pred_fw, sigmas, ctx.deltas)
        L.launch(dev, "mf_point_loss_partials_backward", C.byref(a), out6.data_ptr(), seeds.data_ptr(), L.ptr(g_bw), L.ptr(g_fw),
                 L.ptr(g_sig[0]) if len(g_sig) > 0 else None, L.ptr(g_sig[1]) if len(g_sig) > 1 else None)
        return (None, None, None, None, g_bw, g_fw) + tuple(g_sig)


def loss_means(pairs, inside, pred_bw=None, pred_fw=None, sigmas=(), deltas=(), use_all=False):
    """The node alone: (3,) differentiable means [nof_bw, nof_fw, alphas_mask] of given predictions and raw densities."""
    L.require_gpu(pairs, "supervision.loss_means")
    if len(sigmas) != len(deltas) or len(sigmas) > 2:
        raise RuntimeError(f"supervision: {len(sigmas)} density planes with {len(deltas)} deltas (one delta per NeRF, at most two NeRFs)")
    Q = pairs.shape[0]
    for name, t, shape in (("pred_bw", pred_bw, (Q, 3)), ("pred_fw", pred_fw, (Q, 3))) + tuple(("sigma", s, None) for s in sigmas):
        if t is None:
            continue
        L.require_gpu(t, "supervision.loss_means")
        if (shape is not None and tuple(t.shape) != shape) or (shape is None and t.numel() != Q):
            raise RuntimeError(f"supervision: {name} is {tuple(t.shape)} for {Q} points")
    return _PointLossMeans.apply(pairs, inside, bool(use_all), tuple(float(d) for d in deltas), pred_bw, pred_fw, *sigmas)


def _nof_inputs(nof, exyz, ind_row, xyz):
    """[emb_xyz(xyz) zero-padded to in_channels_xyz | emb_ind(ind) zero-padded to extra_feat_dim], trainer_nof.py:96-108."""
    cols = [exyz.rows(xyz, width=nof.in_channels_xyz)]
    if nof.extra_feat_type == "ind":
        cols.append(F.pad(ind_row, (0, nof.extra_feat_dim - ind_row.shape[1])).expand(xyz.shape[0], -1))
    return torch.cat(cols, -1)


def point_losses(corr, ind, bw_nof, fw_nof, nof_embeddings, *, nerfs=(), nerf_embedding_xyz=None, deltas=(),
                 terms=TERMS, all_points=False, nof_loss="L1", msk_loss="BCE"):
    """The point losses of ``_shared_step`` (trainer_moco_flow.py:330-363; all_points=True: trainer_nof.py:115-125) on a
    Correspondence -> {term: 0-dim differentiable device scalar}, each the reference's value on its compacted set (unweighted;
    an empty set gives 0 where the reference gives NaN).

    ind: the image index as the NoF's embedding takes it, ``idx * 2 / num_frames - 1`` (a float or a one-element tensor).
    nof_embeddings: (nof_embedding_xyz, nof_embedding_ind).  nerfs, deltas: the NeRFs of ``alphas_mask`` (at most two) and the
    step length of each, 1 / N_samples and 1 / (N_samples + N_importance); nerf_embedding_xyz embeds the backward NoF's output.
    terms: which of "nof_bw", "nof_fw", "alphas_mask" to take -- only_msk_loss is terms=("alphas_mask",); fw_nof=None drops
    "nof_fw".  all_points: the L1 terms take every row (stage 2 concatenates both sets).
    The networks run on all Q rows through the existing module calls; one node reduces the three terms.  No host read."""
    if nof_loss != "L1":
        raise NotImplementedError(f"supervision.point_losses: nof_loss={nof_loss!r}; only 'L1' (nn.L1Loss) is built")
    if msk_loss != "BCE":
        raise NotImplementedError(f"supervision.point_losses: msk_loss={msk_loss!r}; only 'BCE' (nn.BCELoss) is built")
    terms = tuple(terms)
    for t in terms:
        if t not in TERMS:
            raise RuntimeError(f"supervision.point_losses: unknown term {t!r}; one of {TERMS}")
    nerfs, deltas = tuple(nerfs), tuple(deltas)
    if len(deltas) != len(nerfs):
        raise RuntimeError(f"supervision.point_losses: {len(deltas)} deltas for {len(nerfs)} NeRFs (one step length each)")
    if len(nerfs) > 2:
        raise RuntimeError(f"supervision.point_losses: {len(nerfs)} NeRFs; at most two (coarse and fine)")
    L.require_gpu(corr.pairs, "supervision.point_losses")
    if fw_nof is None:
        terms = tuple(t for t in terms if t != "nof_fw")
    want_msk = "alphas_mask" in terms
    if want_msk and (len(nerfs) == 0 or nerf_embedding_xyz is None):
        raise RuntimeError("supervision.point_losses: 'alphas_mask' needs nerfs, deltas and nerf_embedding_xyz")
    pairs, dev = corr.pairs, corr.pairs.device
    query, cano = pairs[:, :3].contiguous(), pairs[:, 3:].contiguous()
    exyz, eind = nof_embeddings
    ind_col = ind.detach().to(dev, torch.float32).reshape(1, 1) if isinstance(ind, torch.Tensor) else \
        torch.full((1, 1), float(ind), device=dev, dtype=torch.float32)
    ind_row = eind(ind_col)
    pred_bw = pred_fw = None
    if "nof_bw" in terms or want_msk:
        pred_bw = bw_nof(_nof_inputs(bw_nof, exyz, ind_row, query), query)
    if "nof_fw" in terms:
        pred_fw = fw_nof(_nof_inputs(fw_nof, exyz, ind_row, cano), cano)
    sigmas = []
    if want_msk:
        emb = nerf_embedding_xyz(pred_bw)                                                     # forwarf_nerf, :146-153
        for nerf in nerfs:
            x = F.pad(emb, (0, nerf.in_channels_xyz - emb.shape[1])) if emb.shape[1] < nerf.in_channels_xyz else emb
            sigmas.append(nerf(x, sigma_only=True))
    means = loss_means(pairs, corr.inside, pred_bw if "nof_bw" in terms else None, pred_fw, sigmas, deltas if want_msk else (),
                       use_all=all_points)
    return {t: means[TERMS.index(t)] for t in terms}
