"""Fused point queries: what the trainers spell as forward_nof -> embed ->
zero-pad -> NeRF(sigma_only=True) per 10 000-point chunk (trainer_moco_flow.py:146-187, 500-526;
trainer_nerf.py:215-245) as ONE launch over all points (mf_points_sigma), and the same for the whole of
NeRF.forward -- colour and density of free points (mf_points_radiance)."""
import ctypes as C

import torch

from . import _lib as L


def query_sigma(xyz, nerf, nerf_embedding_xyz, bw_nof=None, nof_embeddings=None, ind=None, return_canonical=False,
                precision=None):
    """xyz (B,3) observation-space points -> raw sigma (B,1) of the canonical NeRF.

    bw_nof / nof_embeddings=[xyz, ind] / ind: optional backward flow at image index ``ind`` (a python
    float in [-1,1) for all points, or a (B,) / (B,1) tensor); without them the query is made in
    canonical space (visualize_mesh with frame_idx == -1). Inference only.
    ``precision``: "f32" | "bf16" | "bf16x3" (None = the module setting of ``rendering.set_precision``); bf16 = hidden GEMMs
    on the bf16 matrix pipe as in render_rays' gradient-free passes (the mesh-extraction lattice ~8x faster); bf16x3 = the
    fp32-class three-product kernels (scalar ``ind`` or no NoF; with a per-point ``ind`` tensor the exact-fp32 kernel runs
    instead, so the setting never costs accuracy)."""
    from . import rendering
    prec = L.PRECISIONS[precision or rendering.PRECISION]
    if prec == L.MF_PREC_BF16X3 and bw_nof is not None and torch.is_tensor(ind) and ind.numel() > 1:
        prec = L.MF_PREC_F32
    L.require_gpu(xyz, "query_sigma")
    x = xyz.detach().float().contiguous()
    B = x.shape[0]
    dev = x.device
    sigma = torch.empty((B, 1), device=dev, dtype=torch.float32)
    canon = torch.empty((B, 3), device=dev, dtype=torch.float32) if (return_canonical and bw_nof is not None) else None
    nd, nb = nerf.packed(prec)
    ex = nerf_embedding_xyz.descriptor()
    fd = fb = fx = fi = None
    ind_t, ind_s = None, 0.0
    if bw_nof is not None:
        fd, fb = bw_nof.packed(prec)
        fx, fi = nof_embeddings[0].descriptor(), nof_embeddings[1].descriptor()
        if torch.is_tensor(ind):
            ind_t = ind.detach().float().reshape(-1).contiguous().to(dev)
            if ind_t.numel() == 1:
                ind_s, ind_t = float(ind_t.item()), None
            elif ind_t.numel() != B:
                raise RuntimeError(f"query_sigma: ind must have 1 or {B} elements")
        else:
            ind_s = float(ind)
    need = int(L.lib().mf_points_sigma_workspace_bytes(prec, fd, 1 if ind_t is not None else 0, B)) if fd is not None else 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev) if need > 0 else None     # bf16 + NoF: per-point index bias
    with torch.cuda.device(dev):
        L.check(L.lib().mf_points_sigma_p(prec, nd, nb.data_ptr(), C.byref(ex), fd, L.ptr(fb),
                                          C.byref(fx) if fx is not None else None,
                                          C.byref(fi) if fi is not None else None, L.ptr(x), L.ptr(ind_t), ind_s, B,
                                          L.ptr(sigma), L.ptr(canon), L.ptr(ws), need, L.current_stream(dev)), "mf_points_sigma")
    return (sigma, canon) if return_canonical else sigma


def _point_index(ind, B, dev, who):
    """``ind`` as query_sigma takes it -> (per-point (B,) tensor | None, scalar)."""
    if torch.is_tensor(ind):
        ind_t = ind.detach().float().reshape(-1).contiguous().to(dev)
        if ind_t.numel() == 1:
            return None, float(ind_t.item())
        if ind_t.numel() != B:
            raise RuntimeError(f"{who}: ind must have 1 or {B} elements")
        return ind_t, 0.0
    return None, float(ind)


def query_radiance(xyz, nerf, nerf_embeddings, view_dirs=None, ind=None, bw_nof=None, nof_embeddings=None,
                   return_canonical=False):
    """xyz (B,3) observation-space points -> (B,4) [rgb | raw sigma] of the canonical NeRF, the columns of NeRF.forward
    (models/nerf.py:101), fp32, one launch (mf_points_radiance).  Inference only.

    nerf_embeddings = [xyz, ind | None, dir | None] as render_rays takes it; the extra block follows nerf_inference
    (models/rendering.py:133-142): a "dir" NeRF embeds ``view_dirs`` (B,3) as given (nothing normalises it), an "ind" NeRF
    the image index ``ind``, a "none" NeRF nothing.  bw_nof / nof_embeddings=[xyz, ind] / ind: optional backward flow at
    image index ``ind`` -- a python float in [-1,1) for all points, or a (1,) / (B,) / (B,1) tensor -- the same value an
    "ind" NeRF embeds (render_rays reads ray column 8 for both).  ``return_canonical``: also the (B,3) points after the
    flow (None without a NoF)."""
    if nerf.extra_feat_type == "latent_code":
        raise NotImplementedError("NeRF model does not support latent code yet!!!")
    L.require_gpu(xyz, "query_radiance")
    x = xyz.detach().float().contiguous()
    if x.dim() != 2 or x.shape[1] != 3:
        raise RuntimeError(f"query_radiance: xyz must be (B, 3), got {tuple(xyz.shape)}")
    B = x.shape[0]
    dev = x.device
    kind = nerf.extra_feat_type
    dirs = eext = None
    if kind == "dir":
        if view_dirs is None:
            raise RuntimeError('query_radiance: a "dir" NeRF needs view_dirs (B, 3)')
        if tuple(view_dirs.shape) != (B, 3):
            raise RuntimeError(f"query_radiance: view_dirs must be ({B}, 3), got {tuple(view_dirs.shape)}")
        if len(nerf_embeddings) < 3 or nerf_embeddings[2] is None:
            raise RuntimeError('query_radiance: a "dir" NeRF needs nerf_embeddings[2], the dir embedding')
        dirs = view_dirs.detach().float().contiguous().to(dev)
        eext = nerf_embeddings[2].descriptor()
    elif kind == "ind":
        if len(nerf_embeddings) < 2 or nerf_embeddings[1] is None:
            raise RuntimeError('query_radiance: an "ind" NeRF needs nerf_embeddings[1], the ind embedding')
        eext = nerf_embeddings[1].descriptor()
    if (kind == "ind" or bw_nof is not None) and ind is None:
        raise RuntimeError('query_radiance: an "ind" NeRF and a NoF need the image index ind')
    ind_t, ind_s = _point_index(ind, B, dev, "query_radiance") if ind is not None else (None, 0.0)
    out = torch.empty((B, 4), device=dev, dtype=torch.float32)
    canon = torch.empty((B, 3), device=dev, dtype=torch.float32) if (return_canonical and bw_nof is not None) else None
    nd, nb = nerf.packed(L.MF_PREC_F32)
    ex = nerf_embeddings[0].descriptor()
    fd = fb = fx = fi = None
    if bw_nof is not None:
        if nof_embeddings is None or len(nof_embeddings) < 2:
            raise RuntimeError("query_radiance: a NoF needs nof_embeddings = [xyz, ind]")
        fd, fb = bw_nof.packed(L.MF_PREC_F32)
        fx, fi = nof_embeddings[0].descriptor(), nof_embeddings[1].descriptor()
    ref = lambda d: C.byref(d) if d is not None else None
    with torch.cuda.device(dev):
        L.check(L.lib().mf_points_radiance(nd, nb.data_ptr(), C.byref(ex), ref(eext), fd, L.ptr(fb), ref(fx), ref(fi), L.ptr(x),
                                           L.ptr(dirs), L.ptr(ind_t), ind_s, B, L.ptr(out), L.ptr(canon),
                                           L.current_stream(dev)), "mf_points_radiance")
    return (out, canon) if return_canonical else out
