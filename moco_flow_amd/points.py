"""Fused point queries: what the trainers spell as forward_nof -> embed ->
zero-pad -> NeRF(sigma_only=True) per 10 000-point chunk (trainer_moco_flow.py:146-187, 500-526;
trainer_nerf.py:215-245) as ONE launch over all points (mf_points_sigma), and the same for the whole of
NeRF.forward -- colour and density of free points (mf_points_radiance).  ``query_sigma_lattice`` evaluates a whole lattice
only where an occupancy grid is occupied (mf_lattice_select / _points / _scatter around the unchanged ``query_sigma``)."""
import ctypes as C

import numpy as np
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
    need = L.need("mf_points_sigma_workspace_bytes", prec, fd, 1 if ind_t is not None else 0, B) if fd is not None else 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev) if need > 0 else None     # bf16 + NoF: per-point index bias
    L.launch(dev, "mf_points_sigma_p", prec, nd, nb.data_ptr(), C.byref(ex), fd, L.ptr(fb), C.byref(fx) if fx is not None else None,
             C.byref(fi) if fi is not None else None, L.ptr(x), L.ptr(ind_t), ind_s, B, L.ptr(sigma), L.ptr(canon), L.ptr(ws), need)
    return (sigma, canon) if return_canonical else sigma


BRICK = 8                                       # lattice points per brick side (mf_lattice_*: 512 points per brick)
LATTICE_CHUNK_BRICKS = (2 ** 31 - 1) // BRICK ** 3   # bricks per query_sigma call: its rows stay below 2^31


def brick_cell_ranges(axis, margin, lo, hi, inv_cell, cells):
    """The (nb, 2) int32 table mf_lattice_select takes for one volume axis: per brick b of the ascending fp32 coordinates
    ``axis`` (n,), the inclusive first and last cell of a grid axis (``cells`` cells over [lo, hi], ``inv_cell`` cells per
    world unit) that the brick's grown index range [max(8b - margin, 0), min(8b + 7 + margin, n - 1)] touches, or the empty
    range (1, 0) where that range lies wholly outside [lo, hi].  The cell of a coordinate is mf_ray_clip's (occ_cell in
    csrc/mf_occupancy.hip), in fp32 with every operation rounded once: clamp(floor((c - lo) * inv_cell), 0, cells - 1)."""
    X = np.asarray(axis, dtype=np.float32).reshape(-1)
    n, cells = X.shape[0], int(cells)
    b = np.arange((n + BRICK - 1) // BRICK, dtype=np.int64)
    x0, x1 = X[np.maximum(BRICK * b - int(margin), 0)], X[np.minimum(BRICK * b + BRICK - 1 + int(margin), n - 1)]
    lo, hi, inv, top = np.float32(lo), np.float32(hi), np.float32(inv_cell), np.float32(cells - 1)

    def cell(x):
        with np.errstate(over="ignore", invalid="ignore"):
            f = np.floor((x - lo) * inv)
        f = np.where(f >= 0, f, np.float32(0))
        f = np.where(f <= top, f, top)
        return np.minimum(f.astype(np.int64), cells - 1)

    out = np.stack([cell(x0), cell(x1)], 1).astype(np.int32)
    out[(x1 < lo) | (x0 > hi)] = (1, 0)
    return out


def query_sigma_lattice(axes, nerf, nerf_embedding_xyz, occupancy, world_of_axis=(0, 1, 2), margin=1, fill=float("-inf"),
                        bw_nof=None, nof_embeddings=None, ind=None, precision=None, return_stats=False):
    """Raw sigma on a lattice, evaluated only where ``occupancy`` (an ``OccupancyGrid``) is occupied: the (n0, n1, n2) fp32
    volume, axis 2 fastest, that ``marching_cubes``, ``vertex_normals`` and ``OccupancyGrid.from_sigma`` take as it is.

    ``axes``: three 1-D ascending fp32 coordinate arrays for volume axes 0, 1, 2 -- numpy arrays or sequences on the host (a
    'cuda' tensor works and costs a read-back; a CPU tensor raises like everywhere in this package).  ``world_of_axis[a]``
    names the world coordinate axis a carries: (0, 1, 2) is ``OccupancyGrid.lattice``'s order, (1, 0, 2) ``mesh.lattice``'s
    'xy' order.  The lattice is cut into bricks of 8 x 8 x 8 points; a brick is ACTIVE iff an occupied cell lies in the box
    of grid cells that its index range, grown by ``margin`` >= 0 lattice points on every side, touches (``brick_cell_ranges``;
    a brick outside the grid's box is inactive).  Steps: select (mf_lattice_select), ONE device -> host read of the number of
    active bricks K -- as ``marching_cubes`` reads its counts --, the active bricks' points (mf_lattice_points), the unchanged
    ``query_sigma`` on them (in chunks of ``LATTICE_CHUNK_BRICKS`` bricks; K = 0 launches none), scatter
    (mf_lattice_scatter).  Everything runs on the current stream.  ``bw_nof`` / ``nof_embeddings`` / ``precision`` as
    ``query_sigma``; ``ind`` a scalar only (a per-point index tensor raises).  ``return_stats``: also (K, bricks).

    Guaranteed for any grid: every point of an active brick carries the value the dense ``query_sigma`` gives it, bit for
    bit (every kernel computes a sample independently of its place in the batch); every other point carries ``fill``.
    NOT guaranteed: that nothing above a threshold hides in an inactive brick.  A coarse pass can miss a thin part; that risk
    belongs to the caller's grid -- its ``dilate``, and a coarse threshold below the value looked for -- as
    ``OccupancyGrid.from_field`` warns for rays.  Nothing here picks a coarse threshold: nobody has validated one on a
    trained checkpoint."""
    who = "query_sigma_lattice"
    if len(axes) != 3:
        raise RuntimeError(f"{who}: axes must be three coordinate arrays, got {len(axes)}")
    woa = tuple(int(w) for w in world_of_axis)
    if sorted(woa) != [0, 1, 2]:
        raise RuntimeError(f"{who}: world_of_axis {world_of_axis!r} is not a permutation of (0, 1, 2)")
    margin = int(margin)
    if margin < 0:
        raise RuntimeError(f"{who}: margin={margin} (>= 0 lattice points)")
    if torch.is_tensor(ind) and ind.numel() > 1:
        raise RuntimeError(f"{who}: ind must be a scalar; a per-point index tensor has no lattice to belong to")
    par = next(nerf.parameters())
    L.require_gpu(par, who)
    dev = par.device
    if occupancy.device != dev:
        raise RuntimeError(f"{who}: the grid on {occupancy.device}, the networks on {dev}")
    host = []
    for a, t in enumerate(axes):
        if torch.is_tensor(t):
            L.require_gpu(t, who)
            t = t.detach().float().cpu().numpy()
        x = np.ascontiguousarray(np.asarray(t, dtype=np.float32))
        if x.ndim != 1 or x.shape[0] < 1 or not np.isfinite(x).all() or not (np.diff(x) >= 0).all():
            raise RuntimeError(f"{who}: axes[{a}] must be 1-D, finite and ascending, got shape {x.shape}")
        host.append(x)
    n = [int(x.shape[0]) for x in host]
    scratch = L.scratch(dev, "mf_lattice_select_scratch_bytes", *n)      # a bad shape is rejected here, before anything is copied
    bricks = int(np.prod([(v + BRICK - 1) // BRICK for v in n], dtype=np.int64))
    ranges = [brick_cell_ranges(host[a], margin, occupancy.lo[woa[a]], occupancy.hi[woa[a]], occupancy.inv_cell[woa[a]],
                                occupancy.dims[woa[a]]) for a in range(3)]
    woa_c = (C.c_int32 * 3)(*woa)
    with torch.no_grad(), torch.cuda.device(dev):
        tables = [torch.from_numpy(r).to(dev) for r in ranges]
        ax = [torch.from_numpy(x).to(dev) for x in host]
        slot = torch.empty(bricks, dtype=torch.int32, device=dev)
        ids = torch.empty(bricks, dtype=torch.int32, device=dev)
        count = torch.empty(1, dtype=torch.int64, device=dev)
        L.enqueue(dev, "mf_lattice_select", occupancy.bits.data_ptr(), *occupancy.dims, *(t.data_ptr() for t in tables), *n, woa_c,
                  slot.data_ptr(), ids.data_ptr(), count.data_ptr(), scratch.data_ptr())
        K = int(count.item())
        parts = []
        for k0 in range(0, K, LATTICE_CHUNK_BRICKS):
            kc = min(LATTICE_CHUNK_BRICKS, K - k0)
            pts = torch.empty((kc * BRICK ** 3, 3), dtype=torch.float32, device=dev)
            L.enqueue(dev, "mf_lattice_points", ids.data_ptr() + 4 * k0, kc, *(t.data_ptr() for t in ax), *n, woa_c, pts.data_ptr())
            parts.append(query_sigma(pts, nerf, nerf_embedding_xyz, bw_nof, nof_embeddings, ind, precision=precision))
            del pts
        sigma = None if not parts else parts[0] if len(parts) == 1 else torch.cat(parts)
        volume = torch.empty(n, dtype=torch.float32, device=dev)
        L.enqueue(dev, "mf_lattice_scatter", L.ptr(sigma), slot.data_ptr(), K, *n, float(fill), volume.data_ptr())
    return (volume, (K, bricks)) if return_stats else volume


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
    L.launch(dev, "mf_points_radiance", nd, nb.data_ptr(), C.byref(ex), ref(eext), fd, L.ptr(fb), ref(fx), ref(fi), L.ptr(x),
             L.ptr(dirs), L.ptr(ind_t), ind_s, B, L.ptr(out), L.ptr(canon))
    return (out, canon) if return_canonical else out
