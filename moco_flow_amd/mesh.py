"""Mesh extraction on the device: marching cubes (mf_mc_count / mf_mc_emit) and visualize_mesh's pipeline around it
(trainer_moco_flow.py:485-548, trainer_nerf.py:200-259) -- sigma lattice, isosurface and the reference's post-processing
without the volume leaving the device."""
import numpy as np
import torch

from . import _lib as L
from .points import query_sigma


def marching_cubes(volume, isovalue, clamp_zero=False):
    """Device counterpart of ``mcubes.marching_cubes(volume, isovalue)``: volume (n0, n1, n2) on a 'cuda' device, each side
    >= 2 and at most 2^31 - 1 points -> (verts (V, 3) float32, tris (T, 3) int64) on the same device, vertices in index
    coordinates of the volume's own axes.  ``clamp_zero``: mesh max(volume, 0) without another pass over the volume.

    Classic Lorensen-Cline cases (scikit-image's triangulation and winding, mf_mc_tables.hpp); a corner is inside iff
    v < isovalue; vertices sorted by lattice edge, triangles by cell: the output is deterministic (include/mocoflow_hip.h
    mf_mc_*).  A non-contiguous or non-fp32 volume is copied to a contiguous fp32 one first.  One device -> host read (the
    two counts)."""
    L.require_gpu(volume, "marching_cubes")
    if volume.dim() != 3:
        raise RuntimeError(f"marching_cubes: volume must be 3-D, got shape {tuple(volume.shape)}")
    n0, n1, n2 = volume.shape
    lib = L.lib()
    need = int(lib.mf_mc_scratch_bytes(n0, n1, n2))
    if need < 0:                                     # bad shape: rejected before anything is allocated or copied
        L.check(need, "mf_mc_scratch_bytes")
    vol = volume.detach().float().contiguous()
    dev = vol.device
    scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    iso, clamp = float(isovalue), 1 if clamp_zero else 0
    with torch.cuda.device(dev):
        stream = L.current_stream(dev)
        L.check(lib.mf_mc_count(vol.data_ptr(), n0, n1, n2, iso, clamp, scratch.data_ptr(), counts.data_ptr(), stream),
                "mf_mc_count")
        V, T = (int(x) for x in counts.tolist())
        verts = torch.empty((V, 3), dtype=torch.float32, device=dev)
        tris = torch.empty((T, 3), dtype=torch.int64, device=dev)
        L.check(lib.mf_mc_emit(vol.data_ptr(), n0, n1, n2, iso, clamp, scratch.data_ptr(), L.ptr(verts) if V else None,
                               L.ptr(tris) if T else None, stream), "mf_mc_emit")
    return verts, tris


def lattice(N_grid, device):
    """visualize_mesh's query points (trainer_moco_flow.py:490-498): np.linspace(-1.5, 1.5, N) in float64 cast to fp32, laid
    out as np.stack(np.meshgrid(x, y, z), -1).reshape(-1, 3) ('xy' indexing: point (a, b, c) is (x[b], y[a], z[c]))."""
    ax = torch.from_numpy(np.linspace(-1.5, 1.5, N_grid).astype(np.float32)).to(device)
    N = N_grid
    return torch.stack([ax.view(1, N, 1).expand(N, N, N), ax.view(N, 1, 1).expand(N, N, N),
                        ax.view(1, 1, N).expand(N, N, N)], -1).reshape(-1, 3)


def extract_mesh(nerf, nerf_embedding_xyz, N_grid=256, sigma_threshold=10, bw_nof=None, nof_embeddings=None, ind=None,
                 precision=None):
    """visualize_mesh (trainer_moco_flow.py:490-538) up to the file: raw sigma of the NeRF on the N_grid^3 lattice over
    [-1.5, 1.5]^3 (query_sigma; with ``bw_nof`` / ``nof_embeddings`` / ``ind`` through the backward flow, ``ind`` =
    frame_idx * 2 / num_frames - 1), the isosurface of max(sigma, 0) at ``sigma_threshold``, then the reference's
    post-processing: vertex columns 0 and 1 swapped, triangle columns 1 and 2 swapped, vertices / N_grid * 3 - 1.5 (the
    reference divides by N_grid, not N_grid - 1).  Returns (verts (V, 3) float32, tris (T, 3) int64) on the NeRF's device;
    ``export_obj`` writes them."""
    dev = next(nerf.parameters()).device
    L.require_gpu(next(nerf.parameters()), "extract_mesh")
    xyz = lattice(N_grid, dev)
    with torch.no_grad():
        sigma = query_sigma(xyz, nerf, nerf_embedding_xyz, bw_nof, nof_embeddings, ind, precision=precision)
        del xyz
        verts, tris = marching_cubes(sigma.view(N_grid, N_grid, N_grid), sigma_threshold, clamp_zero=True)
        verts = verts[:, [1, 0, 2]] / N_grid * 3.0 - 1.5
        tris = tris[:, [0, 2, 1]].contiguous()
    return verts, tris


def export_obj(path, verts, tris):
    """mcubes.export_obj: ``v x y z`` lines, then 1-based ``f i j k`` lines."""
    v = verts.detach().cpu().double().numpy() if torch.is_tensor(verts) else np.asarray(verts, np.float64)
    f = tris.detach().cpu().numpy() if torch.is_tensor(tris) else np.asarray(tris)
    with open(path, "w") as fh:
        if len(v):
            fh.write("\n".join("v %.9g %.9g %.9g" % tuple(r) for r in v) + "\n")
        if len(f):
            fh.write("\n".join("f %d %d %d" % tuple(r) for r in (f.astype(np.int64) + 1)) + "\n")
