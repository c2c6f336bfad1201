"""Mesh extraction on the device: marching cubes (mf_mc_count / mf_mc_emit) and visualize_mesh's pipeline around it
(trainer_moco_flow.py:485-548, trainer_nerf.py:200-259) -- sigma lattice, isosurface and the reference's post-processing
without the volume leaving the device -- and what a coloured mesh adds: vertex normals from the same volume
(mf_mc_normals), vertex colours from the radiance field (query_radiance), a PLY writer that carries both."""
import numpy as np
import torch

from . import _lib as L
from .points import query_radiance, query_sigma


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


def vertex_normals(volume, verts, clamp_zero=False):
    """Unit normals (V, 3) float32 of ``verts`` (V, 3), given in index coordinates of ``volume`` (n0, n1, n2) as
    marching_cubes returns them: minus the normalised gradient of the volume (of max(volume, 0) with ``clamp_zero``), so
    they point toward decreasing values -- out of the body for a density.  The gradient is central differences on the
    lattice (one-sided on a border face), interpolated along the vertex's lattice edge (include/mocoflow_hip.h
    mf_mc_normals); the zero vector where the gradient vanishes or is not finite."""
    L.require_gpu(volume, "vertex_normals")
    if volume.dim() != 3:
        raise RuntimeError(f"vertex_normals: volume must be 3-D, got shape {tuple(volume.shape)}")
    if verts.dim() != 2 or verts.shape[1] != 3:
        raise RuntimeError(f"vertex_normals: verts must be (V, 3), got shape {tuple(verts.shape)}")
    n0, n1, n2 = volume.shape
    lib = L.lib()
    need = int(lib.mf_mc_scratch_bytes(n0, n1, n2))
    if need < 0:                                     # bad shape: rejected before anything is copied
        L.check(need, "mf_mc_scratch_bytes")
    vol = volume.detach().float().contiguous()
    dev = vol.device
    v = verts.detach().float().contiguous().to(dev)
    V = v.shape[0]
    normals = torch.empty((V, 3), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        L.check(lib.mf_mc_normals(vol.data_ptr(), n0, n1, n2, 1 if clamp_zero else 0, L.ptr(v) if V else None, V,
                                  L.ptr(normals) if V else None, L.current_stream(dev)), "mf_mc_normals")
    return normals


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


def extract_colored_mesh(nerf, nerf_embeddings, N_grid=256, sigma_threshold=10, bw_nof=None, nof_embeddings=None, ind=None,
                         precision=None):
    """extract_mesh with what a coloured mesh needs: (verts (V, 3), tris (T, 3), normals (V, 3), colors (V, 3)).

    verts / tris are extract_mesh's for the same arguments (``nerf_embeddings`` = [xyz, ind | None, dir | None] as
    render_rays takes it; ``precision`` applies to the sigma lattice only).  normals: vertex_normals of the kept sigma
    volume (max(sigma, 0)), in the axes of the returned vertices (columns [1, 0, 2] like them; the uniform scale leaves
    directions alone) -- they point out of the body.  colors: query_radiance(...)[:, :3] at the returned vertices in fp32,
    through the same NoF / ``ind``; a "dir" NeRF is looked at straight on, view_dirs = -normal ((0, 0, -1) where the
    normal is zero).  An empty mesh gives four empty tensors."""
    dev = next(nerf.parameters()).device
    L.require_gpu(next(nerf.parameters()), "extract_colored_mesh")
    xyz = lattice(N_grid, dev)
    with torch.no_grad():
        sigma = query_sigma(xyz, nerf, nerf_embeddings[0], bw_nof, nof_embeddings, ind, precision=precision)
        del xyz
        volume = sigma.view(N_grid, N_grid, N_grid)
        raw, tris = marching_cubes(volume, sigma_threshold, clamp_zero=True)
        normals = vertex_normals(volume, raw, clamp_zero=True)[:, [1, 0, 2]].contiguous()
        del sigma, volume
        verts = raw[:, [1, 0, 2]] / N_grid * 3.0 - 1.5
        tris = tris[:, [0, 2, 1]].contiguous()
        if verts.shape[0] == 0:
            return verts, tris, normals, torch.empty((0, 3), dtype=torch.float32, device=dev)
        view_dirs = None
        if nerf.extra_feat_type == "dir":
            zero = (normals == 0).all(1, keepdim=True)
            view_dirs = torch.where(zero, normals.new_tensor([0.0, 0.0, -1.0]), -normals)
        colors = query_radiance(verts, nerf, nerf_embeddings, view_dirs=view_dirs, ind=ind, bw_nof=bw_nof,
                                nof_embeddings=nof_embeddings)[:, :3].contiguous()
    return verts, tris, normals, colors


def export_ply(path, verts, tris, colors=None, normals=None):
    """Binary little-endian PLY: vertex properties x y z (float), optionally nx ny nz (float) and red green blue (uchar,
    clamp(round(255 c), 0, 255) of colours in [0, 1]) -- write_ply_rgb's names and types (utils/vis_utils.py:19-25) -- and
    the faces as ``list uchar int vertex_indices``."""
    def host(a, dtype):
        return a.detach().cpu().numpy().astype(dtype) if torch.is_tensor(a) else np.asarray(a, dtype)

    v = host(verts, np.float32).reshape(-1, 3)
    f = host(tris, np.int64).reshape(-1, 3)
    fields, cols = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")], [v]
    if normals is not None:
        n = host(normals, np.float32).reshape(-1, 3)
        if len(n) != len(v):
            raise RuntimeError(f"export_ply: {len(n)} normals for {len(v)} vertices")
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
        cols.append(n)
    if colors is not None:
        c = host(colors, np.float64).reshape(-1, 3)
        if len(c) != len(v):
            raise RuntimeError(f"export_ply: {len(c)} colours for {len(v)} vertices")
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        cols.append(np.clip(np.rint(255.0 * np.nan_to_num(c)), 0, 255).astype(np.uint8))
    if len(f) and (f.min() < 0 or f.max() >= len(v) or len(v) > 2 ** 31 - 1):
        raise RuntimeError("export_ply: triangle index out of range")
    vrec = np.empty(len(v), dtype=fields)
    k = 0
    for col in cols:
        for j in range(3):
            vrec[fields[k][0]] = col[:, j]
            k += 1
    frec = np.empty(len(f), dtype=[("n", "u1"), ("i", "<i4", (3,))])
    frec["n"] = 3
    frec["i"] = f
    kinds = {"<f4": "float", "u1": "uchar"}
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}"]
    header += [f"property {kinds[t]} {name}" for name, t in fields]
    header += [f"element face {len(f)}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(vrec.tobytes())
        fh.write(frec.tobytes())


def export_obj(path, verts, tris):
    """mcubes.export_obj: ``v x y z`` lines, then 1-based ``f i j k`` lines."""
    v = verts.detach().cpu().double().numpy() if torch.is_tensor(verts) else np.asarray(verts, np.float64)
    f = tris.detach().cpu().numpy() if torch.is_tensor(tris) else np.asarray(tris)
    with open(path, "w") as fh:
        if len(v):
            fh.write("\n".join("v %.9g %.9g %.9g" % tuple(r) for r in v) + "\n")
        if len(f):
            fh.write("\n".join("f %d %d %d" % tuple(r) for r in (f.astype(np.int64) + 1)) + "\n")
