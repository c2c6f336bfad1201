"""Mesh extraction on the device: marching cubes (mf_mc_count / mf_mc_emit) and visualize_mesh's pipeline around it
(trainer_moco_flow.py:485-548, trainer_nerf.py:200-259) -- sigma lattice, isosurface and the reference's post-processing
without the volume leaving the device -- and what a coloured mesh adds: vertex normals from the same volume
(mf_mc_normals), vertex colours from the radiance field (query_radiance), a PLY writer that carries both; and the mesh
clean-up that follows an isosurface at a fixed threshold: connected components (mf_mesh_label, mf_mesh_table_*) and the
filter on them (mf_mesh_filter_*, mf_gather_rows) -- the body kept, the detached specks dropped, on the device; the
reduction of the triangle count by vertex clustering (simplify_mesh: mf_simplify_mesh_*); and vertex adjacency with the
smoothing built on it (vertex_rings: mf_rings_mesh_*, smooth_mesh: mf_smooth_mesh); and how far two meshes are apart
(MeshIndex, closest_point, sample_surface, surface_distance: mf_surface_*); and rays against a mesh -- the first hit, any hit,
what a camera sees of it (cast_rays, visible_from: mf_surface_corners, mf_surface_cast)."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib as L
from .points import query_radiance, query_sigma, query_sigma_lattice


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
    dev = volume.device
    scratch = L.scratch(dev, "mf_mc_scratch_bytes", n0, n1, n2)     # a bad shape is rejected here, before anything is copied
    vol = volume.detach().float().contiguous()
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    iso, clamp = float(isovalue), 1 if clamp_zero else 0
    with torch.cuda.device(dev):
        L.enqueue(dev, "mf_mc_count", vol.data_ptr(), n0, n1, n2, iso, clamp, scratch.data_ptr(), counts.data_ptr())
        V, T = (int(x) for x in counts.tolist())
        verts = torch.empty((V, 3), dtype=torch.float32, device=dev)
        tris = torch.empty((T, 3), dtype=torch.int64, device=dev)
        L.enqueue(dev, "mf_mc_emit", vol.data_ptr(), n0, n1, n2, iso, clamp, scratch.data_ptr(), L.ptr0(verts), L.ptr0(tris))
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
    L.need("mf_mc_scratch_bytes", n0, n1, n2)        # bad shape: rejected before anything is copied
    vol = volume.detach().float().contiguous()
    dev = vol.device
    v = verts.detach().float().contiguous().to(dev)
    V = v.shape[0]
    normals = torch.empty((V, 3), dtype=torch.float32, device=dev)
    L.launch(dev, "mf_mc_normals", vol.data_ptr(), n0, n1, n2, 1 if clamp_zero else 0, L.ptr0(v), V, L.ptr0(normals))
    return normals


def _check_tris(tris, what):
    if tris.dim() != 2 or tris.shape[1] != 3:
        raise RuntimeError(f"{what}: tris must be (T, 3), got shape {tuple(tris.shape)}")
    if tris.dtype != torch.int64:
        raise RuntimeError(f"{what}: tris must be int64, got {tris.dtype}")


def _label(tris, V, bad):
    """Launch the labelling of a checked, contiguous (T, 3) int64 device tensor: labels (V,); the bad-index counter goes to
    ``bad`` (device int64 storage).  No host read."""
    dev, T = tris.device, tris.shape[0]
    scratch = L.scratch(dev, "mf_mesh_label_scratch_bytes", V, T)    # V or T beyond 32-bit indexing: rejected here
    labels = torch.empty(V, dtype=torch.int64, device=dev)
    L.launch(dev, "mf_mesh_label", L.ptr0(tris), T, V, L.ptr0(labels), bad.data_ptr(), scratch.data_ptr())
    return labels


def _table(tris, V, labels, counts, what):
    """The component table of labelled triangles: (ids, tri_counts, vert_counts).  ``counts``: device int64[3] whose entry
    0 a labelling on the same stream has filled; one device -> host read ([bad, C, bad])."""
    dev, T = tris.device, tris.shape[0]
    scratch = L.scratch(dev, "mf_mesh_table_scratch_bytes", V, T)
    with torch.cuda.device(dev):
        L.enqueue(dev, "mf_mesh_table_count", L.ptr0(tris), T, V, L.ptr0(labels), counts.data_ptr() + 8, scratch.data_ptr())
        bad, C, bad2 = (int(x) for x in counts.tolist())
        if bad or bad2:
            raise RuntimeError(f"{what}: {max(bad, bad2)} triangles name a vertex outside [0, {V})")
        ids, tri_counts, vert_counts = (torch.empty(C, dtype=torch.int64, device=dev) for _ in range(3))
        L.enqueue(dev, "mf_mesh_table_emit", V, C, scratch.data_ptr(), L.ptr0(ids), L.ptr0(tri_counts), L.ptr0(vert_counts))
    return ids, tri_counts, vert_counts


def _components(tris, V, what):
    """Labels and table of a checked, contiguous (T, 3) int64 device tensor; one device -> host read."""
    counts = torch.empty(3, dtype=torch.int64, device=tris.device)      # [bad of the labelling, C, bad of the table]
    labels = _label(tris, V, counts)
    return (labels,) + _table(tris, V, labels, counts, what)


def mesh_components(tris, n_verts):
    """Connected components of an indexed mesh: tris (T, 3) int64 on a 'cuda' device over ``n_verts`` vertices ->
    (labels (V,), ids (C,), tri_counts (C,), vert_counts (C,)), all int64 on that device.

    Two vertices are adjacent if some triangle names both (a triangle may repeat an index, a mesh may repeat a triangle);
    labels[v] is the smallest vertex index of v's component, a vertex in no triangle being a component of its own with no
    triangles; ids are the distinct labels, ascending; a triangle counts for the component of its column-0 vertex.  Every
    output is a pure function of the input, bit-identical from run to run (include/mocoflow_hip.h mf_mesh_label).  V and
    T below 2^31.  An index outside [0, n_verts) is never dereferenced and raises RuntimeError.  One device -> host read
    (the number of components with the bad-index counters)."""
    _check_tris(tris, "mesh_components")
    V = int(n_verts)
    if V < 0:
        raise RuntimeError(f"mesh_components: n_verts={V}")
    L.require_gpu(tris, "mesh_components")
    return _components(tris.detach().contiguous(), V, "mesh_components")


def gather_rows(src, inds):
    """src[inds] along dim 0 for a contiguous device tensor of any dtype, as a byte copy (mf_gather_rows)."""
    dev, n = src.device, inds.shape[0]
    out = torch.empty((n,) + tuple(src.shape[1:]), dtype=src.dtype, device=dev)
    row_bytes = int(np.prod(src.shape[1:], dtype=np.int64)) * src.element_size()
    if n and row_bytes:
        L.launch(dev, "mf_gather_rows", src.data_ptr(), src.shape[0], row_bytes, inds.data_ptr(), n, out.data_ptr())
    return out


def filter_components(verts, tris, keep_largest=None, min_triangles=None, attrs=()):
    """Keep whole connected components of a mesh: verts (V, ...) and tris (T, 3) int64 on a 'cuda' device ->
    (verts, tris, *attrs) of the kept components, triangle indices rewritten to the kept vertices.

    Components as mesh_components defines them, ranked by triangle count (descending), then label (ascending):
    ``keep_largest=k`` keeps the first k in that order, ``min_triangles=m`` those with at least m triangles, both given
    their intersection; neither is a ValueError, as is k < 1.  Every vertex of a dropped component goes, a vertex in no
    triangle included (it is a component without triangles).  Kept vertices and triangles stay in their original order;
    vertex rows and the rows of every tensor in ``attrs`` (each (V, ...), any dtype) are copied byte for byte.  Nothing
    kept: (0, ...) tensors.  Two device -> host reads: the labelling's (the number of components) and one for the kept
    counts with the bad-index counter."""
    if keep_largest is None and min_triangles is None:
        raise ValueError("filter_components: give keep_largest, min_triangles or both")
    if keep_largest is not None and int(keep_largest) < 1:
        raise ValueError(f"filter_components: keep_largest={keep_largest} (at least 1)")
    _check_tris(tris, "filter_components")
    if verts.dim() < 1:
        raise RuntimeError("filter_components: verts must be (V, ...)")
    V, T = verts.shape[0], tris.shape[0]
    attrs = tuple(attrs)
    for i, a in enumerate(attrs):
        if a.dim() < 1 or a.shape[0] != V:
            raise RuntimeError(f"filter_components: attrs[{i}] has shape {tuple(a.shape)} for {V} vertices")
    for t in (tris, verts) + attrs:
        L.require_gpu(t, "filter_components")
    tris = tris.detach().contiguous()
    labels, ids, tri_counts, _ = _components(tris, V, "filter_components")
    keep = _keep(ids, tri_counts, V, T, keep_largest, min_triangles)
    return _filter(verts, tris, labels, ids, keep, attrs)


def _keep(ids, tri_counts, V, T, keep_largest, min_triangles):
    """The per-component decision (C,) uint8 from the table, with torch ops on the table's device."""
    C = ids.shape[0]
    keep = torch.ones(C, dtype=torch.bool, device=ids.device)
    if keep_largest is not None and int(keep_largest) < C:
        # rank key (T - triangles) V' + label, V' = max(V, 1): distinct per component (labels are), below 2^62 -- no tie is
        # left to the sort
        order = torch.argsort((T - tri_counts) * max(V, 1) + ids)
        keep = torch.zeros(C, dtype=torch.bool, device=ids.device)
        keep[order[:int(keep_largest)]] = True
    if min_triangles is not None:
        keep &= tri_counts >= int(min_triangles)
    return keep.to(torch.uint8)


def _filter(verts, tris, labels, ids, keep, attrs=()):
    """The mesh of the components whose ``keep`` (C,) uint8 is set; one device -> host read ([Vk, Tk, bad])."""
    dev = tris.device
    V, T, C = verts.shape[0], tris.shape[0], ids.shape[0]
    scratch = L.scratch(dev, "mf_mesh_filter_scratch_bytes", V, T)
    counts = torch.empty(3, dtype=torch.int64, device=dev)
    tp = L.ptr0(tris)
    with torch.cuda.device(dev):
        L.enqueue(dev, "mf_mesh_filter_plan", tp, T, V, L.ptr0(labels), L.ptr0(ids), L.ptr0(keep), C, counts.data_ptr(),
                  scratch.data_ptr())
        Vk, Tk, bad = (int(x) for x in counts.tolist())
        if bad:
            raise RuntimeError(f"filter_components: {bad} triangles name a vertex outside [0, {V})")
        vert_inds = torch.empty(Vk, dtype=torch.int64, device=dev)
        tri_inds = torch.empty(Tk, dtype=torch.int64, device=dev)
        tris_out = torch.empty((Tk, 3), dtype=torch.int64, device=dev)
        L.enqueue(dev, "mf_mesh_filter_emit", tp, T, V, Vk, Tk, scratch.data_ptr(), L.ptr0(vert_inds), L.ptr0(tri_inds),
                  L.ptr0(tris_out))
    return (gather_rows(verts.detach().contiguous(), vert_inds), tris_out,
            *(gather_rows(a.detach().contiguous(), vert_inds) for a in attrs))


def _simplify_grid(lo, hi, cell):
    """Cells per axis of the clustering grid, in float64 on the host: n_a = floor((hi_a - lo_a) / cell) + 1."""
    if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
        raise RuntimeError(f"simplify_mesh: lo={lo.tolist()} hi={hi.tolist()} (a vertex that is not finite, or a bound that is not)")
    if (hi < lo).any():
        raise ValueError(f"simplify_mesh: hi={hi.tolist()} below lo={lo.tolist()}")
    return [int(min(x, 2.0 ** 31)) for x in np.floor((hi - lo) / cell) + 1.0]     # 2^31 on an axis: the library refuses it


def simplify_mesh(verts, tris, cell, lo=None, hi=None, placement="mean", attrs=(), return_map=False, _slots=None):
    """Vertex clustering on the device: verts (V, 3) float32 and tris (T, 3) int64 on a 'cuda' device ->
    (verts_k (Vk, 3) float32, tris_k (Tk, 3) int64, *attrs_k[, first (Vk,) int64, cluster (V,) int64]), the last two with
    ``return_map``.

    ``cell`` > 0 is the edge of a cubic cell in the vertices' own units; ``lo`` / ``hi`` are 3-vectors of host floats and
    default to verts.amin(0) / verts.amax(0), which costs one more device -> host read.  Cells per axis n_a =
    floor((hi_a - lo_a) / cell) + 1 in float64; n0 n1 n2, V and T below 2^31, refused before anything is allocated.  The
    cell of a vertex, per axis in float64: t = (double(v) - lo) / cell, c = floor(t), id = (c0 n1 + c1) n2 + c2.  A vertex
    that is not finite or lies outside [lo, hi] on an axis, and a triangle with an index outside [0, V), raise RuntimeError:
    nothing is clamped, a bad index is never dereferenced.

    A triangle is dropped as degenerate if two of its three cells are equal.  Two others are duplicates if their cell
    triples are equal up to cyclic rotation (the same cells in the opposite winding are not); of each class the triangle
    with the smallest original index survives; survivors keep their order and their corner order.  The new vertices are the
    cells a survivor names, ascending by cell id; every other vertex is dropped, cluster[v] = -1 (a vertex in no triangle,
    a vertex of a cell only degenerate triangles name); first[k] = the smallest original index in cell k, cluster[v] = the
    new index of v's cell.  Rows first[k] of every tensor in ``attrs`` (each (V, ...), any dtype) are copied byte for byte
    (mf_gather_rows).  ``placement="first"``: verts_k[k] = verts[first[k]] byte for byte -- the vertex stays on its lattice
    edge, so vertex_normals stays valid for it.  ``placement="mean"``: the exact mean of the cell's members in fixed point,
    q = llrint((t - c) 2^20) per axis, S = the int64 sum over the n members, verts_k = float32(lo + cell (c + (S / n) / 2^20)),
    each operation rounded once in float64: integer atomics make it independent of their order.  Every output is a pure
    function of the input, bit-identical from run to run (include/mocoflow_hip.h mf_simplify_mesh_*).  Nothing kept:
    (0, ...) tensors; V = 0 or T = 0 is legal.  One device -> host read ([Vk, Tk, bad]) besides the one of the defaults.

    ``_slots`` (private, for tests): the size of the duplicate table, a power of two above T; default the next power of
    two >= 2 T + 1."""
    if placement not in ("mean", "first"):
        raise ValueError(f"simplify_mesh: placement={placement!r} ('mean' or 'first')")
    _check_tris(tris, "simplify_mesh")
    if verts.dim() != 2 or verts.shape[1] != 3:
        raise RuntimeError(f"simplify_mesh: verts must be (V, 3), got shape {tuple(verts.shape)}")
    if verts.dtype != torch.float32:
        raise RuntimeError(f"simplify_mesh: verts must be float32, got {verts.dtype}")
    V, T = verts.shape[0], tris.shape[0]
    attrs = tuple(attrs)
    for i, a in enumerate(attrs):
        if a.dim() < 1 or a.shape[0] != V:
            raise RuntimeError(f"simplify_mesh: attrs[{i}] has shape {tuple(a.shape)} for {V} vertices")
    cell = float(cell)
    if not (cell > 0.0 and np.isfinite(cell)):
        raise ValueError(f"simplify_mesh: cell={cell} (a finite edge above 0)")
    if (lo is None) != (hi is None):
        raise ValueError("simplify_mesh: give both lo and hi, or neither")
    if lo is not None:
        lo, hi = np.asarray(lo, np.float64).reshape(-1), np.asarray(hi, np.float64).reshape(-1)
        if lo.shape != (3,) or hi.shape != (3,):
            raise ValueError("simplify_mesh: lo and hi are 3-vectors")
        n = _simplify_grid(lo, hi, cell)
    for t in (tris, verts) + attrs:
        L.require_gpu(t, "simplify_mesh")
    verts, tris = verts.detach().contiguous(), tris.detach().contiguous()
    if lo is None:
        if V:
            ends = torch.stack([verts.amin(0), verts.amax(0)]).double().cpu().numpy()      # the extra read
        else:
            ends = np.zeros((2, 3))
        lo, hi = ends[0], ends[1]
        n = _simplify_grid(lo, hi, cell)
    slots = int(_slots) if _slots is not None else min(1 << (2 * T).bit_length(), 1 << 31)
    dbl3 = C.c_double * 3
    grid = (dbl3(*lo.tolist()), dbl3(*hi.tolist()), cell, *n)
    scratch, counts = _simplify_plan(verts, tris, grid, slots)
    Vk, Tk, bad = (int(x) for x in counts.tolist())
    if bad:
        raise RuntimeError(f"simplify_mesh: {bad} vertices that are not finite or lie outside [lo, hi], or triangles that name "
                           f"a vertex outside [0, {V})")
    verts_k, tris_k, first, cluster = _simplify_emit(verts, tris, grid, scratch, Vk, Tk, placement == "mean")
    if verts_k is None:
        verts_k = gather_rows(verts, first)
    out = (verts_k, tris_k, *(gather_rows(a.detach().contiguous(), first) for a in attrs))
    return out + (first, cluster) if return_map else out


def _simplify_plan(verts, tris, grid, slots):
    """Launch the planning step on checked, contiguous device tensors: (scratch, counts), counts = device int64 [Vk, Tk, bad].
    ``grid`` = (lo, hi, cell, n0, n1, n2), lo and hi as ctypes double[3].  No host read."""
    dev, V, T = tris.device, verts.shape[0], tris.shape[0]
    # too many cells, V, T or a bad table size: rejected before anything is allocated
    scratch = L.scratch(dev, "mf_simplify_mesh_scratch_bytes", V, T, *grid[3:], slots)
    counts = torch.empty(3, dtype=torch.int64, device=dev)
    L.launch(dev, "mf_simplify_mesh_plan", L.ptr0(verts), V, L.ptr0(tris), T, *grid, slots, counts.data_ptr(),
             scratch.data_ptr())
    return scratch, counts


def _simplify_emit(verts, tris, grid, scratch, Vk, Tk, mean):
    """The emit step after the plan on the same stream, with the counts read: (verts_k or None, tris_k, first, cluster);
    verts_k only for the mean placement."""
    dev, V, T = tris.device, verts.shape[0], tris.shape[0]
    verts_k = torch.empty((Vk, 3), dtype=torch.float32, device=dev) if mean else None
    sums = torch.empty(28 * Vk, dtype=torch.uint8, device=dev) if mean and Vk else None
    tris_k = torch.empty((Tk, 3), dtype=torch.int64, device=dev)
    first = torch.empty(Vk, dtype=torch.int64, device=dev)
    cluster = torch.empty(V, dtype=torch.int64, device=dev)
    L.launch(dev, "mf_simplify_mesh_emit", L.ptr0(verts), V, L.ptr0(tris), T, *grid, Vk, Tk, scratch.data_ptr(), L.ptr(sums),
             L.ptr0(verts_k), L.ptr0(tris_k), L.ptr0(first), L.ptr0(cluster))
    return verts_k, tris_k, first, cluster


MAX_TRIANGLES_PER_VERTEX = 2048          # include/mocoflow_hip.h MF_MESH_MAX_TRIANGLES_PER_VERTEX


def _rings(tris, V, what):
    """vertex_rings on a checked, contiguous (T, 3) int64 device tensor; one device -> host read ([bad, over_cap, R])."""
    dev, T = tris.device, tris.shape[0]
    scratch = L.scratch(dev, "mf_rings_mesh_scratch_bytes", V, T)    # V or 6 T beyond 32-bit indexing: rejected here
    counts = torch.empty(3, dtype=torch.int64, device=dev)
    offsets = torch.empty(V + 1, dtype=torch.int64, device=dev)
    boundary = torch.empty(V, dtype=torch.bool, device=dev)
    with torch.cuda.device(dev):
        L.enqueue(dev, "mf_rings_mesh_plan", L.ptr0(tris), T, V, counts.data_ptr(), offsets.data_ptr(), L.ptr0(boundary),
                  scratch.data_ptr())
        bad, over, R = (int(x) for x in counts.tolist())
        if bad:
            raise RuntimeError(f"{what}: {bad} triangles name a vertex outside [0, {V})")
        if over:
            raise RuntimeError(f"{what}: {over} vertices are in more than MAX_TRIANGLES_PER_VERTEX = "
                               f"{MAX_TRIANGLES_PER_VERTEX} triangles")
        ring = torch.empty(R, dtype=torch.int64, device=dev)
        L.enqueue(dev, "mf_rings_mesh_emit", V, T, R, scratch.data_ptr(), offsets.data_ptr(), L.ptr0(ring))
    return offsets, ring, boundary


def vertex_rings(tris, n_verts):
    """The one-ring of every vertex of an indexed mesh as a CSR structure: tris (T, 3) int64 on a 'cuda' device over
    ``n_verts`` = V vertices -> (offsets (V + 1,) int64, ring (R,) int64, boundary (V,) bool) on that device.

    A triangle that names a vertex outside [0, V) makes the call raise RuntimeError with the count: a bad index is counted
    and never dereferenced, and no ring is written for that call.  A triangle with two equal indices is skipped entirely
    and contributes no edge; it is not an error (simplify_mesh and real meshes produce them).  m(i, j) is the number of
    remaining triangles that contain both i and j, i != j.  ring(i) = { j : m(i, j) >= 1 }, stored ascending by j, each j
    once, at ring[offsets[i] : offsets[i + 1]] -- the same triangle twice, or in both windings, changes m and not the
    ring.  boundary[i] is true iff some j has m(i, j) == 1: an edge in three or more triangles (non-manifold) does not make
    its ends boundary; a vertex in no kept triangle has an empty ring and is not boundary.

    Bounds: V < 2^31 and 6 T < 2^31 (R <= 6 T), refused on the host before anything is allocated.  A vertex in more than
    ``MAX_TRIANGLES_PER_VERTEX`` kept triangles raises RuntimeError naming the count of such vertices: it is found in the
    counting pass, before any segment is sorted, so no lane does work quadratic in an unbounded degree.  V = 0 and T = 0
    are legal: offsets all zero, an empty ring.  Every output is a pure function of the input, bit-identical from run to
    run whatever order the atomics land in (include/mocoflow_hip.h mf_rings_mesh_plan).  One device -> host read
    ([bad, over_cap, R])."""
    _check_tris(tris, "vertex_rings")
    V = int(n_verts)
    if V < 0:
        raise RuntimeError(f"vertex_rings: n_verts={V}")
    L.require_gpu(tris, "vertex_rings")
    return _rings(tris.detach().contiguous(), V, "vertex_rings")


def _smooth_args(iterations, lam, mu, boundary, what="smooth_mesh"):
    if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or iterations < 0:
        raise ValueError(f"{what}: iterations={iterations!r} (an integer, at least 0)")
    if iterations > 1 << 20:
        raise ValueError(f"{what}: iterations={iterations} (at most 2^20)")
    for name, x in (("lam", lam), ("mu", mu)):
        if x is None and name == "mu":
            continue
        if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)) or not math.isfinite(x):
            raise ValueError(f"{what}: {name}={x!r} (a finite number)")
    if boundary not in ("fixed", "free"):
        raise ValueError(f"{what}: boundary={boundary!r} ('fixed' or 'free')")


def smooth_mesh(verts, tris, iterations=10, lam=0.5, mu=-0.53, boundary="fixed", rings=None):
    """Laplacian / Taubin lambda|mu smoothing on the device: verts (V, 3) float32 and tris (T, 3) int64 on a 'cuda' device
    -> verts_s (V, 3) float32.  The triangles are unchanged and not returned.  lam = 0.5, mu = -0.53 are Taubin's values as
    trimesh and Open3D ship them.

    One iteration is a lam step followed by a mu step; ``mu=None`` is plain Laplacian smoothing, ``iterations`` lam steps;
    ``iterations=0`` returns a copy, byte for byte.  One step with factor f (the Python float rounded to float32): every
    vertex reads the positions of the PREVIOUS step (Jacobi with two buffers, never in place).  A vertex that moves, with
    ring j0 < j1 < ... < j(n-1) (vertex_rings), per component in float32, every operation rounded once: s = p[j0];
    s = s + p[jk] for k = 1 .. n-1 in that order; m = s / float(n); d = m - p_i; p_i' = p_i + f d (the product rounded,
    then the sum).  A vertex that does not move is copied byte for byte: an empty ring, and boundary[i] under
    ``boundary="fixed"``; ``boundary="free"`` moves boundary vertices like any other.  Positions that are not finite
    propagate by IEEE rules: nothing is checked and nothing is clamped.  The result is a pure function of the input,
    bit-identical from run to run (include/mocoflow_hip.h mf_smooth_mesh).

    ``rings``: a vertex_rings result for the same ``tris``, so that a caller smoothing several vertex sets over one topology
    builds it once; with it the call reads nothing from the device (``tris`` is then not looked at beyond its shape).
    Without it the call builds the rings itself, at the cost of vertex_rings' one read.  Rings that are no vertex_rings
    result give positions without meaning, never an access outside the buffers.  One host entry enqueues every step on the
    current stream; the two position buffers are allocated per call.

    ValueError before any tensor is looked at: ``iterations`` negative or not an integer, ``lam`` or ``mu`` not finite,
    ``boundary`` not one of the two strings, a ``rings`` tuple whose offsets length is not V + 1."""
    _smooth_args(iterations, lam, mu, boundary)
    if rings is not None:
        if len(rings) != 3:
            raise ValueError("smooth_mesh: rings is (offsets, ring, boundary) as vertex_rings returns them")
        n_off = rings[0].shape[0] if rings[0].dim() == 1 else -1
        n_v = verts.shape[0] if verts.dim() >= 1 else -1
        if n_off != n_v + 1:
            raise ValueError(f"smooth_mesh: rings offsets has shape {tuple(rings[0].shape)} for {n_v} vertices (V + 1 entries)")
    _check_tris(tris, "smooth_mesh")
    if verts.dim() != 2 or verts.shape[1] != 3:
        raise RuntimeError(f"smooth_mesh: verts must be (V, 3), got shape {tuple(verts.shape)}")
    if verts.dtype != torch.float32:
        raise RuntimeError(f"smooth_mesh: verts must be float32, got {verts.dtype}")
    V = verts.shape[0]
    for t in (tris, verts) + (tuple(rings) if rings is not None else ()):
        L.require_gpu(t, "smooth_mesh")
    verts = verts.detach().contiguous()
    if rings is None:
        offsets, ring, bnd = _rings(tris.detach().contiguous(), V, "smooth_mesh")
    else:
        offsets, ring, bnd = rings
        if offsets.dtype != torch.int64 or ring.dtype != torch.int64 or ring.dim() != 1:
            raise RuntimeError("smooth_mesh: rings offsets and ring must be 1-D int64")
        if bnd.dtype not in (torch.bool, torch.uint8) or bnd.shape != (V,):
            raise RuntimeError(f"smooth_mesh: rings boundary must be ({V},) bool")
        offsets, ring, bnd = offsets.contiguous(), ring.contiguous(), bnd.contiguous()
    if iterations == 0 or V == 0:
        return verts.clone()
    dev, R = verts.device, ring.shape[0]
    scratch = L.scratch(dev, "mf_smooth_mesh_scratch_bytes", V, R)
    out = torch.empty_like(verts)
    L.launch(dev, "mf_smooth_mesh", verts.data_ptr(), V, offsets.data_ptr(), L.ptr0(ring), R,
             bnd.data_ptr() if boundary == "fixed" else None, int(iterations), float(lam), 0.0 if mu is None else float(mu),
             0 if mu is None else 1, out.data_ptr(), scratch.data_ptr())
    return out


def _smooth_kwargs(smooth, what):
    """The keywords of smooth_mesh from the ``smooth=`` argument of the extraction calls: an int >= 1 or a dict."""
    if isinstance(smooth, dict):
        extra = set(smooth) - {"iterations", "lam", "mu", "boundary"}
        if extra:
            raise ValueError(f"{what}: smooth has unknown keys {sorted(extra)}")
        kw = dict(smooth)
    elif isinstance(smooth, (int, np.integer)) and not isinstance(smooth, bool) and smooth >= 1:
        kw = {"iterations": int(smooth)}
    else:
        raise ValueError(f"{what}: smooth={smooth!r} (None, an int >= 1, or a dict of smooth_mesh's keywords)")
    _smooth_args(kw.get("iterations", 10), kw.get("lam", 0.5), kw.get("mu", -0.53), kw.get("boundary", "fixed"), what)
    return kw


def lattice(N_grid, device):
    """visualize_mesh's query points (trainer_moco_flow.py:490-498): np.linspace(-1.5, 1.5, N) in float64 cast to fp32, laid
    out as np.stack(np.meshgrid(x, y, z), -1).reshape(-1, 3) ('xy' indexing: point (a, b, c) is (x[b], y[a], z[c]))."""
    ax = torch.from_numpy(np.linspace(-1.5, 1.5, N_grid).astype(np.float32)).to(device)
    N = N_grid
    return torch.stack([ax.view(1, N, 1).expand(N, N, N), ax.view(N, 1, 1).expand(N, N, N),
                        ax.view(1, 1, N).expand(N, N, N)], -1).reshape(-1, 3)


def _sparse_volume(N_grid, nerf, nerf_embedding_xyz, occupancy, margin, bw_nof, nof_embeddings, ind, precision):
    """``lattice``'s sigma volume through ``query_sigma_lattice``: the same coordinates, volume axis 0 carrying y and axis 1
    carrying x ('xy' indexing), 0 in the inactive bricks."""
    ax = np.linspace(-1.5, 1.5, N_grid).astype(np.float32)
    return query_sigma_lattice((ax, ax, ax), nerf, nerf_embedding_xyz, occupancy, world_of_axis=(1, 0, 2), margin=margin,
                               fill=0.0, bw_nof=bw_nof, nof_embeddings=nof_embeddings, ind=ind, precision=precision)


def extract_mesh(nerf, nerf_embedding_xyz, N_grid=256, sigma_threshold=10, bw_nof=None, nof_embeddings=None, ind=None,
                 precision=None, keep_largest=None, min_triangles=None, occupancy=None, margin=1, simplify=None, smooth=None):
    """visualize_mesh (trainer_moco_flow.py:490-538) up to the file: raw sigma of the NeRF on the N_grid^3 lattice over
    [-1.5, 1.5]^3 (query_sigma; with ``bw_nof`` / ``nof_embeddings`` / ``ind`` through the backward flow, ``ind`` =
    frame_idx * 2 / num_frames - 1), the isosurface of max(sigma, 0) at ``sigma_threshold``, then the reference's
    post-processing: vertex columns 0 and 1 swapped, triangle columns 1 and 2 swapped, vertices / N_grid * 3 - 1.5 (the
    reference divides by N_grid, not N_grid - 1).  Returns (verts (V, 3) float32, tris (T, 3) int64) on the NeRF's device;
    ``export_obj`` writes them.  ``keep_largest`` / ``min_triangles`` (not in the reference): filter_components with these
    on the raw isosurface, before the post-processing; both None leaves the path as it was.

    ``occupancy`` (an ``OccupancyGrid``, not in the reference; None leaves the path as it was): sigma is evaluated only in
    the lattice bricks the grid marks, ``margin`` lattice points around each (``_sparse_volume``, ``query_sigma_lattice``),
    and is 0 -- the empty side under the clamp -- everywhere else; no lattice tensor is built, and the call reads one more
    count from the device.  The mesh equals the dense one, bit for bit, exactly when every cell that crosses the threshold
    has its eight corners in active bricks.  A grid from a coarse pass can miss a thin part: that belongs to the grid's
    ``dilate`` and to a coarse threshold below ``sigma_threshold``, which nobody has validated on a trained checkpoint.

    ``simplify`` (not in the reference; None leaves the path as it was, byte for byte): the edge of a clustering cell in
    lattice steps, e.g. ``simplify=4``.  simplify_mesh runs on the raw isosurface in index coordinates, after the component
    filter and before the post-processing, with lo = 0 and hi = N_grid - 1 (known on the host: no extra read) and
    ``placement="mean"``.

    ``smooth`` (not in the reference; None leaves the path as it was, byte for byte): ``smooth=k``, an int >= 1, runs
    smooth_mesh(iterations=k) with its defaults (Taubin, lam = 0.5, mu = -0.53, boundary fixed);
    ``smooth=dict(iterations=..., lam=..., mu=..., boundary=...)`` passes those keywords.  It runs on the raw isosurface in
    index coordinates, AFTER the component filter and after ``simplify``, BEFORE the post-processing (the column swap and
    / N_grid * 3 - 1.5): the bits depend on that order.  The rim a lattice face cuts into the surface is a boundary and
    stays put under the default.  One more device -> host read (vertex_rings')."""
    if smooth is not None:
        smooth = _smooth_kwargs(smooth, "extract_mesh")
    dev = next(nerf.parameters()).device
    L.require_gpu(next(nerf.parameters()), "extract_mesh")
    with torch.no_grad():
        if occupancy is None:
            xyz = lattice(N_grid, dev)
            sigma = query_sigma(xyz, nerf, nerf_embedding_xyz, bw_nof, nof_embeddings, ind, precision=precision)
            del xyz
        else:
            sigma = _sparse_volume(N_grid, nerf, nerf_embedding_xyz, occupancy, margin, bw_nof, nof_embeddings, ind, precision)
        verts, tris = marching_cubes(sigma.view(N_grid, N_grid, N_grid), sigma_threshold, clamp_zero=True)
        if keep_largest is not None or min_triangles is not None:
            verts, tris = filter_components(verts, tris, keep_largest, min_triangles)
        if simplify is not None:
            verts, tris = simplify_mesh(verts, tris, simplify, lo=(0.0,) * 3, hi=(N_grid - 1.0,) * 3, placement="mean")
        if smooth is not None:
            verts = smooth_mesh(verts, tris, **smooth)
        verts = verts[:, [1, 0, 2]] / N_grid * 3.0 - 1.5
        tris = tris[:, [0, 2, 1]].contiguous()
    return verts, tris


def extract_colored_mesh(nerf, nerf_embeddings, N_grid=256, sigma_threshold=10, bw_nof=None, nof_embeddings=None, ind=None,
                         precision=None, keep_largest=None, min_triangles=None, occupancy=None, margin=2, simplify=None,
                         smooth=None):
    """extract_mesh with what a coloured mesh needs: (verts (V, 3), tris (T, 3), normals (V, 3), colors (V, 3)).

    verts / tris are extract_mesh's for the same arguments (``nerf_embeddings`` = [xyz, ind | None, dir | None] as
    render_rays takes it; ``precision`` applies to the sigma lattice only).  normals: vertex_normals of the kept sigma
    volume (max(sigma, 0)), in the axes of the returned vertices (columns [1, 0, 2] like them; the uniform scale leaves
    directions alone) -- they point out of the body.  colors: query_radiance(...)[:, :3] at the returned vertices in fp32,
    through the same NoF / ``ind``; a "dir" NeRF is looked at straight on, view_dirs = -normal ((0, 0, -1) where the
    normal is zero).  An empty mesh gives four empty tensors.  ``keep_largest`` / ``min_triangles``: as in extract_mesh;
    the filter runs before the radiance query, with the normals as a vertex attribute, so a dropped vertex is never
    queried.  ``occupancy`` / ``margin``: as in extract_mesh; the default margin is 2 because the normals' central
    differences read one lattice point beyond a crossing cell's corners -- normals equal the dense ones exactly when those
    neighbours lie in active bricks as well.

    ``simplify``: as in extract_mesh, positions by ``placement="mean"`` as well; it runs after the filter and before the
    radiance query, so colours are queried at the simplified vertices only (the query gets cheaper by the vertex ratio).
    The normal of a new vertex is the normal of ``first`` -- the row of its cell's smallest original vertex, carried as an
    attribute byte for byte: a unit vector (or zero) already, not re-normalised and not averaged.

    ``smooth``: as in extract_mesh, at the same place (after the filter and ``simplify``, before the post-processing).
    Normals and colours belong to the surface the field defines: vertex_normals is valid only for vertices on their lattice
    edges, so the normals are carried unchanged, and the colours are queried at the UNSMOOTHED post-processed positions;
    only the returned positions are smoothed.  Hence ``normals`` and ``colors`` equal those of the same call without
    ``smooth``, bit for bit, and ``verts`` / ``tris`` equal extract_mesh's with the same keywords."""
    if smooth is not None:
        smooth = _smooth_kwargs(smooth, "extract_colored_mesh")
    dev = next(nerf.parameters()).device
    L.require_gpu(next(nerf.parameters()), "extract_colored_mesh")
    with torch.no_grad():
        if occupancy is None:
            xyz = lattice(N_grid, dev)
            sigma = query_sigma(xyz, nerf, nerf_embeddings[0], bw_nof, nof_embeddings, ind, precision=precision)
            del xyz
        else:
            sigma = _sparse_volume(N_grid, nerf, nerf_embeddings[0], occupancy, margin, bw_nof, nof_embeddings, ind, precision)
        volume = sigma.view(N_grid, N_grid, N_grid)
        raw, tris = marching_cubes(volume, sigma_threshold, clamp_zero=True)
        normals = vertex_normals(volume, raw, clamp_zero=True)[:, [1, 0, 2]].contiguous()
        del sigma, volume
        if keep_largest is not None or min_triangles is not None:
            raw, tris, normals = filter_components(raw, tris, keep_largest, min_triangles, attrs=(normals,))
        if simplify is not None:
            raw, tris, normals = simplify_mesh(raw, tris, simplify, lo=(0.0,) * 3, hi=(N_grid - 1.0,) * 3, placement="mean",
                                               attrs=(normals,))
        verts = raw[:, [1, 0, 2]] / N_grid * 3.0 - 1.5
        smoothed = None if smooth is None else smooth_mesh(raw, tris, **smooth)[:, [1, 0, 2]] / N_grid * 3.0 - 1.5
        tris = tris[:, [0, 2, 1]].contiguous()
        if verts.shape[0] == 0:
            return verts, tris, normals, torch.empty((0, 3), dtype=torch.float32, device=dev)
        view_dirs = None
        if nerf.extra_feat_type == "dir":
            zero = (normals == 0).all(1, keepdim=True)
            view_dirs = torch.where(zero, normals.new_tensor([0.0, 0.0, -1.0]), -normals)
        colors = query_radiance(verts, nerf, nerf_embeddings, view_dirs=view_dirs, ind=ind, bw_nof=bw_nof,
                                nof_embeddings=nof_embeddings)[:, :3].contiguous()
    return (verts if smoothed is None else smoothed), tris, normals, colors


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


# ---- mesh-to-mesh distances (csrc/mf_mesh_distance.hip; include/mocoflow_hip.h "mesh-to-mesh distances") ----
_TILE = 64                               # slots per tile and rows per wave (csrc/mf_surface.hpp kSurfTile)
_MD_MODES = {"sweep": 0, "cull": 1}


def _morton(points, lo, hi):
    """30-bit Morton codes (int64) of (N, 3) points, 10 bits per axis over the box [lo, hi], clamped into it.  Plumbing: the
    codes order the slots and the queries and pick a wave's first tile; no result depends on them."""
    ext = (hi - lo).clamp_min(torch.finfo(torch.float32).tiny)
    c = ((points - lo) / ext * 1024.0).nan_to_num(0.0, 0.0, 0.0).clamp(0.0, 1023.0).to(torch.int64)

    def spread(x):
        x = (x | (x << 16)) & 0x030000FF
        x = (x | (x << 8)) & 0x0300F00F
        x = (x | (x << 4)) & 0x030C30C3
        return (x | (x << 2)) & 0x09249249
    return (spread(c[:, 0]) << 2) | (spread(c[:, 1]) << 1) | spread(c[:, 2])


class MeshIndex:
    """What closest_point, sample_surface and surface_distance need of a mesh, built once: verts (V, 3) float32 and tris (T, 3)
    int64 on a 'cuda' device.  ``order``: which triangle each slot of the search holds -- "morton" (triangle centroids quantised
    to 10 bits per axis over the mesh box, bits interleaved, a stable sort), "identity", or an int32 (T,) tensor.  The order is
    plumbing: no result depends on it (an entry outside [0, T) or a repeated one only drops triangles, and is counted).

    records (Tp, 16), edges (Tp, 12), slot_tri (Tp,), tile_box (Tp / 64, 8), tri_slot (T,), area2 (T,), normal (T, 3),
    dropped (T,) uint8, ``dropped_count`` (device int64 scalar), weights / cum (T,) int64: as include/mocoflow_hip.h defines them.
    A dropped triangle (an index outside [0, V), no area, a record field that is not finite) is never returned and never sampled.
    ``corners`` (Tp, 16): what cast_rays reads per slot -- the three vertices as read, the triangle's box, a zero -- built by
    mf_surface_corners on first use and kept.  Nothing is read back from the device."""
    _corners = None

    @property
    def corners(self):
        if self._corners is None:
            corners = torch.empty((self.n_tiles * _TILE, 16), dtype=torch.float32, device=self.device)
            L.launch(self.device, "mf_surface_corners", L.ptr0(self.verts), self.V, L.ptr0(self.tris), self.T, L.ptr0(self.slot_tri),
                     L.ptr0(corners))
            self._corners = corners
        return self._corners

    def __init__(self, verts, tris, order="morton"):
        _check_tris(tris, "MeshIndex")
        if verts.dim() != 2 or verts.shape[1] != 3 or verts.dtype != torch.float32:
            raise RuntimeError(f"MeshIndex: verts must be (V, 3) float32, got {tuple(verts.shape)} {verts.dtype}")
        L.require_gpu(verts, "MeshIndex")
        L.require_gpu(tris, "MeshIndex")
        dev = verts.device
        self.verts, self.tris = verts.detach().contiguous(), tris.detach().contiguous()
        V, T = self.verts.shape[0], self.tris.shape[0]
        Tp = (T + _TILE - 1) // _TILE * _TILE
        self.V, self.T, self.n_tiles, self.device = V, T, Tp // _TILE, dev
        if T and V:
            cen = self.verts[self.tris.clamp(0, V - 1)].mean(1).nan_to_num(0.0, 0.0, 0.0)
            self.lo, self.hi = cen.amin(0), cen.amax(0)
            codes = _morton(cen, self.lo, self.hi)
        else:
            self.lo, self.hi = torch.zeros(3, device=dev), torch.ones(3, device=dev)
            codes = torch.zeros(T, dtype=torch.int64, device=dev)
        if isinstance(order, str):
            if order not in ("morton", "identity"):
                raise ValueError(f"MeshIndex: order is 'morton', 'identity' or an int32 tensor, got {order!r}")
            self.order = torch.sort(codes, stable=True)[1].to(torch.int32) if order == "morton" and T else None
        else:
            L.require_gpu(order, "MeshIndex")
            if order.dtype != torch.int32 or order.shape != (T,):
                raise RuntimeError(f"MeshIndex: order must be int32 ({T},), got {order.dtype} {tuple(order.shape)}")
            self.order = order.contiguous()
        slot_codes = codes if self.order is None else codes[self.order.long().clamp(0, max(T - 1, 0))]
        self.tile_codes = slot_codes[::_TILE].contiguous()                   # ascending under "morton"
        f32 = dict(dtype=torch.float32, device=dev)
        self.records, self.edges = torch.empty((Tp, 16), **f32), torch.empty((Tp, 12), **f32)
        self.slot_tri = torch.empty(Tp, dtype=torch.int32, device=dev)
        self.tile_box = torch.empty((self.n_tiles, 8), **f32)
        self.tri_slot = torch.empty(T, dtype=torch.int32, device=dev)
        self.area2, self.normal = torch.empty(T, **f32), torch.empty((T, 3), **f32)
        self.dropped = torch.empty(T, dtype=torch.uint8, device=dev)
        self.dropped_count = torch.empty((), dtype=torch.int64, device=dev)
        self.weights = torch.empty(T, dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            L.enqueue(dev, "mf_surface_records", L.ptr0(self.verts), V, L.ptr0(self.tris), T, L.ptr0(self.order), L.ptr0(self.records),
                      L.ptr0(self.edges), L.ptr0(self.slot_tri), L.ptr0(self.tile_box), L.ptr0(self.tri_slot), L.ptr0(self.area2),
                      L.ptr0(self.normal), L.ptr0(self.dropped), self.dropped_count.data_ptr())
            if T:
                self.amax = self.area2.amax().reshape(1)
                L.enqueue(dev, "mf_surface_weights", self.area2.data_ptr(), self.dropped.data_ptr(), T, self.amax.data_ptr(),
                          self.weights.data_ptr())
        self.cum = torch.cumsum(self.weights, 0)                            # integers: exact in any order


def _as_index(mesh, what):
    if isinstance(mesh, MeshIndex):
        return mesh
    if isinstance(mesh, (tuple, list)) and len(mesh) == 2:
        return MeshIndex(mesh[0], mesh[1])
    raise RuntimeError(f"{what}: a mesh is a MeshIndex or a (verts, tris) pair")


def _schedule(index, anchors):
    """The schedule of a search: the rows in the Morton order of ``anchors`` (Q >= 1, 3), and per wave of 64 the tile whose code is
    nearest its first row's -> (qorder (Q,) int32, start (waves,) int32 or None without tiles).  No result depends on it."""
    codes, qorder = torch.sort(_morton(anchors, index.lo, index.hi), stable=True)
    first = codes[::_TILE].contiguous()                                      # the code of each wave's first row
    start = (torch.searchsorted(index.tile_codes, first, right=True) - 1).clamp(0, index.n_tiles - 1).to(torch.int32) if index.n_tiles else None
    return qorder.to(torch.int32), start


def closest_point(points, index, mode="cull", return_region=False, return_visited=False):
    """The closest point of a mesh to each of ``points`` (Q, 3) float32 on the index's device -> (d2 (Q,) float32, tri (Q,)
    int32 in the caller's numbering, point (Q, 3) float32[, region (Q,) uint8: 0 edge ab, 1 edge ac, 2 edge bc, 3 the face]
    [, visited (ceil(Q / 64),) int32: the 64-triangle tiles each wave of 64 queries evaluated]).

    Exact in the sense of include/mocoflow_hip.h: the lexicographic minimum of (value, triangle index) over the kept triangles,
    the value of a triangle being the least of four clamped candidates raised to the distance to its box, every operation
    rounded once.  ``mode="cull"`` skips tiles by their boxes, ``"sweep"`` evaluates every one; both give the same bits, as do
    every ``order`` of the index and every order of the queries.  The queries are visited in Morton order and each wave starts
    at the tile whose code is nearest its first query's.  No triangle kept: d2 = +inf, tri = -1, point = 0.  No host read."""
    if not isinstance(index, MeshIndex):
        raise RuntimeError("closest_point: index must be a MeshIndex")
    if mode not in _MD_MODES:
        raise ValueError(f"closest_point: mode is 'cull' or 'sweep', got {mode!r}")
    if points.dim() != 2 or points.shape[1] != 3 or points.dtype != torch.float32:
        raise RuntimeError(f"closest_point: points must be (Q, 3) float32, got {tuple(points.shape)} {points.dtype}")
    L.require_gpu(points, "closest_point")
    dev = index.device
    if points.device != dev:
        raise RuntimeError(f"closest_point: points on {points.device}, the index on {dev}")
    q = points.detach().contiguous()
    Q = q.shape[0]
    d2 = torch.empty(Q, dtype=torch.float32, device=dev)
    tri = torch.empty(Q, dtype=torch.int32, device=dev)
    point = torch.empty((Q, 3), dtype=torch.float32, device=dev)
    region = torch.empty(Q, dtype=torch.uint8, device=dev) if return_region else None
    visited = torch.empty((Q + _TILE - 1) // _TILE, dtype=torch.int32, device=dev) if return_visited else None
    if Q:
        qorder, start = _schedule(index, q)
        L.launch(dev, "mf_surface_closest", L.ptr0(index.records), L.ptr0(index.edges), L.ptr0(index.slot_tri), L.ptr0(index.tile_box),
                 index.T, q.data_ptr(), Q, qorder.data_ptr(), L.ptr0(start), _MD_MODES[mode], d2.data_ptr(),
                 tri.data_ptr(), point.data_ptr(), L.ptr0(region), L.ptr0(visited))
    out = (d2, tri, point)
    if return_region:
        out += (region,)
    if return_visited:
        out += (visited,)
    return out


def sample_surface(index, n, generator=None, draws=None):
    """``n`` points on the surface of the index's mesh, area-weighted: (points (n, 3) float32, tri (n,) int32).  A kept triangle
    has the integer weight max(1, floor(2^20 area / the largest area)), a dropped one 0; a draw r (int64 in [0, 2^53)) picks the
    first triangle whose running weight exceeds floor(r total / 2^53), and u (2 floats in [0, 1)) the point
    (a (1 - s) + b s (1 - u1)) + c s u1 with s = sqrt(u0).  ``draws=(r (n,), u (n, 2))`` injects them; otherwise torch draws them
    on the device (``generator``: a generator of that device).  No triangle kept: tri = -1, points = 0.  No host read."""
    if not isinstance(index, MeshIndex):
        raise RuntimeError("sample_surface: index must be a MeshIndex")
    n = int(n)
    if n < 0:
        raise ValueError(f"sample_surface: n={n}")
    dev = index.device
    if draws is None:
        r = torch.randint(0, 1 << 53, (n,), dtype=torch.int64, device=dev, generator=generator)
        u = torch.rand((n, 2), dtype=torch.float32, device=dev, generator=generator)
    else:
        r, u = draws
        L.require_gpu(r, "sample_surface")
        L.require_gpu(u, "sample_surface")
        if r.dtype != torch.int64 or r.shape != (n,) or u.dtype != torch.float32 or u.shape != (n, 2):
            raise RuntimeError(f"sample_surface: draws are (r int64 ({n},), u float32 ({n}, 2))")
        r, u = r.contiguous(), u.contiguous()
    points = torch.empty((n, 3), dtype=torch.float32, device=dev)
    tri = torch.empty(n, dtype=torch.int32, device=dev)
    if n:
        L.launch(dev, "mf_surface_sample", L.ptr0(index.verts), index.V, L.ptr0(index.tris), index.T, L.ptr0(index.cum), r.data_ptr(),
                 u.data_ptr(), n, points.data_ptr(), tri.data_ptr())
    return points, tri


def surface_stats(d2, thresholds=(), tri_src=None, tri_dst=None, normal_src=None, normal_dst=None):
    """The fused statistics of one direction: d2 (n,) float32 -> (f64 (4,) = [sum d, sum d^2, max d, sum |n_src . n_dst|],
    i64 (10,) = [rows with d <= thresholds[k] (k < 8), finite rows, rows left out]) on the device; d = sqrt(d2) in float32, sums
    in float64 in a fixed order (identical from run to run).  A row with a negative tri_src / tri_dst is left out and counted."""
    L.require_gpu(d2, "surface_stats")
    thresholds = tuple(float(t) for t in thresholds)
    if len(thresholds) > 8:
        raise ValueError(f"surface_stats: at most 8 thresholds, got {len(thresholds)}")
    dev, n = d2.device, d2.shape[0]
    d2 = d2.detach().contiguous()
    f64 = torch.empty(4, dtype=torch.float64, device=dev)
    i64 = torch.empty(10, dtype=torch.int64, device=dev)
    scratch = L.scratch(dev, "mf_surface_stats_scratch_bytes", n)
    tau = (C.c_float * 8)(*thresholds)
    L.launch(dev, "mf_surface_stats", L.ptr0(d2), n, L.ptr0(tri_src), L.ptr0(tri_dst), L.ptr0(normal_src),
             0 if normal_src is None else normal_src.shape[0], L.ptr0(normal_dst), 0 if normal_dst is None else normal_dst.shape[0],
             tau, len(thresholds), f64.data_ptr(), i64.data_ptr(), scratch.data_ptr())
    return f64, i64


def _direction(src, dst, n, thresholds, generator, draws):
    points, ts = sample_surface(src, n, generator, draws)
    d2, td, _ = closest_point(points, dst)
    f64, i64 = surface_stats(d2, thresholds, ts, td, src.normal, dst.normal)
    k = len(thresholds)
    finite = i64[8].to(torch.float64)
    return dict(mean=f64[0] / finite, rms=torch.sqrt(f64[1] / finite), max=f64[2], within=i64[:k], normal_consistency=f64[3] / finite,
                finite=i64[8], left_out=i64[9], d=torch.sqrt(d2), sums=f64)


def surface_distance(mesh_a, mesh_b, n=100_000, thresholds=(), generator=None, draws=None):
    """How far two surfaces are apart: ``n`` area-weighted samples of each mesh against the other.  A mesh is a MeshIndex or a
    (verts, tris) pair; ``draws=((r, u), (r, u))`` injects the samples of a and of b (sample_surface).  -> a dict of device
    tensors: ``a2b`` and ``b2a``, each a dict of mean, rms, max (of the distances of the finite rows), within[k] (rows with
    d <= thresholds[k], int64), normal_consistency (the mean |n_src . n_dst| of the two face normals), finite, left_out (int64),
    d (n,) the distances and sums (the raw float64 sums); ``chamfer`` = (mean_a2b + mean_b2a) / 2; ``fscore[k]`` = 2 P R / (P + R)
    with P = within_a2b[k] / finite_a2b and R = within_b2a[k] / finite_b2a (0 where P + R = 0).  Means of no finite row are NaN.
    No host read."""
    a, b = _as_index(mesh_a, "surface_distance"), _as_index(mesh_b, "surface_distance")
    if a.device != b.device:
        raise RuntimeError(f"surface_distance: meshes on {a.device} and {b.device}")
    thresholds = tuple(float(t) for t in thresholds)
    da, db = (None, None) if draws is None else draws
    ab = _direction(a, b, n, thresholds, generator, da)
    ba = _direction(b, a, n, thresholds, generator, db)
    P, R = ab["within"].to(torch.float64) / ab["finite"], ba["within"].to(torch.float64) / ba["finite"]
    fscore = torch.where(P + R > 0, 2 * P * R / (P + R), torch.zeros_like(P))
    return dict(a2b=ab, b2a=ba, chamfer=(ab["mean"] + ba["mean"]) / 2, fscore=fscore)


# ---- ray casts against a mesh (csrc/mf_mesh_rays.hip; include/mocoflow_hip.h "ray casts against a mesh") ----
_MR_MODES = {"first": 0, "any": 1}


def _ray_bounds(bound, Q, dev, what):
    if not isinstance(bound, torch.Tensor):
        return None
    L.require_gpu(bound, "cast_rays")
    if bound.device != dev or bound.dtype != torch.float32 or bound.shape not in ((), (Q,)):
        raise RuntimeError(f"cast_rays: {what} is a float or a float32 tensor () or ({Q},) on {dev}, got {bound.dtype} {tuple(bound.shape)}")
    return bound.detach().expand(Q).contiguous()


def cast_rays(index, origins=None, dirs=None, rays=None, t_min=0.0, t_max=math.inf, mode="first", cull=True, return_visited=False):
    """Rays against the index's mesh.  Either ``origins`` and ``dirs`` (Q, 3) float32 with ``t_min`` / ``t_max`` as floats or
    float32 (Q,) tensors, or ``rays`` (Q, >= 8) float32 rows in the package's layout (o, d, near, far: the bounds are the rows').
    A hit at parameter t lies at o + t d (d is not normalised by anyone).  ``mode="first"`` -> (t (Q,) float32, tri (Q,) int32
    in the caller's numbering, bary (Q, 3) float32: the weights of the triangle's three vertices); a miss is t = +inf, tri = -1,
    bary = 0.  ``mode="any"`` -> hit (Q,) uint8.  [, visited (ceil(Q / 64),) int32: the 64-triangle tiles each wave of 64 rays
    evaluated].  Both faces count.

    Exact in the sense of include/mocoflow_hip.h: a triangle is accepted by sign tests on edge functions of vertices sheared along
    the ray, every operation rounded once, so a ray through a shared edge or vertex of a closed mesh is never lost between two
    triangles; ``first`` is the lexicographic minimum of (t, triangle index) over the accepted kept triangles.  ``cull=True`` skips
    tiles by their boxes, ``False`` evaluates every one; both give the same bits, as do every ``order`` of the index and every
    order of the rays.  A ray with a component that is not finite, a zero direction or t_min > t_max hits nothing.  The rays are
    visited in the Morton order of the point each reaches at the distance of the mesh's centre, and a wave starts at the tile
    whose code is nearest its first ray's: plumbing that no result depends on.  No host read."""
    if not isinstance(index, MeshIndex):
        raise RuntimeError("cast_rays: index must be a MeshIndex")
    if mode not in _MR_MODES:
        raise ValueError(f"cast_rays: mode is 'first' or 'any', got {mode!r}")
    dev = index.device
    if rays is not None:
        if origins is not None or dirs is not None:
            raise ValueError("cast_rays: give origins and dirs, or rays, not both")
        if rays.dim() != 2 or rays.shape[1] < 8 or rays.dtype != torch.float32:
            raise RuntimeError(f"cast_rays: rays must be (Q, >= 8) float32, got {tuple(rays.shape)} {rays.dtype}")
        L.require_gpu(rays, "cast_rays")
        rays = rays.detach()
        if rays.shape[0] and (rays.stride(1) != 1 or rays.stride(0) < rays.shape[1]):
            rays = rays.contiguous()                                         # (a column slice or a row subset is read in place)
        Q, stride = rays.shape[0], rays.stride(0) if rays.shape[0] else 8
        o, d = rays[:, 0:3], rays[:, 3:6]
        o_ptr, bound_stride = rays.data_ptr(), stride
        d_ptr, lo_ptr, hi_ptr = o_ptr + 12, o_ptr + 24, o_ptr + 28
    else:
        if origins is None or dirs is None:
            raise ValueError("cast_rays: give origins and dirs, or rays")
        for name, x in (("origins", origins), ("dirs", dirs)):
            if x.dim() != 2 or x.shape[1] != 3 or x.dtype != torch.float32:
                raise RuntimeError(f"cast_rays: {name} must be (Q, 3) float32, got {tuple(x.shape)} {x.dtype}")
            L.require_gpu(x, "cast_rays")
        if origins.shape != dirs.shape:
            raise RuntimeError(f"cast_rays: origins {tuple(origins.shape)} and dirs {tuple(dirs.shape)}")
        o, d = origins.detach().contiguous(), dirs.detach().contiguous()
        Q, stride = o.shape[0], 3
        lo, hi = _ray_bounds(t_min, Q, dev, "t_min"), _ray_bounds(t_max, Q, dev, "t_max")
        if lo is None and hi is None:                                        # one pair of bounds for every ray
            held, bound_stride = torch.tensor([float(t_min), float(t_max)], dtype=torch.float32, device=dev), 0
            lo_ptr, hi_ptr = held.data_ptr(), held.data_ptr() + 4      # (held until the launch is enqueued)
        else:
            lo = torch.full((Q,), float(t_min), dtype=torch.float32, device=dev) if lo is None else lo
            hi = torch.full((Q,), float(t_max), dtype=torch.float32, device=dev) if hi is None else hi
            bound_stride, lo_ptr, hi_ptr = 1, lo.data_ptr(), hi.data_ptr()
        o_ptr, d_ptr = o.data_ptr(), d.data_ptr()
    if o.device != dev:
        raise RuntimeError(f"cast_rays: rays on {o.device}, the index on {dev}")
    first = mode == "first"
    t = torch.empty(Q, dtype=torch.float32, device=dev) if first else None
    tri = torch.empty(Q, dtype=torch.int32, device=dev) if first else None
    bary = torch.empty((Q, 3), dtype=torch.float32, device=dev) if first else None
    hit = None if first else torch.empty(Q, dtype=torch.uint8, device=dev)
    visited = torch.empty((Q + _TILE - 1) // _TILE, dtype=torch.int32, device=dev) if return_visited else None
    if Q:
        centre = (index.lo + index.hi) * 0.5
        reach = (centre - o).norm(dim=1, keepdim=True) / d.norm(dim=1, keepdim=True)
        qorder, start = _schedule(index, o + d * reach)
        L.launch(dev, "mf_surface_cast", L.ptr0(index.corners), L.ptr0(index.slot_tri), L.ptr0(index.tile_box), index.T, o_ptr, d_ptr, stride,
                 lo_ptr, hi_ptr, bound_stride, Q, qorder.data_ptr(), L.ptr0(start), _MR_MODES[mode], 1 if cull else 0, L.ptr0(t), L.ptr0(tri),
                 L.ptr0(bary), L.ptr0(hit), L.ptr0(visited))
    out = (t, tri, bary) if first else (hit,)
    if return_visited:
        out += (visited,)
    return out if len(out) > 1 else out[0]


def visible_from(index, points, eye, bias):
    """Which of ``points`` (Q, 3) float32 the point ``eye`` sees past the index's mesh -> (Q,) uint8, 1 where the segment from
    points[i] to eye is free.  ``eye``: (3,) or (Q, 3) float32 on the index's device.  An any-hit cast_rays with o = points,
    d = eye - points and t in [bias, 1].  ``bias``: a float in units of the segment, chosen by the caller: it excludes the surface
    the point itself sits on (a vertex or a surface sample of this mesh is hit at t = 0, give or take rounding); too large a
    bias also excludes an occluder that close to the point.  A point that is not finite, or that is the eye, counts as seen."""
    if points.dim() != 2 or points.shape[1] != 3 or points.dtype != torch.float32:
        raise RuntimeError(f"visible_from: points must be (Q, 3) float32, got {tuple(points.shape)} {points.dtype}")
    if not isinstance(eye, torch.Tensor) or eye.dtype != torch.float32 or eye.shape not in ((3,), tuple(points.shape)):
        raise RuntimeError(f"visible_from: eye must be a float32 tensor (3,) or {tuple(points.shape)}")
    L.require_gpu(points, "visible_from")
    L.require_gpu(eye, "visible_from")
    points = points.detach()
    return cast_rays(index, points, (eye.detach() - points).contiguous(), t_min=float(bias), t_max=1.0, mode="any") ^ 1
