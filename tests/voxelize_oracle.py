"""The contracts of mf_voxel_mesh, mf_voxel_fill and mf_voxel_dilate (include/mocoflow_hip.h; OccupancyGrid.from_mesh, .filled,
.dilated) restated in numpy and Python ints.  No GPU, no package code.

Snapping is numpy fp32 with the kernel's three roundings (subtract, multiply, multiply by 64), then rint and saturation.  The
surface predicate -- the closed snapped triangle meets the closed cell -- is decided by the 13-axis separating-axis test on int64
(the kernel uses Schwarz and Seidel's formulation: bounding box, plane against the critical corners, three projected edge
tests).  The fill is a flood from the border, the dilation shifted ORs."""
import numpy as np

f32 = np.float32
SUB = 64                                  # sub-cell units per cell
SNAP_LO, SNAP_HI = -(1 << 16), 1 << 17    # saturation of a snapped coordinate
MAX_SIDE = 1024


def grid_constants(dims, lo, hi):
    """(lo, hi, inv_cell) as fp32, the way OccupancyGrid computes them: the cell edge in float64 from the fp32 box."""
    lo32, hi32 = np.asarray(lo, dtype=np.float32), np.asarray(hi, dtype=np.float32)
    edge = (hi32.astype(np.float64) - lo32.astype(np.float64)) / np.asarray(dims, dtype=np.float64)
    return lo32, hi32, (1.0 / edge).astype(np.float32)


def snap(verts, lo, inv_cell):
    """(V, 3) fp32 -> (q int64 (V, 3), finite bool (V,)); q of a non-finite vertex is meaningless."""
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    lo, inv = np.asarray(lo, dtype=np.float32), np.asarray(inv_cell, dtype=np.float32)
    finite = np.isfinite(v).all(1)
    with np.errstate(all="ignore"):
        s = ((np.where(finite[:, None], v, f32(0)) - lo) * inv) * f32(SUB)       # every operation rounded to fp32
        s = np.clip(s, f32(SNAP_LO), f32(SNAP_HI))
    assert s.dtype == np.float32
    return np.rint(s).astype(np.int64), finite


def cell_of(points, lo, inv_cell, dims):
    """mf_ray_clip's cell rule: clamp(floor((p - lo) * inv_cell), 0, g - 1) in fp32."""
    p = np.asarray(points, dtype=np.float32)
    fl = np.floor((p - np.asarray(lo, f32)) * np.asarray(inv_cell, f32))
    return np.clip(fl, 0, np.asarray(dims, f32) - 1).astype(np.int64)


def _normal(q):
    e0, e1 = q[:, 1] - q[:, 0], q[:, 2] - q[:, 1]
    return np.cross(e0, e1)                                  # int64: components below 2^37


def sat_meets(q, cells):
    """q (P, 3, 3) int64 snapped corners, cells (P, 3) int64 -> bool (P,): the closed triangle meets the closed box
    [64 c, 64 c + 64]^3, by the 13-axis separating-axis test.  A zero axis separates nothing."""
    q = np.asarray(q, dtype=np.int64)
    box = np.asarray(cells, dtype=np.int64) * SUB
    eye = np.eye(3, dtype=np.int64)
    axes = [np.broadcast_to(eye[a], box.shape) for a in range(3)]
    axes.append(_normal(q))
    for i in range(3):
        e = q[:, (i + 1) % 3] - q[:, i]
        for a in range(3):
            axes.append(np.cross(e, np.broadcast_to(eye[a], e.shape)))
    ok = np.ones(len(q), dtype=bool)
    for ax in axes:
        t = (q * ax[:, None, :]).sum(-1)                     # (P, 3) projections of the corners
        b0 = (box * ax).sum(-1)
        bmin = b0 + np.minimum(ax * SUB, 0).sum(-1)
        bmax = b0 + np.maximum(ax * SUB, 0).sum(-1)
        ok &= (t.min(1) <= bmax) & (bmin <= t.max(1))
    return ok


def surface(verts, tris, dims, lo, hi, chunk=1 << 21):
    """(dense bool (gx, gy, gz), dropped) of mf_voxel_mesh."""
    dims = tuple(int(g) for g in dims)
    assert all(1 <= g <= MAX_SIDE for g in dims)
    lo32, hi32, inv = grid_constants(dims, lo, hi)
    verts = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    tris = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    V = len(verts)
    dense = np.zeros(dims, dtype=bool)
    valid = ((tris >= 0) & (tris < V)).all(1)
    if V == 0 or len(tris) == 0:
        return dense, (len(tris) if V == 0 else 0)           # without vertices every index is outside [0, V)
    qv, finite = snap(verts, lo32, inv)
    safe = np.where(valid[:, None], tris, 0)
    valid &= finite[safe].all(1)
    q = qv[safe]                                             # (T, 3, 3)
    valid &= (_normal(q) != 0).any(1)
    dropped = int((~valid).sum())
    q = q[valid]
    g = np.asarray(dims, dtype=np.int64)
    first = np.maximum(-((-q.min(1)) // SUB) - 1, 0)         # ceil(min / 64) - 1
    last = np.minimum(q.max(1) // SUB, g - 1)
    keep = (last >= first).all(1)
    q, first, last = q[keep], first[keep], last[keep]
    nc = last - first + 1
    counts = nc.prod(1)
    start = 0
    while start < len(q):
        stop, total = start, 0
        while stop < len(q) and (stop == start or total + counts[stop] <= chunk):
            total += counts[stop]
            stop += 1
        cnt = counts[start:stop]
        tri_of = np.repeat(np.arange(start, stop), cnt)
        off = np.arange(total) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        nz, ny = nc[tri_of, 2], nc[tri_of, 1]
        r = off // nz
        cells = first[tri_of] + np.stack([r // ny, r % ny, off - r * nz], 1)
        hit = sat_meets(q[tri_of], cells)
        c = cells[hit]
        dense[c[:, 0], c[:, 1], c[:, 2]] = True
        start = stop
    return dense, dropped


def fill(dense):
    """dense plus the empty cells that are not 6-connected through empty cells to the outside of the grid: a flood from the
    border, one layer of neighbours per sweep."""
    dense = np.asarray(dense, dtype=bool)
    empty = ~dense
    outside = np.zeros_like(dense)
    for a in range(3):
        idx = [slice(None)] * 3
        for side in (0, -1):
            idx[a] = side
            outside[tuple(idx)] = empty[tuple(idx)]
    while True:
        grown = outside.copy()
        for a in range(3):
            up, dn = [slice(None)] * 3, [slice(None)] * 3
            up[a], dn[a] = slice(1, None), slice(None, -1)
            grown[tuple(up)] |= outside[tuple(dn)]
            grown[tuple(dn)] |= outside[tuple(up)]
        grown &= empty
        if (grown == outside).all():
            return dense | (empty & ~outside)
        outside = grown


def dilate(dense, radii):
    """Box dilation by (rx, ry, rz) cells, clipped to the grid: shifted ORs, axis by axis."""
    out = np.asarray(dense, dtype=bool).copy()
    for a, r in enumerate(radii):
        assert r >= 0
        src = out.copy()
        for s in range(1, min(int(r), src.shape[a] - 1) + 1):
            up, dn = [slice(None)] * 3, [slice(None)] * 3
            up[a], dn[a] = slice(s, None), slice(None, -s)
            out[tuple(up)] |= src[tuple(dn)]
            out[tuple(dn)] |= src[tuple(up)]
    return out


def pack(dense):
    """bool (gx, gy, gz) -> uint32 (gx, gy, ceil(gz / 32)): cell k is bit k % 32 of word k / 32, padding bits zero."""
    gx, gy, gz = dense.shape
    wz = (gz + 31) // 32
    padded = np.zeros((gx, gy, wz * 32), dtype=np.uint64)
    padded[:, :, :gz] = dense
    return (padded.reshape(gx, gy, wz, 32) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)


def unpack(bits, gz):
    gx, gy, wz = bits.shape
    b = (np.asarray(bits).view(np.uint32)[..., None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)
    return b.reshape(gx, gy, wz * 32)[:, :, :gz].astype(bool)


def radii(dims, lo, hi, dilate_cells, thickness):
    """from_mesh's rule: r_a = dilate_a + ceil(thickness / cell_a), float64, the cell edge from the fp32 box."""
    lo32, hi32 = np.asarray(lo, dtype=np.float32), np.asarray(hi, dtype=np.float32)
    cell = (hi32.astype(np.float64) - lo32.astype(np.float64)) / np.asarray(dims, dtype=np.float64)
    d = (dilate_cells,) * 3 if np.isscalar(dilate_cells) else tuple(dilate_cells)
    return tuple(int(d[a]) + int(np.ceil(float(thickness) / cell[a])) for a in range(3))


def from_mesh(verts, tris, dims, lo, hi, dilate_cells=1, thickness=0.0, solid=True):
    """(dense, dropped) of OccupancyGrid.from_mesh."""
    dense, dropped = surface(verts, tris, dims, lo, hi)
    if solid:
        dense = fill(dense)
    return dilate(dense, radii(dims, lo, hi, dilate_cells, thickness)), dropped


# ---- the kernel's formulation in Python ints: for the overflow bound and as a second statement of the predicate -----------------

def schwarz_seidel(q, cell, terms=None):
    """The predicate as csrc/mf_voxelize.hip forms it (vox_setup, vox_hit), in Python ints: q three corners of three ints, cell
    three ints.  ``terms``: a list that receives every intermediate the kernel holds in an int64.  None: a zero normal."""
    q = [[int(x) for x in c] for c in q]
    T = terms if terms is not None else []
    e = [[q[(i + 1) % 3][a] - q[i][a] for a in range(3)] for i in range(3)]
    n = [e[0][(a + 1) % 3] * e[1][(a + 2) % 3] - e[0][(a + 2) % 3] * e[1][(a + 1) % 3] for a in range(3)]
    T += [x for row in e for x in row] + n
    T += [e[0][(a + 1) % 3] * e[1][(a + 2) % 3] for a in range(3)] + [e[0][(a + 2) % 3] * e[1][(a + 1) % 3] for a in range(3)]
    if n == [0, 0, 0]:
        return None
    pc = [int(c) * SUB for c in cell]
    for a in range(3):
        mn, mx = min(c[a] for c in q), max(c[a] for c in q)
        if pc[a] > mx or pc[a] + SUB < mn:
            return False
    nv0, up, down = 0, 0, 0
    for a in range(3):
        nv0 += n[a] * q[0][a]
        up += n[a] * SUB if n[a] > 0 else 0
        down += n[a] * SUB if n[a] < 0 else 0
        T += [n[a] * q[0][a], nv0, up, down]
    d_lo, d_hi = down - nv0, up - nv0
    t = 0
    for a in range(3):
        t += n[a] * pc[a]
        T += [n[a] * pc[a], t]
    T += [d_lo, d_hi, t + d_lo, t + d_hi]
    hit = t + d_lo <= 0 <= t + d_hi
    for a in range(3):
        u, v = (a + 1) % 3, (a + 2) % 3
        sgn = 1 if n[a] >= 0 else -1
        for i in range(3):
            mu, mv = -e[i][v] * sgn, e[i][u] * sgn
            c = -(mu * q[i][u] + mv * q[i][v]) + SUB * (max(mu, 0) + max(mv, 0))
            f = mu * pc[u] + mv * pc[v] + c
            T += [mu * q[i][u], mv * q[i][v], c, mu * pc[u], mv * pc[v], f]
            hit = hit and f >= 0
    return hit


# ---- meshes ----------------------------------------------------------------------------------------------------------------------

def icosphere(subdivisions, center=(0.0, 0.0, 0.0), radius=1.0):
    """(verts fp32 (V, 3), tris int64 (T, 3)): 20 * 4^subdivisions triangles, closed, outward-facing."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def midpoint(a, b):
            key = (a, b) if a < b else (b, a)
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    verts = np.asarray(v) * radius + np.asarray(center, dtype=np.float64)
    return verts.astype(np.float32), np.asarray(f, dtype=np.int64)


def torus(major, minor, nu=24, nv=12, center=(0.0, 0.0, 0.0)):
    """A closed torus around the z axis through ``center``: nu x nv quads, two triangles each."""
    u = np.arange(nu) * (2 * np.pi / nu)
    w = np.arange(nv) * (2 * np.pi / nv)
    uu, ww = np.meshgrid(u, w, indexing="ij")
    ring = major + minor * np.cos(ww)
    verts = np.stack([ring * np.cos(uu), ring * np.sin(uu), minor * np.sin(ww)], -1).reshape(-1, 3) + np.asarray(center)
    tris = []
    for i in range(nu):
        for j in range(nv):
            a, b = i * nv + j, ((i + 1) % nu) * nv + j
            c, d = i * nv + (j + 1) % nv, ((i + 1) % nu) * nv + (j + 1) % nv
            tris += [(a, b, d), (a, d, c)]
    return verts.astype(np.float32), np.asarray(tris, dtype=np.int64)


def merge(*meshes):
    """One mesh of several: indices shifted."""
    verts, tris, base = [], [], 0
    for v, t in meshes:
        verts.append(v)
        tris.append(t + base)
        base += len(v)
    return np.concatenate(verts).astype(np.float32), np.concatenate(tris).astype(np.int64)


def nested_spheres(subdivisions, center, outer, inner):
    return merge(icosphere(subdivisions, center, outer), icosphere(subdivisions, center, inner))


def hemisphere(subdivisions, center=(0.0, 0.0, 0.0), radius=1.0):
    """The open upper half of an icosphere: the triangles whose centroid lies above the centre, the rim left open."""
    v, t = icosphere(subdivisions, center, radius)
    return v, t[v[t].mean(1)[:, 2] > center[2]]


def grid_point(ijk, lo, hi, dims):
    """World coordinates (float64) of grid coordinates ijk (cells, fractional): lo + ijk * cell."""
    lo32, hi32 = np.asarray(lo, dtype=np.float32).astype(np.float64), np.asarray(hi, dtype=np.float32).astype(np.float64)
    return lo32 + np.asarray(ijk, dtype=np.float64) * (hi32 - lo32) / np.asarray(dims, dtype=np.float64)
