"""The numpy restatement of csrc/mf_mesh_rays.hip's contract (include/mocoflow_hip.h, "ray casts against a mesh"): every operation
in np.float32, rounded once, in the header's order, with max / min that ignore a NaN (np.fmax / np.fmin, as fmaxf / fminf do).
Brute force, vectorised over triangles and chunked over rays: the ray set-up, the sheared vertices (sheared once per VERTEX, so
that two triangles sharing one see the same three numbers -- the kernel recomputes them per corner from the same operands), the
edge functions, the clamped t, the four acceptance conditions, the (t, index) minimum and the winner's barycentrics; the corner
rows of mf_surface_corners; the tile predicate of the culled search, and that search as a wave performs it.  Beside it a plain Moeller-Trumbore, in float64 as the
judge and in float32 as the thing the contract replaces, the blob mesh and the ray families of the watertightness tests.  The
index (slots, tiles, the drop rule) is mesh_distance_oracle.records' -- the cast reads the same one.  As there, the only float
comparison that is not bit for bit is the sign of a zero, so callers compare with == (np.array_equal)."""
import numpy as np

import mesh_distance_oracle as D

F = np.float32
TILE = D.TILE
records = D.records


# ---------------------------------------------------------------- meshes and rays ---------------------------------------------
def icosphere(subdivisions):
    """Unit icosphere in float64: 20 * 4^s triangles, outward orientation."""
    g = (1 + 5 ** 0.5) / 2
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    t = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdivisions):
        mid, out = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in t:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        t = out
    return np.array(v), np.array(t, dtype=np.int64)


BLOB_CENTER = np.array([0.1, -0.2, 0.05])
BLOB_SCALE = np.array([1.0, 0.7, 1.3])


def blob(subdivisions=3, seed=7):
    """A closed star-shaped surface: an icosphere whose radius is perturbed (smoothly and per vertex), scaled by BLOB_SCALE about
    BLOB_CENTER.  1 280 triangles (20 tiles) and 642 vertices at 3 subdivisions.  -> verts float32, tris int64."""
    v, t = icosphere(subdivisions)
    rng = np.random.default_rng(seed)
    r = 1 + 0.15 * np.sin(3 * v[:, 0] + 1) * np.cos(2 * v[:, 1]) + 0.1 * np.sin(5 * v[:, 2]) + 0.03 * rng.uniform(-1, 1, len(v))
    return (v * r[:, None] * BLOB_SCALE + BLOB_CENTER).astype(F), t


def blob_interior():
    """A point inside every blob(), off its centre."""
    return (BLOB_CENTER + np.array([0.05, 0.03, -0.04])).astype(F)


def mesh_edges(tris):
    e = np.sort(np.concatenate([tris[:, [0, 1]], tris[:, [1, 2]], tris[:, [2, 0]]]), axis=1)
    return np.unique(e, axis=0)


AXES = np.array([d for d in np.ndindex(3, 3, 3) if 1 <= np.abs(np.array(d) - 1).sum() <= 2], dtype=F) - F(1)      # 6 axes, 12 diagonals


def ray_families(verts, tris, origin, n_random=3000, seed=11):
    """The directions, from `origin`, of the watertightness tests as a dict of float32 (n, 3) arrays: through every vertex,
    through three points of every edge, through every centroid, `n_random` random directions, the 18 axis and face-diagonal
    directions.  A direction is target - origin in float32: the q of that vertex in the kernel."""
    o = np.asarray(origin, dtype=F)
    e = mesh_edges(tris)
    a, b = verts[e[:, 0]], verts[e[:, 1]]
    on_edges = np.concatenate([a + (b - a) * F(f) for f in (0.25, 0.5, 0.75)])
    centroids = (verts[tris[:, 0]] + verts[tris[:, 1]] + verts[tris[:, 2]]) * F(1 / 3)
    rnd = np.random.default_rng(seed).normal(size=(n_random, 3))
    rnd = (rnd / np.linalg.norm(rnd, axis=1, keepdims=True)).astype(F)
    return dict(vertices=verts - o, edges=(on_edges - o).astype(F), centroids=(centroids - o).astype(F), random=rnd, axes=AXES.copy())


# ---------------------------------------------------------------- the contract ------------------------------------------------
def corners(R):
    """mf_surface_corners: per slot a, b, c as read, the triangle's box lo, hi, a zero; zeros for a slot without a triangle."""
    s = np.flatnonzero(R["slot_tri"] >= 0)
    v = R["verts"][R["tris"][R["slot_tri"][s]]]                             # (n, 3, 3)
    out = np.zeros((len(R["slot_tri"]), 16), F)
    out[s, 0:9] = v.reshape(-1, 9)
    out[s, 9:12] = np.fmin(np.fmin(v[:, 0], v[:, 1]), v[:, 2])
    out[s, 12:15] = np.fmax(np.fmax(v[:, 0], v[:, 1]), v[:, 2])
    return out


def bounds(Q, t_min, t_max):
    return np.broadcast_to(np.asarray(t_min, dtype=F), (Q,)).copy(), np.broadcast_to(np.asarray(t_max, dtype=F), (Q,)).copy()


def setup(o, d, t_min=0.0, t_max=np.inf):
    """Per ray: dead, the axes kx, ky, kz, the shear Sx, Sy, Sz, and o, t_min, t_max -- a dict of (Q, ...) arrays."""
    o, d = np.ascontiguousarray(o, dtype=F).reshape(-1, 3), np.ascontiguousarray(d, dtype=F).reshape(-1, 3)
    Q = len(o)
    t_min, t_max = bounds(Q, t_min, t_max)
    with np.errstate(all="ignore"):
        dead = ~np.isfinite(o).all(1) | ~np.isfinite(d).all(1) | (d == 0).all(1) | ~(t_min <= t_max)
        kz = np.where(dead, 0, np.argmax(np.abs(np.nan_to_num(d, nan=0.0, posinf=0.0, neginf=0.0)), axis=1))      # the first of the largest
        kx = (kz + 1) % 3
        ky = (kx + 1) % 3
        rows = np.arange(Q)
        swap = d[rows, kz] < 0
        kx, ky = np.where(swap, ky, kx), np.where(swap, kx, ky)
        dz = d[rows, kz]
        S = np.stack([d[rows, kx] / dz, d[rows, ky] / dz, F(1) / dz], -1).astype(F)
    return dict(dead=dead, k=np.stack([kx, ky, kz], -1), S=S, o=o, t_min=t_min, t_max=t_max, Q=Q)


def _rows(ray, i):
    return {k: (v[i] if isinstance(v, np.ndarray) else v) for k, v in ray.items()}


def shear(p, ray):
    """p (N, 3) points against Q rays -> (Q, N, 3): x = q[kx] - Sx q[kz], y = q[ky] - Sy q[kz], z = Sz q[kz], q = p - o."""
    with np.errstate(all="ignore"):
        q = p[None, :, :] - ray["o"][:, None, :]
        q = np.take_along_axis(q, np.broadcast_to(ray["k"][:, None, :], q.shape), axis=2)       # (q[kx], q[ky], q[kz])
        S = ray["S"][:, None, :]
        return np.stack([q[..., 0] - S[..., 0] * q[..., 2], q[..., 1] - S[..., 1] * q[..., 2], S[..., 2] * q[..., 2]], -1)


def tri_terms(A, B, C, t_min, t_max):
    """Sheared corners (..., 3) -> U, V, W, det, t, accepted."""
    ty = A.dtype.type
    with np.errstate(all="ignore"):
        U = C[..., 0] * B[..., 1] - C[..., 1] * B[..., 0]
        V = A[..., 0] * C[..., 1] - A[..., 1] * C[..., 0]
        W = B[..., 0] * A[..., 1] - B[..., 1] * A[..., 0]
        det = (U + V) + W
        t_raw = ((U * A[..., 2] + V * B[..., 2]) + W * C[..., 2]) * (ty(1) / det)
        zmin = np.fmin(np.fmin(A[..., 2], B[..., 2]), C[..., 2])
        zmax = np.fmax(np.fmax(A[..., 2], B[..., 2]), C[..., 2])
        t = np.fmin(np.fmax(t_raw, zmin), zmax)
        sign = ((U >= 0) & (V >= 0) & (W >= 0)) | ((U <= 0) & (V <= 0) & (W <= 0))
        own = np.ones(U.shape, bool)
        for k in (0, 1):
            own &= (np.fmin(np.fmin(A[..., k], B[..., k]), C[..., k]) <= 0) & (0 <= np.fmax(np.fmax(A[..., k], B[..., k]), C[..., k]))
        acc = sign & (det != 0) & own & (t_min <= t) & (t <= t_max)
    return U, V, W, det, t, acc


def evaluate(R, ray):
    """Every ray of `ray` against every kept triangle, in ascending caller's index -> (kept, U, V, W, det, t, accepted (Q, n))."""
    kept = np.flatnonzero(R["dropped"] == 0)
    tris = R["tris"][kept]
    used = np.unique(tris)                                                  # shear each vertex once
    P = shear(R["verts"][used], ray)
    i = np.searchsorted(used, tris)
    U, V, W, det, t, acc = tri_terms(P[:, i[:, 0]], P[:, i[:, 1]], P[:, i[:, 2]], ray["t_min"][:, None], ray["t_max"][:, None])
    return kept, U, V, W, det, t, acc & ~ray["dead"][:, None]


def cast(R, o, d, t_min=0.0, t_max=np.inf, pairs=1 << 20):
    """mf_surface_cast by brute force -> t (Q) float32, tri (Q) int32, bary (Q, 3) float32, hit (Q) uint8."""
    ray = setup(o, d, t_min, t_max)
    Q = ray["Q"]
    t_out, tri, bary, hit = np.full(Q, np.inf, F), np.full(Q, -1, np.int32), np.zeros((Q, 3), F), np.zeros(Q, np.uint8)
    n = int((R["dropped"] == 0).sum())
    if not n or not Q:
        return t_out, tri, bary, hit
    step = max(1, pairs // n)
    for i in range(0, Q, step):
        sl = slice(i, i + step)
        kept, U, V, W, det, t, acc = evaluate(R, _rows(ray, sl))
        any_ = acc.any(1)
        best = np.where(acc, t, F(np.inf)).min(1)
        j = (acc & (t == best[:, None])).argmax(1)                          # the lowest index among the accepted at the least t
        rows = np.arange(len(j))
        with np.errstate(all="ignore"):
            rdet = F(1) / det[rows, j]
            b = np.stack([U[rows, j] * rdet, V[rows, j] * rdet, W[rows, j] * rdet], -1)
        t_out[sl] = np.where(any_, best, F(np.inf))
        tri[sl] = np.where(any_, kept[j], -1)
        bary[sl] = np.where(any_[:, None], b, F(0))
        hit[sl] = any_
    return t_out, tri, bary, hit


def visible(R, points, eye, bias):
    """visible_from: 1 where no kept triangle is accepted on the segment points -> eye with t in [bias, 1]."""
    points = np.asarray(points, dtype=F).reshape(-1, 3)
    d = (np.broadcast_to(np.asarray(eye, dtype=F), points.shape) - points).astype(F)
    return (1 - cast(R, points, d, bias, 1.0)[3]).astype(np.uint8)


def tile_intervals(R, ray):
    """The sheared intervals of every tile box for every ray -> x0, x1, y0, y1, z0, z1, each (Q, n_tiles)."""
    box = R["tile_box"]
    with np.errstate(all="ignore"):
        pick = lambda p: np.take_along_axis(p[None, :, :] - ray["o"][:, None, :], np.broadcast_to(ray["k"][:, None, :], (ray["Q"], len(p), 3)), axis=2)
        l, h = pick(box[:, 0:3]), pick(box[:, 3:6])
        S = ray["S"][:, None, :]
        out = []
        for a in (0, 1):
            sl, sh = S[..., a] * l[..., 2], S[..., a] * h[..., 2]
            out += [l[..., a] - np.fmax(sl, sh), h[..., a] - np.fmin(sl, sh)]
        zl, zh = S[..., 2] * l[..., 2], S[..., 2] * h[..., 2]
        return out + [np.fmin(zl, zh), np.fmax(zl, zh)]


def tile_wanted(R, ray, best=np.inf):
    """The tile predicate per (ray, tile): a live ray wants a tile that holds a kept slot, has 0 inside its x and y intervals and
    a z interval that meets [t_min, min(t_max, best)]."""
    x0, x1, y0, y1, z0, z1 = tile_intervals(R, ray)
    best = np.broadcast_to(np.asarray(best, dtype=F), (ray["Q"],))[:, None]
    with np.errstate(all="ignore"):
        geo = (x0 <= 0) & (0 <= x1) & (y0 <= 0) & (0 <= y1) & ~(z1 < ray["t_min"][:, None]) & ~(z0 > ray["t_max"][:, None]) & (z0 <= best)
    return geo & (R["tile_box"][None, :, 6] != 0) & ~ray["dead"][:, None]


def cast_culled(R, o, d, t_min, t_max, mode, qorder=None, start=None, cull=True):
    """The cast as a wave performs it: 64 rays in the visiting order, the tiles of mesh_distance_oracle.tile_walk, one decision
    per tile.  A lane is done if its ray is dead or, in mode 1 (any), has found a hit; under `cull` the wave stops once every
    lane is done and skips a tile that holds no kept slot or that no lane still at work wants at its current best.  A tile that
    is not skipped is evaluated slot by slot, as the lanes do.  -> t, tri, bary (mode 0; else None), hit (mode 1; else None) and
    the number of tiles each wave evaluated."""
    ray = setup(o, d, t_min, t_max)
    Q, n = ray["Q"], len(R["tile_box"])
    qorder = np.arange(Q) if qorder is None else np.asarray(qorder)
    t_out, tri, bary, hit = np.full(Q, np.inf, F), np.full(Q, -1, np.int32), np.zeros((Q, 3), F), np.zeros(Q, np.uint8)
    rows_of, slot_tri = corners(R).reshape(n, TILE, 16), R["slot_tri"].reshape(n, TILE)
    visited = []
    for w in range(-(-Q // TILE)):
        rows = qorder[w * TILE:(w + 1) * TILE]
        r = dict(_rows(ray, rows), Q=len(rows))
        best, btri, found = np.full(len(rows), np.inf, F), np.full(len(rows), -1, np.int32), np.zeros(len(rows), bool)
        buvw = np.zeros((len(rows), 4), F)                                  # the winner's U, V, W, det
        count = 0
        for t in D.tile_walk(start[w] if start is not None else 0, n):
            if cull:
                done = r["dead"] | found if mode == 1 else r["dead"]
                if done.all():
                    break
                if not (~done & tile_wanted(dict(tile_box=R["tile_box"][t:t + 1]), r, best)[:, 0]).any():
                    continue
            count += 1
            A, B, C = (shear(rows_of[t, :, k:k + 3], r) for k in (0, 3, 6))
            U, V, W, det, th, acc = tri_terms(A, B, C, r["t_min"][:, None], r["t_max"][:, None])
            acc &= ~r["dead"][:, None] & (slot_tri[t] >= 0)[None, :]
            for j in range(TILE):                                           # slot by slot, as the lanes do
                if mode == 1:                                               # best stays +inf: any hit will do
                    found |= acc[:, j]
                    continue
                win = acc[:, j] & D.better(th[:, j], slot_tri[t, j], best, btri)
                best = np.where(win, th[:, j], best)
                btri = np.where(win, slot_tri[t, j], btri).astype(np.int32)
                buvw = np.where(win[:, None], np.stack([U[:, j], V[:, j], W[:, j], det[:, j]], -1), buvw)
        with np.errstate(all="ignore"):
            rdet = F(1) / buvw[:, 3:4]
            t_out[rows], tri[rows], bary[rows] = best, btri, np.where(btri[:, None] >= 0, buvw[:, 0:3] * rdet, F(0))
        hit[rows] = found
        visited.append(count)
    first = mode == 0
    return (t_out if first else None, tri if first else None, bary if first else None, None if first else hit, np.array(visited))


# ---------------------------------------------------------------- Moeller-Trumbore --------------------------------------------
def moller_trumbore(R, o, d, dtype=np.float64, pairs=1 << 20):
    """The textbook test over the kept triangles in `dtype`, both faces, t > 0 -> t, tri (-1: none), (u, v) of the nearest hit."""
    ty = np.dtype(dtype).type
    o, d = np.asarray(o, dtype=dtype).reshape(-1, 3), np.asarray(d, dtype=dtype).reshape(-1, 3)
    kept = np.flatnonzero(R["dropped"] == 0)
    v = R["verts"].astype(dtype)[R["tris"][kept]]
    a, e1, e2 = v[None, :, 0], (v[:, 1] - v[:, 0])[None], (v[:, 2] - v[:, 0])[None]
    Q = len(o)
    t_out, tri, uv = np.full(Q, np.inf, dtype), np.full(Q, -1, np.int32), np.zeros((Q, 2), dtype)
    step = max(1, pairs // max(len(kept), 1))
    for i in range(0, Q, step):
        oo, dd = o[i:i + step, None, :], d[i:i + step, None, :]
        with np.errstate(all="ignore"):
            pv = np.cross(dd, e2)
            det = D.dot(e1, pv)
            inv = ty(1) / det
            tv = oo - a
            u = D.dot(tv, pv) * inv
            qv = np.cross(tv, e1)
            w = D.dot(dd, qv) * inv
            t = D.dot(e2, qv) * inv
            ok = (det != 0) & (u >= 0) & (w >= 0) & (u + w <= 1) & (t > 0)
        t = np.where(ok, t, np.inf)
        j = t.argmin(1)
        rows = np.arange(len(j))
        any_ = ok.any(1)
        t_out[i:i + step] = np.where(any_, t[rows, j], np.inf)
        tri[i:i + step] = np.where(any_, kept[j], -1)
        uv[i:i + step] = np.where(any_[:, None], np.stack([u[rows, j], w[rows, j]], -1), 0)
    return t_out, tri, uv
