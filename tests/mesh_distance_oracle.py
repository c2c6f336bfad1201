"""The numpy restatement of csrc/mf_mesh_distance.hip's contract (include/mocoflow_hip.h, "mesh-to-mesh distances"): every
operation in np.float32, rounded once, in the header's order, with dot(x, y) = (x0 y0 + x1 y1) + x2 y2 and max / min that ignore
a NaN (np.fmax / np.fmin, as fmaxf / fminf do).  Brute force and chunked: records and the drop rule, the four clamped candidates,
the box clamp, the (value, index) minimum, the integer weights, the 128-bit target in Python integers, the barycentric point, the
statistics; and the culled search a wave performs, restated tile by tile.  The same expressions evaluate in float64 when they are
handed float64 (closest_f64).  The only float comparison that is not bit for bit is the sign of a zero: np.fmax(-0.0, 0.0) and
v_max_f32 need not agree on it, so callers compare with == (np.array_equal), which a NaN still fails."""
import numpy as np

F = np.float32
TILE = 64
WEIGHT_ONE = 1 << 20


def dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def clamp01(x):
    one = x.dtype.type(1)
    return np.fmin(np.fmax(x, x.dtype.type(0)), one)


def box_lb(q, lo, hi):
    g = np.fmax(np.fmax(lo - q, q - hi), q.dtype.type(0))
    return dot(g, g)


# ---------------------------------------------------------------- meshes ------------------------------------------------------
def cube():
    v = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=F)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    t = [[a, b, c] for a, b, c, d in quads] + [[a, c, d] for a, b, c, d in quads]
    return v, np.array(t, dtype=np.int64)


def octahedron():
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=F)
    t = [[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]]
    return v, np.array(t, dtype=np.int64)


def uv_sphere(n_lat=50, n_lon=50, radius=1.0, center=(0.1, -0.2, 0.05)):
    """2 n_lon (n_lat - 1) triangles: 4 900 by default."""
    th = np.linspace(0.0, np.pi, n_lat + 1)[1:-1]
    ph = np.linspace(0.0, 2 * np.pi, n_lon, endpoint=False)
    ring = np.stack([np.sin(th)[:, None] * np.cos(ph), np.sin(th)[:, None] * np.sin(ph), np.cos(th)[:, None] * np.ones_like(ph)], -1)
    v = np.concatenate([[[0, 0, 1.0]], ring.reshape(-1, 3), [[0, 0, -1.0]]]) * radius + np.asarray(center)
    idx = lambda i, j: 1 + i * n_lon + j % n_lon
    t = []
    for j in range(n_lon):
        t.append([0, idx(0, j), idx(0, j + 1)])
        t.append([len(v) - 1, idx(n_lat - 2, j + 1), idx(n_lat - 2, j)])
        for i in range(n_lat - 2):
            t.append([idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)])
            t.append([idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)])
    return v.astype(F), np.array(t, dtype=np.int64)


def soup(seed=5, n_random=2000, n_sliver=500, n_zero=20, n_bad=5, side=3.0):
    """Random triangles in a box of side `side`, slivers (the third vertex on the opposite edge +- 1e-6), zero-area triangles and
    triangles with an index out of range, shuffled: 2 525 triangles."""
    rng = np.random.default_rng(seed)
    a = rng.random((n_random, 3)) * side
    rnd = np.stack([a, a + rng.normal(size=a.shape) * 0.15, a + rng.normal(size=a.shape) * 0.15], 1)
    p, q = rng.random((n_sliver, 3)) * side, rng.random((n_sliver, 3)) * side
    sl = np.stack([p, q, p + (q - p) * rng.random((n_sliver, 1)) + rng.choice([-1e-6, 1e-6], size=(n_sliver, 3))], 1)
    z = rng.random((n_zero, 3)) * side
    zero = np.stack([z, z + 0.2, z + 0.4], 1)                               # collinear
    zero[: n_zero // 2, 1] = zero[: n_zero // 2, 0]                         # and a repeated vertex
    corners = np.concatenate([rnd, sl, zero]).astype(F)
    verts = corners.reshape(-1, 3)
    tris = np.arange(len(verts), dtype=np.int64).reshape(-1, 3)
    bad = np.array([[0, 1, len(verts)], [-1, 2, 3], [4, 1 << 40, 5], [6, 7, -(1 << 35)], [len(verts) + 7, 0, 1]], dtype=np.int64)[:n_bad]
    tris = np.concatenate([tris, bad])
    return verts, tris[rng.permutation(len(tris))]


# ---------------------------------------------------------------- records -----------------------------------------------------
def records(verts, tris, order=None):
    """Everything mf_surface_records writes, as a dict of arrays."""
    verts = np.ascontiguousarray(verts, dtype=F).reshape(-1, 3)
    tris = np.ascontiguousarray(tris, dtype=np.int64).reshape(-1, 3)
    V, T = len(verts), len(tris)
    Tp = -(-T // TILE) * TILE
    order = np.arange(T, dtype=np.int64) if order is None else np.asarray(order, dtype=np.int64)
    tri_slot = np.full(T, -1, dtype=np.int32)
    for s in range(T - 1, -1, -1):                                          # the lowest slot keeps the triangle
        if 0 <= order[s] < T:
            tri_slot[order[s]] = s
    inr = ((tris >= 0) & (tris < V)).all(1)
    ti = np.where(inr[:, None], tris, 0)
    vv = verts if V else np.zeros((1, 3), F)
    with np.errstate(all="ignore"):
        a, b, c = vv[ti[:, 0]], vv[ti[:, 1]], vv[ti[:, 2]]
        ab, ac, bc = b - a, c - a, c - b
        d00, d01, d11 = dot(ab, ab), dot(ab, ac), dot(ac, ac)
        one = F(1)
        r_ab, r_ac, r_bc = one / d00, one / d11, one / dot(bc, bc)
        rden = one / (d00 * d11 - d01 * d01)
        n = np.stack([ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1], ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2], ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]], -1)
        nn = dot(n, n)
        fields = np.concatenate([a, ab, ac, np.stack([r_ab, r_ac, r_bc, d00, d01, d11, rden], -1)], -1).astype(F)
        kept = inr & (nn > 0) & np.isfinite(nn) & np.isfinite(fields).all(1) & (tri_slot >= 0)
        area2 = np.where(kept, np.sqrt(nn), F(0)).astype(F)
        normal = np.where(kept[:, None], n * (one / np.where(kept, area2, one))[:, None], F(0)).astype(F)
    lo, hi = np.fmin(np.fmin(a, b), c), np.fmax(np.fmax(a, b), c)
    rec = np.zeros((Tp, 16), F)
    edges = np.zeros((Tp, 12), F)
    edges[:, 6:9], edges[:, 9:12] = np.inf, -np.inf
    slot_tri = np.full(Tp, -1, dtype=np.int32)
    t = np.flatnonzero(kept)
    s = tri_slot[t]
    rec[s] = fields[t]
    edges[s] = np.concatenate([b[t], bc[t], lo[t], hi[t]], -1)
    slot_tri[s] = t
    tile_box = np.zeros((Tp // TILE, 8), F)
    e = edges.reshape(-1, TILE, 12)
    if Tp:
        tile_box[:, 0:3], tile_box[:, 3:6] = e[:, :, 6:9].min(1), e[:, :, 9:12].max(1)
        tile_box[:, 6] = (slot_tri.reshape(-1, TILE) >= 0).sum(1)
    return dict(records=rec, edges=edges, slot_tri=slot_tri, tile_box=tile_box, tri_slot=tri_slot, verts=verts, tris=tris,
                area2=area2, normal=normal, dropped=(~kept).astype(np.uint8), dropped_count=int((~kept).sum()), V=V, T=T)


# ---------------------------------------------------------------- the value of a triangle -------------------------------------
def tri_value(rec, edges, q):
    """rec (..., 16), edges (..., 12), q (..., 3), broadcast against each other, in the dtype of the arrays (float32: the
    contract; float64: the same expressions evaluated exactly enough to judge it) -> value, region, P, lb."""
    ty = q.dtype.type
    a, ab, ac = rec[..., 0:3], rec[..., 3:6], rec[..., 6:9]
    r_ab, r_ac, r_bc, d00, d01, d11, rden = (rec[..., k] for k in range(9, 16))
    b, bc, lo, hi = edges[..., 0:3], edges[..., 3:6], edges[..., 6:9], edges[..., 9:12]
    with np.errstate(all="ignore"):
        qa = q - a
        d20, d21 = dot(qa, ab), dot(qa, ac)
        p0 = a + ab * clamp01(d20 * r_ab)[..., None]
        p1 = a + ac * clamp01(d21 * r_ac)[..., None]
        p2 = b + bc * clamp01(dot(q - b, bc) * r_bc)[..., None]
        v = clamp01((d11 * d20 - d01 * d21) * rden)
        w = np.fmin(np.fmax((d00 * d21 - d01 * d20) * rden, ty(0)), ty(1) - v)
        p3 = (a + ab * v[..., None]) + ac * w[..., None]
        m = np.full(np.broadcast_shapes(d20.shape), np.inf, dtype=q.dtype)
        region = np.zeros(m.shape, dtype=np.uint8)
        P = np.broadcast_to(p0, m.shape + (3,)).copy()
        for k, p in enumerate((p0, p1, p2, p3)):
            e = q - p
            c = dot(e, e)
            win = c < m
            m = np.where(win, c, m)
            if k:
                region = np.where(win, np.uint8(k), region)
                P = np.where(win[..., None], p, P)
        lb = box_lb(q, lo, hi)
        return np.where(lb > m, lb, m), region, P, lb


def closest(R, query, pairs=1 << 20):
    """Brute force over the kept triangles: d2, tri, point, region -- the lexicographic minimum of (value, caller's index)."""
    q = np.ascontiguousarray(query, dtype=F).reshape(-1, 3)
    Q = len(q)
    d2, tri = np.full(Q, np.inf, F), np.full(Q, -1, np.int32)
    point, region = np.zeros((Q, 3), F), np.zeros(Q, np.uint8)
    t = np.flatnonzero(R["dropped"] == 0)                                   # ascending caller's index
    if not len(t) or not Q:
        return d2, tri, point, region
    s = R["tri_slot"][t]
    rec, edges = R["records"][s], R["edges"][s]
    step = max(1, pairs // len(t))
    for i in range(0, Q, step):
        qq = q[i:i + step]
        val, reg, P, _ = tri_value(rec[None], edges[None], qq[:, None, :])
        best = np.where(np.isnan(val), F(np.inf), val).min(1)
        eq = val == best[:, None]                                           # a NaN never wins
        j = eq.argmax(1)                                                    # the lowest index among equal values
        any_ = eq.any(1)
        rows = np.arange(len(qq))
        d2[i:i + step] = np.where(any_, best, F(np.inf))
        tri[i:i + step] = np.where(any_, t[j], -1)
        point[i:i + step] = np.where(any_[:, None], P[rows, j], F(0))
        region[i:i + step] = np.where(any_, reg[rows, j], 0)
    return d2, tri, point, region


def records_f64(R, t):
    """The records and edge rows of the caller's triangles t, every expression of mf_surface_records evaluated in float64 from the
    fp32 vertices."""
    v = R["verts"].astype(np.float64)
    a, b, c = (v[R["tris"][t, k]] for k in range(3))
    ab, ac, bc = b - a, c - a, c - b
    d00, d01, d11 = dot(ab, ab), dot(ab, ac), dot(ac, ac)
    rec = np.concatenate([a, ab, ac, np.stack([1 / d00, 1 / d11, 1 / dot(bc, bc), d00, d01, d11, 1 / (d00 * d11 - d01 * d01)], -1)], -1)
    return rec, np.concatenate([b, bc, np.minimum(np.minimum(a, b), c), np.maximum(np.maximum(a, b), c)], -1)


def closest_f64(R, query, pairs=1 << 20):
    """The least value over the kept triangles with every expression in float64 -> d2 (Q) float64."""
    q = np.ascontiguousarray(query, dtype=np.float64).reshape(-1, 3)
    t = np.flatnonzero(R["dropped"] == 0)
    rec, edges = records_f64(R, t)
    step = max(1, pairs // max(len(t), 1))
    out = np.full(len(q), np.inf)
    for i in range(0, len(q), step):
        out[i:i + step] = np.nanmin(tri_value(rec[None], edges[None], q[i:i + step, None, :])[0], axis=1)
    return out


def better(d, tri, best, btri):
    """md_better: (d, tri) lexicographically below (best, btri), indices compared as unsigned (-1 = none, the largest)."""
    u = lambda x: np.asarray(x).astype(np.int64) & 0xFFFFFFFF
    return (np.asarray(tri) >= 0) & ((d < best) | ((d == best) & (u(tri) < u(btri))))


def tile_walk(start, n):
    """The tiles a wave visits, in its order: s, s + 1, s - 1, s + 2, ... inside [0, n), s = `start` clamped into it."""
    s = min(max(int(start), 0), n - 1)
    for k in range(2 * max(s, n - 1 - s) + 1):
        d = (k + 1) >> 1
        t = s + d if k & 1 else s - d
        if 0 <= t < n:
            yield t


def closest_culled(R, query, qorder=None, start=None, cull=True):
    """The search as a wave performs it: 64 queries in the visiting order, the tiles of tile_walk, one decision per tile.
    -> d2, tri, slot per query, and the number of tiles each wave evaluated."""
    q = np.ascontiguousarray(query, dtype=F).reshape(-1, 3)
    Q, n = len(q), len(R["tile_box"])
    qorder = np.arange(Q) if qorder is None else np.asarray(qorder)
    d2, tri, slot = np.full(Q, np.inf, F), np.full(Q, -1, np.int32), np.full(Q, -1, np.int64)
    visited = []
    rec, edges, slot_tri = (R[k].reshape(n, TILE, -1) for k in ("records", "edges", "slot_tri"))
    for w in range(-(-Q // TILE)):
        rows = qorder[w * TILE:(w + 1) * TILE]
        qq = q[rows]
        best, btri, bslot = np.full(len(rows), np.inf, F), np.full(len(rows), -1, np.int32), np.full(len(rows), -1, np.int64)
        count = 0
        for t in tile_walk(start[w] if start is not None else 0, n):
            if cull:
                lb = box_lb(qq, R["tile_box"][t, 0:3], R["tile_box"][t, 3:6])
                with np.errstate(invalid="ignore"):
                    if R["tile_box"][t, 6] == 0 or not (lb <= best).any():
                        continue
            count += 1
            val = tri_value(rec[t][None], edges[t][None], qq[:, None, :])[0]
            for j in range(TILE):                                           # slot by slot, as the lanes do
                win = better(val[:, j], slot_tri[t, j, 0], best, btri)
                best = np.where(win, val[:, j], best)
                btri = np.where(win, slot_tri[t, j, 0], btri).astype(np.int32)
                bslot = np.where(win, t * TILE + j, bslot)
        d2[rows], tri[rows], slot[rows] = best, btri, bslot
        visited.append(count)
    return d2, tri, slot, np.array(visited)


# ---------------------------------------------------------------- samples -----------------------------------------------------
def weights(area2, dropped):
    area2 = np.asarray(area2, dtype=F)
    amax = area2.max() if len(area2) else F(0)
    with np.errstate(all="ignore"):
        x = np.floor(area2 * (F(WEIGHT_ONE) / amax))
        w = np.where(x >= 1, np.where(x < 4 * WEIGHT_ONE, x, 4 * WEIGHT_ONE), 1)
    return np.where(np.asarray(dropped) != 0, 0, np.nan_to_num(w, nan=1.0)).astype(np.int64)


def targets(r, total):
    """floor(r total / 2^53) in Python integers, r masked to [0, 2^53)."""
    return [((int(x) & ((1 << 53) - 1)) * int(total)) >> 53 for x in r]


def sample(verts, tris, cum, r, u):
    verts, tris, u = np.asarray(verts, dtype=F), np.asarray(tris, dtype=np.int64), np.asarray(u, dtype=F).reshape(-1, 2)
    n, T, V = len(r), len(tris), len(verts)
    points, tri = np.zeros((n, 3), F), np.full(n, -1, np.int32)
    total = int(cum[-1]) if T else 0
    if total <= 0:
        return points, tri
    t = np.searchsorted(np.asarray(cum, dtype=np.int64), np.array(targets(r, total), dtype=np.int64), side="right")      # the first cum > target
    ok = ((tris[t] >= 0) & (tris[t] < V)).all(1)
    ti = np.where(ok[:, None], tris[t], 0)
    a, b, c = verts[ti[:, 0]], verts[ti[:, 1]], verts[ti[:, 2]]
    s = np.sqrt(u[:, 0])
    b0, b1, b2 = F(1) - s, s * (F(1) - u[:, 1]), s * u[:, 1]
    p = (a * b0[:, None] + b * b1[:, None]) + c * b2[:, None]
    return np.where(ok[:, None], p, F(0)).astype(F), np.where(ok, t, -1).astype(np.int32)


# ---------------------------------------------------------------- statistics --------------------------------------------------
def stats(d2, thresholds=(), tri_src=None, tri_dst=None, n_src=None, n_dst=None):
    """-> dict: sum_d, sum_d2, max_d, sum_nn (float64), within (8 ints), finite, left_out; and abs_d / abs_d2 / abs_nn, the sums
    of the absolute terms (what a summation-order bound is relative to)."""
    d2 = np.asarray(d2, dtype=F)
    n = len(d2)
    ts = np.zeros(n, np.int32) if tri_src is None else np.asarray(tri_src)
    td = np.zeros(n, np.int32) if tri_dst is None else np.asarray(tri_dst)
    left = (ts < 0) | (td < 0)
    with np.errstate(invalid="ignore"):
        use = ~left & (d2 >= 0) & (d2 < np.inf)
        d = np.sqrt(d2[use])
    d64 = d.astype(np.float64)
    out = dict(sum_d=float(d64.sum()), sum_d2=float((d64 * d64).sum()), max_d=float(d64.max()) if len(d64) else 0.0, finite=int(use.sum()),
               left_out=int(left.sum()), within=[int((d <= F(thresholds[k])).sum()) if k < len(thresholds) else 0 for k in range(8)], sum_nn=0.0)
    if n_src is not None and n_dst is not None and tri_src is not None and tri_dst is not None:
        ok = (ts[use] < len(n_src)) & (td[use] < len(n_dst))
        nn = np.abs(dot(np.asarray(n_src, dtype=F)[ts[use][ok]], np.asarray(n_dst, dtype=F)[td[use][ok]])).astype(np.float64)
        out["sum_nn"] = float(nn.sum())
    return out
