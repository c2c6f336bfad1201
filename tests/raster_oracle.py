"""numpy restatement of the rasterizer's contract (moco_flow_amd/csrc/mf_raster.hip), test-only.

    project(verts, c2w, f, cx, cy, znear, dtype)   the projection in `dtype` (float64: the truth; float32: the yardstick)
    snap(xy)                                       rint(256 x) as int64
    coverage(screen, tris, H, W, off)              per triangle: the integer edge values e (T, H, W, 3) after the winding sign, and
                                                   the covered mask under the top-left rule -- integers only
    rasterize(screen, inv_z, tris, H, W, off, dtype)   face / depth / bary with depth and barycentrics in `dtype`, the nearest
                                                   covering triangle by (depth, index)
    icosphere(level), grid_mesh(nx, ny, ...)       test meshes"""
import numpy as np

BEHIND = -2 ** 31
GUARD = 1 << 23


def project(verts, c2w, f, cx, cy, znear=1e-3, dtype=np.float64):
    """-> x, y, inv_z (V,) in `dtype` and ok (V,) bool (z > znear); with dtype float32 every operation is rounded once, in the
    kernel's order."""
    t = dtype
    v = np.asarray(verts).astype(t)
    m = np.asarray(c2w, dtype=np.float64)[:3, :4].astype(np.float32).astype(t)
    f, cx, cy = t(np.float32(f)), t(np.float32(cx)), t(np.float32(cy))
    p = v - m[:, 3]
    cam = [(m[0, a] * p[:, 0] + m[1, a] * p[:, 1]) + m[2, a] * p[:, 2] for a in range(3)]
    z = -cam[2]
    ok = z > t(np.float32(znear))
    with np.errstate(divide="ignore", invalid="ignore"):
        x = cx + (f * cam[0]) / z
        y = cy - (f * cam[1]) / z
        inv_z = t(1) / z
    return x, y, np.where(ok, inv_z, t(0)), ok


def snap(x):
    return np.rint(np.asarray(x, dtype=np.float64) * 256).astype(np.int64)


def tri_status(screen, tris, V):
    """(dropped (T,), sign (T,)) of the contract: dropped = a vertex index outside [0, V), a flagged vertex or one beyond the guard band."""
    tris = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    screen = np.asarray(screen, dtype=np.int64).reshape(-1, 2)
    bad_index = ((tris < 0) | (tris >= V)).any(axis=1)
    safe = np.where(bad_index[:, None], 0, tris) if V > 0 else np.zeros_like(tris)
    if V == 0:
        return np.ones(len(tris), bool), np.zeros(len(tris), np.int64)
    p = screen[safe]                                                    # (T, 3, 2)
    dropped = bad_index | (p[:, :, 0] == BEHIND).any(axis=1) | (np.abs(p) > GUARD).any(axis=(1, 2))
    area = (p[:, 1, 0] - p[:, 0, 0]) * (p[:, 2, 1] - p[:, 0, 1]) - (p[:, 1, 1] - p[:, 0, 1]) * (p[:, 2, 0] - p[:, 0, 0])
    return dropped, np.where(dropped, 0, np.sign(area))


def coverage(screen, tris, H, W, off=0):
    """e (T, H, W, 3) int64 edge values (winding sign applied) and covered (T, H, W) bool; off = 0 or 128 sub-pixel units."""
    tris = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    screen = np.asarray(screen, dtype=np.int64).reshape(-1, 2)
    T, V = len(tris), len(screen)
    dropped, sgn = tri_status(screen, tris, V)
    sx = (np.arange(W, dtype=np.int64) * 256 + off)[None, None, :]
    sy = (np.arange(H, dtype=np.int64) * 256 + off)[None, :, None]
    e = np.zeros((T, H, W, 3), np.int64)
    cov = np.ones((T, H, W), bool) & (sgn != 0)[:, None, None]
    if V == 0 or T == 0:
        return e, cov & False
    p = screen[np.where((sgn == 0)[:, None], 0, tris)]
    for k in range(3):
        a, b = p[:, (k + 1) % 3], p[:, (k + 2) % 3]
        dx, dy = (sgn * (b[:, 0] - a[:, 0]))[:, None, None], (sgn * (b[:, 1] - a[:, 1]))[:, None, None]
        e[..., k] = dx * (sy - a[:, 1][:, None, None]) - dy * (sx - a[:, 0][:, None, None])
        top_left = (dy < 0) | ((dy == 0) & (dx > 0))
        cov &= np.where(top_left, e[..., k] >= 0, e[..., k] > 0)
    return e, cov


def shade(e, inv_z_tri, dtype=np.float64):
    """depth (…,) and bary (…, 3) from edge values e (…, 3) and the vertices' inv_z (…, 3) in `dtype`, the kernel's order."""
    t = dtype
    fk = e.astype(t) * np.asarray(inv_z_tri).astype(t)
    den = (fk[..., 0] + fk[..., 1]) + fk[..., 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        z = e.sum(axis=-1).astype(t) / den
        bary = fk / den[..., None]
    return z, bary


def rasterize(screen, inv_z, tris, H, W, off=0, dtype=np.float64):
    """-> face (H, W) int32, depth (H, W), bary (H, W, 3), second (H, W): the nearest covering triangle by (depth, index) with
    depth in `dtype`, and the depth of the second-nearest covering triangle (+inf without one)."""
    tris = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    T = len(tris)
    e, cov = coverage(screen, tris, H, W, off)
    face = np.full((H, W), -1, np.int32)
    depth = np.full((H, W), np.inf, dtype)
    second = np.full((H, W), np.inf, dtype)
    bary = np.zeros((H, W, 3), dtype)
    if T == 0 or not cov.any():
        return face, depth, bary, second
    w = np.asarray(inv_z)[np.where(cov.any(axis=(1, 2))[:, None], tris, 0)]       # (T, 3)
    z, b = shade(e, w[:, None, None, :], dtype)
    z = np.where(cov, z, np.inf)
    order = np.argsort(z, axis=0, kind="stable")                        # ties: the lower index first
    first = order[0]
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    hit = cov.any(axis=0)
    face[hit] = first[hit]
    depth = np.where(hit, z[first, jj, ii], np.inf).astype(dtype)
    bary = np.where(hit[..., None], b[first, jj, ii], 0).astype(dtype)
    if T > 1:
        second = z[order[1], jj, ii]
    return face, depth, bary, second


def quantise(v):
    """(uint8) clamp(v 255 + 0.5, 0, 255) in fp32, truncated (vis.frame_sheet's rounding)."""
    t = np.asarray(v, dtype=np.float32) * np.float32(255) + np.float32(0.5)
    return np.clip(np.nan_to_num(t, nan=0.0), 0, 255).astype(np.uint8)


def interpolate(attrs, tris, face, bary, dtype=np.float32):
    """(H, W, C) = (b0 a0 + b1 a1) + b2 a2 in `dtype`; zeros where face < 0."""
    a = np.asarray(attrs).astype(dtype)
    tris = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    hit = face >= 0
    vi = tris[np.where(hit, face, 0)] if len(tris) else np.zeros(face.shape + (3,), np.int64)
    b = np.asarray(bary).astype(dtype)
    if len(a) == 0 or len(tris) == 0:
        return np.zeros(face.shape + (a.shape[1],), dtype)
    out = (b[..., 0:1] * a[vi[..., 0]] + b[..., 1:2] * a[vi[..., 1]]) + b[..., 2:3] * a[vi[..., 2]]
    return np.where(hit[..., None], out, 0).astype(dtype)


def icosphere(level=2, radius=1.0, center=(0, 0, 0)):
    """verts (V, 3) float64, tris (T, 3) int64: level 2 has 162 vertices and 320 triangles, outward winding."""
    g = (1 + np.sqrt(5)) / 2
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1),
         (-g, 0, -1), (-g, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, nf = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v) * radius + np.asarray(center, dtype=np.float64), np.array(f, dtype=np.int64)


def grid_mesh(nx, ny, x0=0.0, y0=0.0, dx=1.0, dy=1.0, flip=False, alternate=True):
    """A planar (nx x ny cells) mesh of 2 nx ny triangles over the points (x0 + i dx, y0 + j dy), as 2-D positions (V, 2) float64 and
    tris (T, 3) int64; `alternate` switches the diagonal from cell to cell; `flip` reverses every winding."""
    ii, jj = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="xy")
    pts = np.stack([x0 + ii.ravel() * dx, y0 + jj.ravel() * dy], axis=1).astype(np.float64)
    idx = lambda i, j: j * (nx + 1) + i
    tris = []
    for j in range(ny):
        for i in range(nx):
            a, b, c, d = idx(i, j), idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)
            if alternate and (i + j) % 2:
                tris += [(a, b, d), (b, c, d)]
            else:
                tris += [(a, b, c), (a, c, d)]
    tris = np.array(tris, dtype=np.int64).reshape(-1, 3)
    return pts, (tris[:, ::-1].copy() if flip else tris)
