"""The contract of mf_grid_edt (include/mocoflow_hip.h; OccupancyGrid.euclid_metric, .squared_distance, .dilated_euclidean and
from_mesh(shell="euclidean")) restated in numpy and Python ints.  No GPU, no package code.

The metric is integers from float64 arithmetic: w_a = floor(65536 (cell_a / cmax)^2), R = ceil(65536 (t / cmax)^2),
r_a = isqrt(R // w_a).  d2 is the brute-force minimum over the set cells, capped at R + 1; ``separable_d2`` is the windowed
three-pass restatement the kernels follow, kept here as a second statement of the same function.  The surface, the fill and the
box dilation come from tests/voxelize_oracle.py."""
import math

import numpy as np

import voxelize_oracle as VO

ONE = 1 << 16                             # the weight of the longest cell edge
R_LIMIT = 1 << 30                         # R stays below it
MAX_SIDE = 1024


def cell_edges(dims, lo, hi):
    """The cell edges in float64 from the fp32 box, as OccupancyGrid.cell holds them."""
    lo32, hi32 = np.asarray(lo, dtype=np.float32), np.asarray(hi, dtype=np.float32)
    return (hi32.astype(np.float64) - lo32.astype(np.float64)) / np.asarray(dims, dtype=np.float64)


def euclid_metric(cell, radius):
    """(w, R, r) as Python ints; ValueError where the contract refuses."""
    c = [float(x) for x in np.asarray(cell, dtype=np.float64).reshape(3)]
    t = float(radius)
    if not all(math.isfinite(x) and x > 0 for x in c) or not (0.0 <= t < math.inf):
        raise ValueError((c, t))
    cmax = max(c)
    w = []
    for x in c:
        q = x / cmax
        w.append(int(math.floor(ONE * (q * q))))
    q = t / cmax
    big = ONE * (q * q)
    if min(w) < 1 or not big < float(R_LIMIT):
        raise ValueError((w, big))
    R = int(math.ceil(big))
    if R >= R_LIMIT:
        raise ValueError(R)
    return tuple(w), R, tuple(math.isqrt(R // x) for x in w)


def squared_distance(dense, w, R, chunk=64):
    """int32 (gx, gy, gz): min(R + 1, min over the set cells of sum w_a (index difference)^2), by brute force in int64."""
    dense = np.asarray(dense, dtype=bool)
    out = np.full(dense.shape, int(R) + 1, dtype=np.int64)
    idx = np.argwhere(dense).astype(np.int64)
    ax = [np.arange(g, dtype=np.int64) for g in dense.shape]
    for s in range(0, len(idx), chunk):
        c = idx[s:s + chunk]
        t = [int(w[a]) * (ax[a][None, :] - c[:, a:a + 1]) ** 2 for a in range(3)]       # (n, g_a) each
        d = t[0][:, :, None, None] + t[1][:, None, :, None] + t[2][:, None, None, :]
        out = np.minimum(out, d.min(0))
    assert out.min() >= 0 and out.max() <= int(R) + 1
    return out.astype(np.int32)


def separable_d2(dense, w, R):
    """The same function as three windowed passes: z -> the distance in cells to the nearest set cell of the row, capped at
    r_z + 1; y and x -> minima over |d| <= r_a of w_a d^2 + the previous pass, capped at R + 1.  Every intermediate is checked
    to fit an int32."""
    dense = np.asarray(dense, dtype=bool)
    gx, gy, gz = dense.shape
    R = int(R)
    r = [math.isqrt(R // int(x)) for x in w]
    cap = R + 1
    g = np.full(dense.shape, r[2] + 1, dtype=np.int64)
    for d in range(0, min(r[2], gz - 1) + 1):
        up, dn = np.zeros_like(dense), np.zeros_like(dense)
        up[:, :, :gz - d] = dense[:, :, d:]
        dn[:, :, d:] = dense[:, :, :gz - d]
        g = np.where((up | dn) & (g > d), d, g)
    tz = np.where(g > r[2], cap, int(w[2]) * np.minimum(g, r[2]) ** 2)
    assert tz.max() <= cap
    passes = tz
    for a in (1, 0):
        prev, n = passes, dense.shape[a]
        best = np.full(dense.shape, cap, dtype=np.int64)
        for d in range(-min(r[a], n - 1), min(r[a], n - 1) + 1):
            src, dst = [slice(None)] * 3, [slice(None)] * 3
            src[a] = slice(max(d, 0), n + min(d, 0))
            dst[a] = slice(max(-d, 0), n + min(-d, 0))
            term = int(w[a]) * d * d + prev[tuple(src)]
            assert int(w[a]) * d * d <= R and term.max() <= 2 * R + 1 < 1 << 31
            best[tuple(dst)] = np.minimum(best[tuple(dst)], term)
        passes = np.minimum(best, cap)
    return passes.astype(np.int32)


def dilate_euclidean(dense, cell, radius):
    """The cells with d2 <= R in the metric of (cell, radius)."""
    w, R, _ = euclid_metric(cell, radius)
    return squared_distance(dense, w, R) <= R


def from_mesh_euclidean(verts, tris, dims, lo, hi, dilate_cells=1, thickness=0.0, solid=True):
    """(dense, dropped) of OccupancyGrid.from_mesh(shell="euclidean"): surface, fill if solid, the Euclidean dilation by the
    thickness, the box dilation by dilate_a + 1."""
    dense, dropped = VO.surface(verts, tris, dims, lo, hi)
    if solid:
        dense = VO.fill(dense)
    dense = dilate_euclidean(dense, cell_edges(dims, lo, hi), thickness)
    d = (dilate_cells,) * 3 if np.isscalar(dilate_cells) else tuple(dilate_cells)
    return VO.dilate(dense, tuple(int(x) + 1 for x in d)), dropped
