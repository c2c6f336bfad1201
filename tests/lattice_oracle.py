"""numpy restatement of the sparse lattice query (include/mocoflow_hip.h: mf_lattice_select, mf_lattice_points,
mf_lattice_scatter; the host tables of moco_flow_amd.points.brick_cell_ranges), brick by brick and point by point.

Everything the kernels decide is integer work on tables the host builds in fp32, so there is no tolerance anywhere: the cell of
a coordinate is mf_ray_clip's -- floor((c - lo) * inv_cell) in fp32, every operation rounded once, clamped to [0, G - 1] -- and
the loops below are written for the shapes of the tests, not for speed."""
import numpy as np

BRICK = 8
EMPTY = (1, 0)


def n_bricks(n):
    return tuple((int(v) + BRICK - 1) // BRICK for v in n)


def cell(x, lo, inv, cells):
    """occ_cell of csrc/mf_occupancy.hip for one fp32 coordinate."""
    x, lo, inv = np.float32(x), np.float32(lo), np.float32(inv)
    with np.errstate(over="ignore", invalid="ignore"):
        f = np.floor(np.float32(np.float32(x - lo) * inv))
    f = f if f >= 0 else np.float32(0)
    top = np.float32(cells - 1)
    f = f if f <= top else top
    return min(int(f), cells - 1)


def range_table(axis, margin, lo, hi, inv, cells):
    """(nb, 2) int32: per brick the first and last cell its grown index range touches, or EMPTY."""
    X = np.asarray(axis, dtype=np.float32)
    n = len(X)
    out = np.zeros((n_bricks([n])[0], 2), dtype=np.int32)
    for b in range(len(out)):
        i0, i1 = max(BRICK * b - margin, 0), min(BRICK * b + BRICK - 1 + margin, n - 1)
        if X[i1] < np.float32(lo) or X[i0] > np.float32(hi):
            out[b] = EMPTY
        else:
            out[b] = (cell(X[i0], lo, inv, cells), cell(X[i1], lo, inv, cells))
    return out


def range_tables(axes, margin, dims, lo, hi, inv_cell, world_of_axis=(0, 1, 2)):
    """The three tables of a lattice against a grid of ``dims`` cells over lo .. hi: volume axis a looks at grid axis
    world_of_axis[a]."""
    return [range_table(axes[a], margin, lo[w], hi[w], inv_cell[w], dims[w]) for a, w in enumerate(world_of_axis)]


def select(dense, tables, n, world_of_axis=(0, 1, 2)):
    """mf_lattice_select on the grid as a bool array (Gx, Gy, Gz): (slot (nb0 nb1 nb2,) int32, brick_ids (K,) int32, K)."""
    nb = n_bricks(n)
    slot = np.full(nb[0] * nb[1] * nb[2], -1, dtype=np.int32)
    ids = []
    for lin, b in enumerate(np.ndindex(*nb)):                      # b0 slowest, b2 fastest
        box = [None] * 3
        for a in range(3):
            c0, c1 = (int(v) for v in tables[a][b[a]])
            c0, c1 = max(c0, 0), min(c1, dense.shape[world_of_axis[a]] - 1)
            box[world_of_axis[a]] = slice(c0, c1 + 1) if c0 <= c1 else None
        if all(s is not None for s in box) and dense[tuple(box)].any():
            slot[lin] = len(ids)
            ids.append(lin)
    return slot, np.asarray(ids, dtype=np.int32), len(ids)


def select_fast(dense, tables, n, world_of_axis=(0, 1, 2)):
    """``select`` for lattices of many bricks, all bricks at once: the number of occupied cells in a brick's box from the
    3-D summed-area table of the grid (int64, exact).  ``select`` stays the definition; tests/test_lattice_cpu.py holds this
    one to it."""
    nb = n_bricks(n)
    sat = np.zeros(tuple(g + 1 for g in dense.shape), dtype=np.int64)
    sat[1:, 1:, 1:] = dense.astype(np.int64).cumsum(0).cumsum(1).cumsum(2)
    first, past, some = [None] * 3, [None] * 3, np.ones(nb, dtype=bool)
    for a in range(3):
        w = world_of_axis[a]
        t = np.asarray(tables[a], dtype=np.int64).reshape(nb[a], 2)
        c0, c1 = np.maximum(t[:, 0], 0), np.minimum(t[:, 1], dense.shape[w] - 1)
        shape = [1, 1, 1]
        shape[a] = nb[a]
        ok = c0 <= c1
        first[w], past[w] = np.where(ok, c0, 0).reshape(shape), np.where(ok, c1 + 1, 0).reshape(shape)
        some = some & ok.reshape(shape)
    cells = np.zeros(nb, dtype=np.int64)
    for corner in np.ndindex(2, 2, 2):                             # inclusion and exclusion over the box's eight corners
        at = tuple(np.broadcast_to(past[w] if corner[w] else first[w], nb) for w in range(3))
        cells += (-1) ** (3 - sum(corner)) * sat[at]
    on = (some & (cells > 0)).reshape(-1)
    ids = np.flatnonzero(on).astype(np.int32)
    return np.where(on, np.cumsum(on) - 1, -1).astype(np.int32), ids, len(ids)


def points(brick_ids, axes, world_of_axis=(0, 1, 2)):
    """mf_lattice_points: (K 512, 3) fp32."""
    n = [len(a) for a in axes]
    nb = n_bricks(n)
    out = np.zeros((len(brick_ids) * BRICK ** 3, 3), dtype=np.float32)
    l0, l1, l2 = np.meshgrid(np.arange(BRICK), np.arange(BRICK), np.arange(BRICK), indexing="ij")
    local = [l0.reshape(-1), l1.reshape(-1), l2.reshape(-1)]       # l2 fastest
    for r, lin in enumerate(brick_ids):
        b = np.unravel_index(int(lin), nb)
        for a in range(3):
            idx = np.minimum(BRICK * b[a] + local[a], n[a] - 1)
            out[r * BRICK ** 3:(r + 1) * BRICK ** 3, world_of_axis[a]] = np.asarray(axes[a], dtype=np.float32)[idx]
    return out


def scatter(sigma, slot, n, fill):
    """mf_lattice_scatter: the dense (n0, n1, n2) fp32 volume of the compact rows."""
    nb = n_bricks(n)
    sigma = np.asarray(sigma, dtype=np.float32).reshape(-1)
    vol = np.full(n, fill, dtype=np.float32)
    i0, i1, i2 = np.indices(n)
    s = np.asarray(slot)[((i0 // BRICK) * nb[1] + i1 // BRICK) * nb[2] + i2 // BRICK].astype(np.int64)
    on = s >= 0
    local = (i0 % BRICK) * 64 + (i1 % BRICK) * 8 + i2 % BRICK
    vol[on] = sigma[s[on] * BRICK ** 3 + local[on]]
    return vol


def gather(vol, brick_ids):
    """The compact rows a dense volume holds for ``brick_ids`` (a partial brick repeats its last point): scatter's inverse."""
    n = vol.shape
    ax = [np.arange(v, dtype=np.float32) for v in n]
    idx = points(brick_ids, ax).astype(np.int64)
    return vol[idx[:, 0], idx[:, 1], idx[:, 2]].astype(np.float32)


def active_mask(slot, n):
    """bool (n0, n1, n2): the points of active bricks."""
    nb = n_bricks(n)
    on = (slot >= 0).reshape(nb)
    return np.repeat(np.repeat(np.repeat(on, BRICK, 0), BRICK, 1), BRICK, 2)[:n[0], :n[1], :n[2]]
