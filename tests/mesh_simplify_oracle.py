"""The contract of simplify_mesh (include/mocoflow_hip.h mf_simplify_mesh_*), restated in numpy with float64 and int64: the
oracle of tests/test_mesh_simplify_cpu.py and tests/test_gpu_mesh_simplify.py, and the meshes both files use.  It shares no
code with the product: np.floor / np.rint for the cells, np.unique on the rotation-canonical cell triples (its first
occurrence is the smallest triangle index), np.minimum.at / np.add.at for what the device does with integer atomics."""
import functools

import numpy as np

FRAC = 2.0 ** 20


class BadMesh(Exception):
    """A vertex that is not finite or outside [lo, hi], or a triangle index outside [0, V)."""


def grid(verts, cell, lo=None, hi=None):
    """(lo, hi, n): float64 bounds (the vertices' own when not given) and int64 cells per axis."""
    if lo is None:
        lo = verts.min(0) if len(verts) else np.zeros(3)
        hi = verts.max(0) if len(verts) else np.zeros(3)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
        raise BadMesh("bounds")
    n = (np.floor((hi - lo) / np.float64(cell)) + 1.0).astype(np.int64)
    return lo, hi, n


def simplify(verts, tris, cell, lo=None, hi=None, placement="mean", attrs=()):
    """-> (verts_k, tris_k, first, cluster, *attrs_k) as numpy arrays; raises BadMesh where the device raises RuntimeError."""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    V = len(verts)
    cell = np.float64(cell)
    lo, hi, n = grid(verts, cell, lo, hi)
    x = verts.astype(np.float64)
    with np.errstate(invalid="ignore"):
        if not (np.isfinite(x).all() and (x >= lo).all() and (x <= hi).all()):
            raise BadMesh("vertex")
    if len(tris) and (tris.min() < 0 or tris.max() >= V):
        raise BadMesh("index")
    t = (x - lo) / cell
    c = np.floor(t)
    q = np.rint((t - c) * FRAC).astype(np.int64)
    c = c.astype(np.int64)
    cid = (c[:, 0] * n[1] + c[:, 1]) * n[2] + c[:, 2]
    tc = cid[tris]                                                       # (T, 3) cells of the corners
    alive = np.nonzero((tc[:, 0] != tc[:, 1]) & (tc[:, 1] != tc[:, 2]) & (tc[:, 0] != tc[:, 2]))[0]
    start = np.argmin(tc[alive], 1)                                      # rotate the smallest cell to the front
    canon = np.stack([tc[alive, (start + j) % 3] for j in range(3)], 1)
    _, where = np.unique(canon, axis=0, return_index=True)               # first occurrence: the smallest triangle index
    keep = np.sort(alive[where])
    used = np.unique(tc[keep])                                           # the new vertices: used cells, ascending
    Vk = len(used)
    pos = np.searchsorted(used, cid)
    member = (pos < Vk) & (used[np.minimum(pos, max(Vk - 1, 0))] == cid) if Vk else np.zeros(V, bool)
    cluster = np.where(member, pos, -1).astype(np.int64)
    first = np.full(Vk, V, np.int64)
    np.minimum.at(first, cluster[member], np.nonzero(member)[0])
    tris_k = np.searchsorted(used, tc[keep]).astype(np.int64).reshape(-1, 3)
    if placement == "first":
        verts_k = verts[first]
    else:
        S = np.zeros((Vk, 3), np.int64)
        np.add.at(S, cluster[member], q[member])
        cnt = np.bincount(cluster[member], minlength=Vk).astype(np.float64)
        cu = np.stack([used // (n[1] * n[2]), used // n[2] % n[1], used % n[2]], 1).astype(np.float64)
        verts_k = (lo + cell * (cu + (S.astype(np.float64) / cnt[:, None]) / FRAC)).astype(np.float32)
    return (verts_k.reshape(-1, 3), tris_k, first, cluster) + tuple(np.asarray(a)[first] for a in attrs)


def duplicate_classes(verts, tris, cell, lo=None, hi=None):
    """Sizes of the duplicate classes of the non-degenerate triangles, descending (the CPU tests' proof that a fixture has some)."""
    verts, tris = np.asarray(verts, np.float32), np.asarray(tris, np.int64)
    lo, hi, n = grid(verts, cell, lo, hi)
    c = np.floor((verts.astype(np.float64) - lo) / np.float64(cell)).astype(np.int64)
    tc = ((c[:, 0] * n[1] + c[:, 1]) * n[2] + c[:, 2])[tris]
    tc = tc[(tc[:, 0] != tc[:, 1]) & (tc[:, 1] != tc[:, 2]) & (tc[:, 0] != tc[:, 2])]
    start = np.argmin(tc, 1)
    canon = np.stack([tc[np.arange(len(tc)), (start + j) % 3] for j in range(3)], 1)
    return np.sort(np.unique(canon, axis=0, return_counts=True)[1])[::-1]


# ---------------------------------------------------------------- the meshes of both test files
def hand_meshes():
    """name -> (verts, tris, cell, lo, hi): at most 12 triangles each, unit cells over [0, 4]^3 unless said otherwise."""
    lo, hi = (0.0, 0.0, 0.0), (4.0, 4.0, 4.0)
    f = lambda rows: np.array(rows, np.float32).reshape(-1, 3)
    i = lambda rows: np.array(rows, np.int64).reshape(-1, 3)
    A, B, C, D = (0.5, 0.5, 0.5), (1.5, 0.5, 0.5), (0.5, 1.5, 0.5), (1.5, 1.5, 2.5)
    out = {}
    # triangle 2 is triangle 0 rotated and made of other vertices of the same cells: the lower index survives
    out["rotated_duplicate"] = (f([A, B, C, (0.25, 0.75, 0.25), (1.75, 0.25, 0.75), (0.75, 1.25, 0.25), D]),
                                i([[0, 1, 2], [1, 6, 2], [5, 3, 4], [4, 5, 3], [2, 0, 1]]), 1.0, lo, hi)
    # the same three cells in the opposite winding: not duplicates, both survive
    out["opposite_winding"] = (f([A, B, C, (0.75, 0.25, 0.75), (1.25, 0.75, 0.25), (0.25, 1.75, 0.75)]),
                               i([[0, 1, 2], [3, 5, 4], [2, 1, 0]]), 1.0, lo, hi)
    # triangle 1 has two corners in one cell
    out["degenerate"] = (f([A, B, C, (0.75, 0.75, 0.75), D]), i([[0, 1, 2], [0, 3, 4], [1, 2, 4], [3, 3, 3]]), 1.0, lo, hi)
    # vertices 3 and 5 are in no triangle; 5 shares a used cell and is clustered, 3 sits alone and is dropped
    out["unused_vertex"] = (f([A, B, C, (3.5, 3.5, 3.5), D, (0.75, 0.25, 0.25)]), i([[0, 1, 2], [2, 1, 4]]), 1.0, lo, hi)
    # a speck (vertices 4..7, four triangles) that falls into one cell: its vertices go, cluster = -1
    out["speck"] = (f([A, B, C, D, (3.1, 3.1, 3.1), (3.4, 3.1, 3.1), (3.1, 3.4, 3.1), (3.1, 3.1, 3.4)]),
                    i([[0, 1, 2], [1, 3, 2], [4, 5, 6], [4, 6, 7], [4, 7, 5], [5, 7, 6]]), 1.0, lo, hi)
    # a closed tetrahedron, an octahedron's worth of faces around it, twelve triangles; cells of edge 0.75 from lo = -0.1
    v = f([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1), (0.1, 0.1, 0.05), (0.6, 0.05, 0.1)])
    t = i([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2], [4, 7, 5], [4, 6, 7], [1, 4, 5], [2, 6, 4], [3, 5, 6], [8, 9, 2], [9, 8, 3],
           [5, 7, 6]])
    out["twelve"] = (v, t, 0.75, (-0.1, -0.1, -0.1), (1.3, 1.3, 1.3))
    return out


@functools.lru_cache(maxsize=None)
def sphere():
    """(verts, tris) of the marching-cubes mesh (tests/mc_oracle.py) of a sphere of radius 8.3 on a 24^3 lattice.  Its
    distance field carries a ripple of 1.6 lattice steps: a smooth sphere clusters without a single duplicate class, the
    folds of the rippled one give some at every cell size of SPHERE_CELLS."""
    import mc_oracle as O
    g = np.arange(24, dtype=np.float32)
    X, Y, Z = np.meshgrid(g, g, g, indexing="ij")
    d = np.sqrt((X - 11.3) ** 2 + (Y - 12.1) ** 2 + (Z - 11.6) ** 2) + 1.6 * np.sin(2.1 * X) * np.sin(2.6 * Y + 1) * np.sin(2.3 * Z + 2)
    verts, tris = O.marching_cubes(d.astype(np.float32), 8.3)
    return np.ascontiguousarray(verts, np.float32), np.ascontiguousarray(tris, np.int64)


SPHERE_BOUNDS = ((0.0, 0.0, 0.0), (23.0, 23.0, 23.0))
SPHERE_CELLS = (2.0, 3.0, 5.5)
SHEET_N = 740


@functools.lru_cache(maxsize=None)
def sheet():
    """A 740 x 740 height field: 547 600 vertices, 1 092 242 triangles, both above 2048 x 256.  x = row, y = column (exact
    integers), z a smooth height with a fine ripple, 0 .. 60.  The last four rows of vertices repeat the positions of the four
    before them, so their triangles are duplicates (other vertices, the same cells, the same winding) at any cell size."""
    N = SHEET_N
    i, j = np.meshgrid(np.arange(N, dtype=np.float64), np.arange(N, dtype=np.float64), indexing="ij")
    z = 30.0 + 24.0 * np.sin(i / 37.0) * np.cos(j / 23.0) + 5.5 * np.sin(i * 1.7 + j * 0.9)
    grid_pos = np.stack([i, j, z], -1)
    grid_pos[N - 4:] = grid_pos[N - 8:N - 4]
    verts = grid_pos.reshape(-1, 3).astype(np.float32)
    a = (np.arange(N - 1)[:, None] * N + np.arange(N - 1)[None, :]).reshape(-1).astype(np.int64)
    tris = np.concatenate([np.stack([a, a + N, a + 1], 1), np.stack([a + 1, a + N, a + N + 1], 1)])
    tris = tris[np.random.default_rng(3).permutation(len(tris))]
    assert verts.shape == (547600, 3) and tris.shape == (1092242, 3)
    return verts, np.ascontiguousarray(tris)


SHEET_BOUNDS = ((0.0, 0.0, 0.0), (739.0, 739.0, 60.0))
FAN_T = 50_000


@functools.lru_cache(maxsize=None)
def fan():
    """50 000 triangles whose corners fall into the 8 cells of a 2 x 2 x 2 grid: a handful of key classes, thousands of
    triangles racing for each slot.  Vertex v lies in cell v % 8, at a position of its own inside it."""
    rng = np.random.default_rng(5)
    V = 4096
    cellbits = np.arange(V) % 8
    corner = np.stack([(cellbits >> 2) & 1, (cellbits >> 1) & 1, cellbits & 1], 1).astype(np.float64)
    verts = (corner + rng.uniform(0.05, 0.95, (V, 3))).astype(np.float32)
    tris = rng.integers(0, V, (FAN_T, 3)).astype(np.int64)
    return verts, tris


FAN_BOUNDS = ((0.0, 0.0, 0.0), (1.99, 1.99, 1.99))


@functools.lru_cache(maxsize=None)
def expected(name, cell, given, placement="mean"):
    """The oracle's result on a named fixture, computed once and shared: (verts_k, tris_k, first, cluster, attr_k)."""
    verts, tris, bounds = {"sphere": (*sphere(), SPHERE_BOUNDS), "sheet": (*sheet(), SHEET_BOUNDS), "fan": (*fan(), FAN_BOUNDS)}[name]
    lo, hi = bounds if given else (None, None)
    return simplify(verts, tris, cell, lo, hi, placement, attrs=(attribute(len(verts)),))


def attribute(V):
    """An int16 (V, 3) per-vertex attribute: rows that say which vertex they came from, in an odd row size (6 bytes)."""
    return (np.arange(V, dtype=np.int64)[:, None] * 7 + np.arange(3)).astype(np.int16)
