"""The contracts of vertex_rings and smooth_mesh (include/mocoflow_hip.h mf_rings_mesh_*, mf_smooth_mesh), restated in numpy: the
oracle of tests/test_mesh_smooth_cpu.py and tests/test_gpu_mesh_smooth.py, and the meshes both files use.  It shares no code
with the product: np.unique on i V + j keys for the rings, and a float32 accumulation vectorised by the RANK of a neighbour in
its ring, so that every vertex adds its neighbours in ascending order and every operation is rounded to float32 once."""
import functools

import numpy as np

import mesh_simplify_oracle as S

LAM, MU = 0.5, -0.53


class BadMesh(Exception):
    """A triangle index outside [0, V)."""


def rings(tris, V):
    """-> (offsets (V + 1,) int64, ring (R,) int64, boundary (V,) bool)."""
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    V = int(V)
    if len(tris) and (tris.min() < 0 or tris.max() >= V):
        raise BadMesh("index")
    keep = tris[(tris[:, 0] != tris[:, 1]) & (tris[:, 1] != tris[:, 2]) & (tris[:, 0] != tris[:, 2])]
    i = np.concatenate([keep[:, 0], keep[:, 1], keep[:, 1], keep[:, 2], keep[:, 2], keep[:, 0]])
    j = np.concatenate([keep[:, 1], keep[:, 0], keep[:, 2], keep[:, 1], keep[:, 0], keep[:, 2]])
    keys, m = np.unique(i * V + j, return_counts=True)                   # ascending by i, then j; m(i, j)
    owner = keys // V if V else keys
    offsets = np.zeros(V + 1, np.int64)
    np.cumsum(np.bincount(owner, minlength=V), out=offsets[1:])
    boundary = np.zeros(V, bool)
    boundary[owner[m == 1]] = True
    return offsets, (keys % V if V else keys).astype(np.int64), boundary


def max_multiplicity(tris, V):
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    keep = tris[(tris[:, 0] != tris[:, 1]) & (tris[:, 1] != tris[:, 2]) & (tris[:, 0] != tris[:, 2])]
    i = np.concatenate([keep[:, 0], keep[:, 1], keep[:, 2]])
    j = np.concatenate([keep[:, 1], keep[:, 2], keep[:, 0]])
    return int(np.unique(np.minimum(i, j) * V + np.maximum(i, j), return_counts=True)[1].max())


def raw_entries(tris, V):
    """Per vertex, twice the number of kept triangles that name it."""
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    keep = tris[(tris[:, 0] != tris[:, 1]) & (tris[:, 1] != tris[:, 2]) & (tris[:, 0] != tris[:, 2])]
    return 2 * np.bincount(keep.reshape(-1), minlength=V)


def step(p, offsets, ring, moves, f):
    """One Jacobi step with factor f on (V, 3) float32 positions."""
    f = np.float32(f)
    n = (offsets[1:] - offsets[:-1]).astype(np.int64)
    act = np.nonzero(moves & (n > 0))[0]
    s = p[ring[offsets[act]]].astype(np.float32)
    k = 1
    live = act
    rows = np.arange(len(act))
    while True:
        more = n[live] > k
        if not more.any():
            break
        live, rows = live[more], rows[more]
        s[rows] = (s[rows] + p[ring[offsets[live] + k]]).astype(np.float32)
        k += 1
    m = (s / n[act].astype(np.float32)[:, None]).astype(np.float32)
    d = (m - p[act]).astype(np.float32)
    out = p.copy()
    out[act] = (p[act] + (f * d).astype(np.float32)).astype(np.float32)
    return out


def smooth(verts, tris, iterations=10, lam=LAM, mu=MU, boundary="fixed", rings_=None):
    verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    offsets, ring, bnd = rings_ if rings_ is not None else rings(tris, len(verts))
    moves = ~bnd if boundary == "fixed" else np.ones(len(verts), bool)
    p = verts.copy()
    with np.errstate(all="ignore"):
        for _ in range(int(iterations)):
            p = step(p, offsets, ring, moves, lam)
            if mu is not None:
                p = step(p, offsets, ring, moves, mu)
    return p


# ---------------------------------------------------------------- the meshes of both test files
def hand_meshes():
    """name -> (verts (V, 3) float32, tris): at most 12 triangles each."""
    i = lambda rows: np.array(rows, np.int64).reshape(-1, 3)
    rng = np.random.default_rng(11)
    pos = lambda V: (rng.uniform(-1, 1, (V, 3)) * 3).astype(np.float32)
    out = {}
    out["tetrahedron"] = (pos(4), i([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]]))
    out["octahedron"] = (pos(6), i([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]]))
    out["one_triangle"] = (pos(3), i([[0, 1, 2]]))
    out["two_on_an_edge"] = (pos(4), i([[0, 1, 2], [2, 1, 3]]))
    out["three_on_an_edge"] = (pos(5), i([[0, 1, 2], [1, 0, 3], [0, 1, 4]]))
    out["same_twice"] = (pos(4), i([[0, 1, 2], [0, 1, 2], [2, 1, 3]]))
    out["both_windings"] = (pos(4), i([[0, 1, 2], [2, 1, 0], [2, 1, 3]]))
    out["repeated_index"] = (pos(5), i([[0, 1, 2], [3, 3, 4], [1, 4, 1], [2, 2, 2], [2, 1, 3]]))
    out["lonely_vertex"] = (pos(6), i([[0, 1, 2], [2, 1, 4]]))                        # 3 and 5 are in no triangle
    # a closed fan around vertex 0 over a rim 1 .. 6, then the rim closed by a second apex: twelve triangles, no boundary
    rim = [1, 2, 3, 4, 5, 6]
    out["twelve"] = (pos(8), i([[0, rim[k], rim[(k + 1) % 6]] for k in range(6)] + [[7, rim[(k + 1) % 6], rim[k]] for k in range(6)]))
    return out


def hub(n):
    """A disc of n triangles around vertex 0 over a rim of n vertices: vertex 0 is in n triangles."""
    r = np.arange(n, dtype=np.int64)
    tris = np.stack([np.zeros(n, np.int64), 1 + r, 1 + (r + 1) % n], 1)
    ang = 2 * np.pi * np.arange(n) / n
    verts = np.concatenate([[[0.0, 0.0, 0.7]], np.stack([np.cos(ang), np.sin(ang), 0.1 * np.sin(7 * ang)], 1)]).astype(np.float32)
    return verts, tris


sphere, sheet, fan = S.sphere, S.sheet, S.fan


@functools.lru_cache(maxsize=None)
def expected_rings(name):
    """The oracle's rings of a named fixture, computed once and shared (leave them unchanged)."""
    verts, tris = {"sphere": sphere, "sheet": sheet, "fan": fan}[name]()
    return rings(tris, len(verts))


@functools.lru_cache(maxsize=None)
def expected_smooth(name, iterations, boundary="fixed", mu=MU):
    verts, tris = {"sphere": sphere, "sheet": sheet, "fan": fan}[name]()
    return smooth(verts, tris, iterations, LAM, mu, boundary, rings_=expected_rings(name))
