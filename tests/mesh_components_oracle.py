"""Numpy oracle of the mesh clean-up contract (include/mocoflow_hip.h mf_mesh_*; moco_flow_amd.mesh.mesh_components /
filter_components): a serial union-find, the component table, the ranking and the filter, as plainly as they can be said.

tris (T, 3) int64 over V vertices.  Two vertices are adjacent if some triangle names both; the label of a vertex is the
smallest vertex index of its connected component (a vertex in no triangle is a component of its own, with no triangles);
a triangle belongs to the component of its column-0 vertex; components rank by triangle count (descending), then label
(ascending); a filter keeps whole components and leaves kept vertices and triangles in their original order."""
import numpy as np


def labels(tris, V):
    """(V,) int64: the smallest vertex index of each vertex's component."""
    parent = list(range(V))

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    for a, b, c in np.asarray(tris, np.int64).reshape(-1, 3).tolist():
        for u, v in ((a, b), (b, c)):
            ru, rv = find(u), find(v)
            if ru < rv:
                parent[rv] = ru
            elif rv < ru:
                parent[ru] = rv
    return np.array([find(v) for v in range(V)], np.int64).reshape(V)


def table(tris, lab):
    """(ids, tri_counts, vert_counts), each (C,) int64, ids ascending."""
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    V = len(lab)
    ids = np.flatnonzero(lab == np.arange(V)).astype(np.int64)
    tri_counts = np.bincount(lab[tris[:, 0]], minlength=V)[ids].astype(np.int64) if V else np.zeros(0, np.int64)
    vert_counts = np.bincount(lab, minlength=V)[ids].astype(np.int64) if V else np.zeros(0, np.int64)
    return ids, tri_counts, vert_counts


def components(tris, V):
    lab = labels(tris, V)
    return (lab,) + table(tris, lab)


def pattern_mesh(pattern):
    """(tris, V) of the mesh a pattern spells: component c owns the vertices v with pattern[v] == c (at least three) and is a
    strip over them in ascending order; the rows are in the order of their column-0 vertex.  In element order the vertices'
    labels are the pattern itself and the triangles' are the pattern without the last two vertices of every component."""
    pattern = np.asarray(pattern, np.int64)
    rows = []
    for c in np.unique(pattern):
        v = np.flatnonzero(pattern == c)
        assert len(v) >= 3, c
        rows.append(np.stack([v[:-2], v[1:-1], v[2:]], 1))
    tris = np.concatenate(rows)
    return tris[np.argsort(tris[:, 0], kind="stable")], len(pattern)


BRANCHES = ("carry_add", "take_flush", "take_empty", "leader_add_holding")


def wave_count_replay(keys, threads, max_blocks):
    """The decisions of wave_count (csrc/mf_mesh_components.hip) for ``keys`` in element order -- the labels of the
    triangles' column-0 vertices, or of the vertices -- under a grid of min(ceil(N / threads), max_blocks) workgroups of
    ``threads`` threads in waves of 64: a wave holds one (key, count) pair across the trips of its grid-stride loop, and per
    trip visits its distinct keys in the order of their first lane.  Returns (adds, later): ``adds[k]`` the sum of everything
    added to counter k, the final flush included; ``later[b]`` how often branch b of BRANCHES was taken on a trip after the
    first: the held key seen again (its count goes to the pair), a new majority taking a non-empty pair (which is flushed),
    a key taking an empty pair, and a minority key added by its leader while another key is held."""
    keys = np.asarray(keys, np.int64).reshape(-1).tolist()
    N = len(keys)
    blocks = min(-(-N // threads), max_blocks)
    adds, later = {}, dict.fromkeys(BRANCHES, 0)

    def add(k, c):
        adds[k] = adds.get(k, 0) + c

    for first in range(0, blocks * threads, 64):                    # the wave's first element on its first trip
        held, n = 0, 0
        for trip, start in enumerate(range(first, N, blocks * threads)):
            seen = {}                                               # insertion order: the order of the leaders
            for k in keys[start:start + 64]:
                seen[k] = seen.get(k, 0) + 1
            for k, c in seen.items():
                if n and k == held:
                    n += c
                    branch = "carry_add"
                elif c > 32 or not n:
                    branch = "take_flush" if n else "take_empty"
                    if n:
                        add(held, n)
                    held, n = k, c
                else:
                    add(k, c)
                    branch = "leader_add_holding"
                later[branch] += trip > 0
        if n:
            add(held, n)
    return adds, later


def ranking(ids, tri_counts):
    """Positions into the table in rank order: triangle count descending, then label ascending."""
    return np.lexsort((ids, -tri_counts))


def keep_mask(ids, tri_counts, keep_largest=None, min_triangles=None):
    """(C,) bool: the per-component decision of filter_components."""
    if keep_largest is None and min_triangles is None:
        raise ValueError("give keep_largest, min_triangles or both")
    if keep_largest is not None and keep_largest < 1:
        raise ValueError("keep_largest < 1")
    keep = np.ones(len(ids), bool)
    if keep_largest is not None:
        keep[:] = False
        keep[ranking(ids, tri_counts)[:keep_largest]] = True
    if min_triangles is not None:
        keep &= tri_counts >= min_triangles
    return keep


def filter_components(verts, tris, keep_largest=None, min_triangles=None, attrs=(), comps=None):
    """(verts, tris, *attrs) of the kept components: rows copied in their original order, indices rewritten.  ``comps``:
    components(tris, len(verts)) where a caller has it already."""
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    V = len(verts)
    lab, ids, tri_counts, _ = components(tris, V) if comps is None else comps
    keep = keep_mask(ids, tri_counts, keep_largest, min_triangles)
    keep_root = np.zeros(V, bool)
    keep_root[ids[keep]] = True
    vkeep = keep_root[lab]
    tkeep = vkeep[tris[:, 0]]
    remap = np.cumsum(vkeep) - 1
    return (verts[vkeep], remap[tris[tkeep]].astype(np.int64).reshape(-1, 3)) + tuple(a[vkeep] for a in attrs)
