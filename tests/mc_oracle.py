"""TEST INFRASTRUCTURE ONLY -- numpy restatement of the device marching cubes' exact contract (mf_mesh.hip,
include/mocoflow_hip.h mf_mc_*), on the committed case table (moco_flow_amd/csrc/mf_mc_tables.hpp).

  classification   corner below  <=>  v < iso  (NaN is not below); clamp_zero reads v < 0 ? 0 : v
  vertices         one per crossing lattice edge (p, axis), sorted by edge id 3 p + axis (p = C-order point index);
                   t = (iso - f(p)) / (f(p + e) - f(p)) in fp32, position = p + t e_axis in index coordinates (fp32)
  triangles        sorted by the C-order index of their cell, within a cell in table order; raw table winding

Everything is float32 arithmetic with one rounding per operation, as the kernel computes it."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE_PATH = os.path.join(ROOT, "moco_flow_amd", "csrc", "mf_mc_tables.hpp")


def load_table(path=TABLE_PATH):
    """(ntri (256,) int64, edges (256, 15) int64 with -1 pads) parsed from the committed header."""
    text = open(path).read()
    body = lambda name: text.split(name, 1)[1].split("};", 1)[0].split("=", 1)[1]
    ntri = np.array([int(x) for x in re.findall(r"-?\d+", re.sub(r"//[^\n]*", "", body("kNumTri[256]")))], np.int64)
    edges = np.array([int(x) for x in re.findall(r"-?\d+", re.sub(r"//[^\n]*", "", body("kTriEdges[256]")).split("{", 1)[1])],
                     np.int64)
    return ntri, edges.reshape(256, 15)


NTRI, EDGES = load_table()


def edge_offset(e):
    """(axis, offset of the edge's first corner (o0, o1, o2)) of cube edge e."""
    a, u, v = e >> 2, (e >> 1) & 1, e & 1
    o = [0, 0, 0]
    others = [i for i in range(3) if i != a]
    o[others[0]], o[others[1]] = u, v
    return a, tuple(o)


EDGE_OFF = np.array([edge_offset(e)[1] for e in range(12)], np.int64)     # (12, 3): first corner of each cube edge


def _prep(vol, iso, clamp_zero):
    f = np.ascontiguousarray(vol, dtype=np.float32)
    if clamp_zero:
        f = np.where(f < 0, np.float32(0), f)
    return f, f < np.float32(iso)


def _crossings(below):
    """cross (n0, n1, n2, 3) bool: lattice edge (p, axis) exists and crosses."""
    cross = np.zeros(below.shape + (3,), bool)
    cross[:-1, :, :, 0] = below[:-1] != below[1:]
    cross[:, :-1, :, 1] = below[:, :-1] != below[:, 1:]
    cross[:, :, :-1, 2] = below[:, :, :-1] != below[:, :, 1:]
    return cross


def _cases(below):
    n0, n1, n2 = below.shape
    case = np.zeros((n0 - 1, n1 - 1, n2 - 1), np.int64)
    for c in range(8):
        o0, o1, o2 = (c >> 2) & 1, (c >> 1) & 1, c & 1
        case |= below[o0:n0 - 1 + o0, o1:n1 - 1 + o1, o2:n2 - 1 + o2].astype(np.int64) << c
    return case


def marching_cubes(vol, iso, clamp_zero=False, row0=0):
    """(verts (V, 3) float32, tris (T, 3) int64) of the contract above.  row0: axis-0 index of vol's first row when vol is a
    slab of a larger volume (positions are then those of the larger volume)."""
    f, below = _prep(vol, iso, clamp_zero)
    n0, n1, n2 = f.shape
    cross = _crossings(below)
    flat = cross.reshape(-1)
    vid = np.cumsum(flat, dtype=np.int64) - 1                     # vertex index of edge id 3 p + a (valid where it crosses)
    eid = np.flatnonzero(flat)
    p, a = eid // 3, eid % 3
    strides = np.array([n1 * n2, n2, 1], np.int64)
    ff = f.reshape(-1)
    f0, f1 = ff[p], ff[p + strides[a]]
    t = (np.float32(iso) - f0) / (f1 - f0)
    idx = np.stack(np.unravel_index(p, f.shape), -1)
    idx[:, 0] += row0
    idx = idx.astype(np.float32)
    idx[np.arange(len(p)), a] = idx[np.arange(len(p)), a] + t
    verts = idx

    cshape = (n0 - 1, n1 - 1, n2 - 1)
    case = _cases(below).reshape(-1)
    nt = NTRI[case]
    cell = np.repeat(np.arange(case.size, dtype=np.int64), nt)      # cells in C order, each once per triangle
    slot = np.arange(cell.size, dtype=np.int64) - np.repeat(np.cumsum(nt) - nt, nt)
    ci, cj, ck = np.unravel_index(cell, cshape)
    base = (ci * n1 + cj) * n2 + ck                                 # the cell's first corner as a lattice point
    tris = np.empty((cell.size, 3), np.int64)
    for k in range(3):
        e = EDGES[case[cell], 3 * slot + k]
        tris[:, k] = vid[3 * (base + EDGE_OFF[e] @ strides) + (e >> 2)]
    return verts, tris


def counts(vol, iso, clamp_zero=False, rows=None, chunk=32):
    """(V, T) of marching_cubes(vol, iso, clamp_zero) restricted to lattice points / cells whose axis-0 index lies in
    rows = (r0, r1) (default: all), computed chunk by chunk along axis 0 (for volumes too large for marching_cubes)."""
    n0 = vol.shape[0]
    r0, r1 = rows if rows is not None else (0, n0)
    V = T = 0
    for s in range(r0, r1, chunk):
        e = min(s + chunk, r1)
        f, below = _prep(vol[s:min(e + 1, n0)], iso, clamp_zero)
        cross = _crossings(below)[:e - s]
        V += int(cross.sum())
        if below.shape[0] > 1:
            T += int(NTRI[_cases(below)[:e - s]].sum())
    return V, T


def slab(vol, iso, r0, r1, clamp_zero=False):
    """The part of marching_cubes(vol, iso, clamp_zero) that lattice points / cells in rows [r0, r1) of axis 0 own
    (r1 + 2 <= n0): (verts, tris, index of the first of those vertices, of the first of those triangles); vertex indices
    global.  Rows r1, r1 + 1 come along so that the vertices the slab's last cells use are complete and in global order."""
    V0, T0 = counts(vol, iso, clamp_zero, rows=(0, r0))
    verts, tris = marching_cubes(vol[r0:r1 + 2], iso, clamp_zero, row0=r0)
    Vs, Ts = counts(vol, iso, clamp_zero, rows=(r0, r1))
    return verts[:Vs], tris[:Ts] + V0, V0, T0


def same_mesh_as_sets(verts_a, tris_a, verts_b, tris_b, tol=1e-5):
    """Whether two meshes are equal as sets: a bijection of vertices within `tol` (max-abs, index units), and the same
    triangles as vertex triples up to cyclic rotation (which keeps the winding).  Returns (ok, message)."""
    from scipy.spatial import cKDTree
    va, vb = np.asarray(verts_a, np.float64), np.asarray(verts_b, np.float64)
    if va.shape != vb.shape or np.shape(tris_a) != np.shape(tris_b):
        return False, f"shapes differ: V {va.shape} vs {vb.shape}, T {np.shape(tris_a)} vs {np.shape(tris_b)}"
    if len(va) == 0:
        return True, "empty"
    dist, match = cKDTree(vb).query(va, p=np.inf)
    if dist.max() > tol:
        return False, f"vertex {int(dist.argmax())} has no partner within {tol} (nearest {dist.max():.3g})"
    if len(np.unique(match)) != len(match):
        return False, "vertex matching is not a bijection"

    def canon(t):
        t = np.asarray(t, np.int64)
        r = np.argmin(t, 1)
        t = np.stack([t[np.arange(len(t)), (r + k) % 3] for k in range(3)], 1)
        return t[np.lexsort(t.T[::-1])]
    ta, tb = canon(match[np.asarray(tris_a, np.int64)]), canon(tris_b)
    if not np.array_equal(ta, tb):
        return False, f"triangle sets differ ({int((ta != tb).any(1).sum())} of {len(ta)} rows after sorting)"
    return True, "equal"


def all_cases_volume(seed=0):
    """(2, 2, 512) volume whose cells k = 2 c (c = 0..255) are case c, values +-[0.1, 1] (no value equals 0): with
    isovalue 0 every table entry is exercised (the odd cells between them get whatever case their corners make)."""
    rng = np.random.default_rng(seed)
    vol = np.empty((2, 2, 512), np.float32)
    for c in range(256):
        for corner in range(8):
            o0, o1, o2 = (corner >> 2) & 1, (corner >> 1) & 1, corner & 1
            mag = rng.uniform(0.1, 1.0)
            vol[o0, o1, 2 * c + o2] = -mag if (c >> corner) & 1 else mag
    return vol
