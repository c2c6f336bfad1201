"""TEST INFRASTRUCTURE ONLY -- numpy restatement of mf_mc_normals (mf_mesh.hip, include/mocoflow_hip.h) and a reader for the
files export_ply writes.

  v                vol, or vol < 0 ? 0 : vol with clamp_zero
  lattice gradient per axis (v(q + e_k) - v(q - e_k)) / 2; on a border face the one-sided difference
  vertex p         i_k = min(floor(p_k), n_k - 1) (0 for p_k < 0 or NaN), t_k = p_k - i_k; a = axis of the largest t_k (ties:
                   the lowest), t = t_a; g(p) = (1 - t) g(i) + t g(i + e_a), g(i) when t is 0
  normal           -g / ||g||; the zero vector where ||g|| is 0 or g is not finite

``dtype=np.float32``: every operation rounds to fp32 once, in the kernel's order; ``np.float64``: the same formulas on the
fp32 inputs in double precision (the yardstick of the fp32 evaluation's own error)."""
import numpy as np


def lattice_gradient(v, q):
    """v (n0, n1, n2), q (V, 3) int lattice points -> (V, 3) gradient in v's dtype."""
    n = np.array(v.shape)
    g = np.empty((len(q), 3), v.dtype)
    half = v.dtype.type(0.5)
    for a in range(3):
        lo, hi = q.copy(), q.copy()
        lo[:, a] = np.maximum(q[:, a] - 1, 0)
        hi[:, a] = np.minimum(q[:, a] + 1, n[a] - 1)
        d = v[hi[:, 0], hi[:, 1], hi[:, 2]] - v[lo[:, 0], lo[:, 1], lo[:, 2]]
        g[:, a] = np.where(hi[:, a] - lo[:, a] == 2, d * half, d)
    return g


def gradient_at(vol, verts, clamp_zero=False, dtype=np.float32):
    """The interpolated gradient g(p) (V, 3) of the contract above, before normalisation."""
    with np.errstate(all="ignore"):
        v = np.asarray(vol, np.float32)
        if clamp_zero:
            v = np.where(v < 0, np.float32(0), v)
        v = v.astype(dtype)
        p = np.asarray(verts, np.float32).reshape(-1, 3)
        n = np.array(v.shape)
        cell = np.where(p >= 0, np.minimum(np.floor(p), (n - 1).astype(np.float32)), np.float32(0)).astype(np.int64)
        t3 = p.astype(dtype) - cell.astype(dtype)
        a = np.zeros(len(p), np.int64)
        t = t3[:, 0].copy()
        for k in (1, 2):
            up = t3[:, k] > t
            a[up] = k
            t[up] = t3[up, k]
        g = lattice_gradient(v, cell)
        far = cell.copy()
        rows = np.arange(len(p))
        far[rows, a] = np.minimum(cell[rows, a] + 1, n[a] - 1)
        h = lattice_gradient(v, far)
        one = dtype(1)
        mixed = (one - t)[:, None] * g + t[:, None] * h
        return np.where((t > 0)[:, None], mixed, g)


def normals(vol, verts, clamp_zero=False, dtype=np.float32):
    """(V, 3) normals in ``dtype``."""
    with np.errstate(all="ignore"):
        g = gradient_at(vol, verts, clamp_zero, dtype)
        len2 = g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1] + g[:, 2] * g[:, 2]
        ok = (len2 > 0) & (len2 < np.inf)
        inv = dtype(1) / np.sqrt(np.where(ok, len2, dtype(1)))
        return np.where(ok[:, None], -(g * inv[:, None]), dtype(0)).astype(dtype)


def read_ply(path):
    """(header lines, vertex record array, faces (T, 3) int32) of a binary little-endian PLY with float / uchar vertex
    properties and one ``list uchar int`` face property of triangles."""
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    kinds = {"float": "<f4", "uchar": "u1"}
    counts, fields, element = {}, [], None
    for ln in lines[2:-1]:
        w = ln.split()
        if w[0] == "element":
            element = w[1]
            counts[element] = int(w[2])
        elif w[0] == "property" and element == "vertex":
            fields.append((w[2], kinds[w[1]]))
        elif w[0] == "property":
            assert element == "face" and w[1:] == ["list", "uchar", "int", "vertex_indices"], ln
    vdt = np.dtype(fields)
    fdt = np.dtype([("n", "u1"), ("i", "<i4", (3,))])
    V, T = counts["vertex"], counts["face"]
    assert len(data) == end + V * vdt.itemsize + T * fdt.itemsize
    verts = np.frombuffer(data, vdt, V, end)
    faces = np.frombuffer(data, fdt, T, end + V * vdt.itemsize)
    assert np.all(faces["n"] == 3)
    return lines, verts, faces["i"]
