"""CPU-side checks (-m "not gpu") of the mesh-to-grid path (csrc/mf_voxelize.hip; OccupancyGrid.from_mesh, from_smpl, filled,
dilated): the numpy oracle of its contracts (tests/voxelize_oracle.py) against independent statements -- the surface predicate
against an exact clip of the triangle by the cell in fractions.Fraction and against the kernel's own formulation in Python ints,
the fill against scipy.ndimage.binary_fill_holes, the dilation against its definition --; the guarantees (a) and (b) of
from_mesh's docstring as properties of the oracle; the overflow bound of the integer arithmetic at the saturation corners; the
library's exports, ABI version and ctypes prototypes; every refusal that is made before a launch.  None of it touches a GPU."""
import ctypes as C
import itertools
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import voxelize_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW_SYMBOLS = ("mf_voxel_mesh", "mf_voxel_fill_scratch_bytes", "mf_voxel_fill", "mf_voxel_dilate_scratch_bytes", "mf_voxel_dilate")
DIMS = (4, 5, 6)


# ---- the surface predicate -------------------------------------------------------------------------------------------------------

def clip_meets(q, cell):
    """The closed triangle q (three corners of three ints, in sub-cell units) meets the closed cell: Sutherland-Hodgman against
    the six half-spaces, exact in Fractions; a closed half-space keeps what touches it."""
    poly = [tuple(Fraction(int(x)) for x in c) for c in q]
    for a in range(3):
        for bound, keep_above in ((int(cell[a]) * O.SUB, True), (int(cell[a]) * O.SUB + O.SUB, False)):
            inside = (lambda p: p[a] >= bound) if keep_above else (lambda p: p[a] <= bound)
            out = []
            for i, p in enumerate(poly):
                r = poly[(i + 1) % len(poly)]
                if inside(p):
                    out.append(p)
                if inside(p) != inside(r):
                    t = (bound - p[a]) / (r[a] - p[a])
                    out.append(tuple(p[c] + t * (r[c] - p[c]) for c in range(3)))
            poly = out
            if not poly:
                return False
    return True


def random_triangles(n, seed):
    """Corners in sub-cell units around the 4 x 5 x 6 grid: many on cell faces, edges and corners, some outside, some without
    area (a repeated corner, three collinear corners)."""
    rng = np.random.default_rng(seed)
    top = np.asarray(DIMS) * O.SUB
    tris = []
    for k in range(n):
        step = (1, 16, 32, 64)[k % 4]                                          # coarser steps land on cell boundaries
        base = rng.integers(-O.SUB, top + O.SUB, size=3)
        q = base + rng.integers(-2 * O.SUB, 2 * O.SUB + 1, size=(3, 3))
        q = (q // step) * step
        if k % 16 == 5:
            q[2] = q[0]                                                        # no area
        if k % 16 == 9:
            q[2] = 2 * q[1] - q[0]                                             # collinear
        if k % 16 == 13:
            q[:, rng.integers(3)] = rng.integers(0, DIMS[0]) * O.SUB           # lies in a cell face
        if k % 32 == 7:
            q += top + 3 * O.SUB                                               # wholly outside
        tris.append(q)
    return np.asarray(tris, dtype=np.int64)


def test_surface_predicate_equals_an_exact_clip_and_the_kernels_formulation():
    tris = random_triangles(320, 11)
    cells = np.asarray(list(itertools.product(*[range(g) for g in DIMS])), dtype=np.int64)
    expect = np.zeros(DIMS, dtype=bool)
    n_degenerate = n_outside = n_touch = 0
    for q in tris:
        sat = O.sat_meets(np.broadcast_to(q, (len(cells), 3, 3)), cells)
        degenerate = not np.cross(q[1] - q[0], q[2] - q[1]).any()
        n_degenerate += degenerate
        n_outside += (not degenerate) and not sat.any()
        for c, s in zip(cells, sat):
            ss = O.schwarz_seidel(q, c)
            if degenerate:
                assert ss is None
                continue
            assert ss == bool(s), (q.tolist(), c.tolist())                     # the two formulations decide one predicate
            lo, hi = c * O.SUB, c * O.SUB + O.SUB
            if (q.max(0) < lo - O.SUB).any() or (q.min(0) > hi + O.SUB).any():
                assert not s                                                   # a cell away from the bounding box: no clip needed
                continue
            want = clip_meets(q, c)
            assert want == bool(s), (q.tolist(), c.tolist())
            n_touch += want and ((q.max(0) == lo) | (q.min(0) == hi)).any()
            expect[tuple(c)] |= want
    assert n_degenerate >= 30 and n_outside >= 10 and n_touch >= 10            # the draw holds the cases it is meant to hold
    # the whole mesh through surface(): corners q / 64 in a box whose cells are unit cubes snap back to q exactly
    verts = (tris.reshape(-1, 3) / float(O.SUB)).astype(np.float32)
    assert np.array_equal(verts.astype(np.float64) * O.SUB, tris.reshape(-1, 3))
    dense, dropped = O.surface(verts, np.arange(len(verts)).reshape(-1, 3), DIMS, (0, 0, 0), DIMS)
    assert dropped == n_degenerate and np.array_equal(dense, expect)


def test_faces_corners_and_skipped_triangles():
    lo, hi = (0, 0, 0), DIMS
    face = np.array([[1.0, 1.25, 1.25], [1.0, 1.75, 1.25], [1.0, 1.25, 1.75]], np.float32)     # in the face x = 1 of cell (1, 1, 1)
    dense, dropped = O.surface(face, [[0, 1, 2]], DIMS, lo, hi)
    assert dropped == 0 and sorted(map(tuple, np.argwhere(dense))) == [(0, 1, 1), (1, 1, 1)]
    corner = np.array([[2.0, 2.0, 2.0], [2.25, 2.0, 2.0], [2.0, 2.25, 2.0]], np.float32)       # a corner on a cell corner
    dense, _ = O.surface(corner, [[0, 1, 2]], DIMS, lo, hi)
    assert dense[1:3, 1:3, 1:3].all() and dense.sum() == 8
    verts = np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [np.nan, 0, 0], [np.inf, 0, 0], [0.5, 0.5, 0.5 + 1e-4]], np.float32)
    tris = [[0, 1, 2], [0, 1, -1], [0, 1, 6], [0, 1, 3], [0, 4, 1], [0, 0, 1], [0, 5, 1]]    # the last: no area once snapped
    dense, dropped = O.surface(verts, tris, DIMS, lo, hi)
    assert dropped == 6 and np.array_equal(dense, O.surface(verts, tris[:1], DIMS, lo, hi)[0])
    assert O.surface(verts, np.zeros((0, 3), np.int64), DIMS, lo, hi)[1] == 0
    dense, dropped = O.surface(np.zeros((0, 3), np.float32), tris, DIMS, lo, hi)                # no vertex: every index is outside
    assert dropped == 7 and not dense.any()


def test_snapping_saturates_and_rounds_to_even():
    lo, hi, inv = O.grid_constants((4, 4, 4), (0, 0, 0), (4, 4, 4))
    v = np.array([[0.5 / 64, 1.5 / 64, 2.5 / 64], [-2000.0, 3000.0, 1e30], [-1e30, 2048.0, -1024.0], [3.4e38, -3.4e38, 0.0]], np.float32)
    q, finite = O.snap(v, lo, inv)
    assert finite.all() and q.tolist() == [[0, 2, 2], [-65536, 131072, 131072], [-65536, 131072, -65536], [131072, -65536, 0]]
    assert O.snap(np.array([[np.nan, 0, 0], [0, np.inf, 0]], np.float32), lo, inv)[1].tolist() == [False, False]


# ---- the overflow bound ----------------------------------------------------------------------------------------------------------

def test_overflow_bound_at_the_saturation_corners():
    """Corners at the ends of the snapped range against cells at the ends of the largest grid: every value the kernel holds in an
    int64 stays below 2^57 (edges below 2^18, normal components below 2^37), so int64 arithmetic wraps nowhere -- run in Python
    ints, and the same sums run in numpy int64 give the same numbers."""
    ends = (O.SNAP_LO, O.SNAP_HI)
    corners = list(itertools.product(ends, repeat=3))
    cells = list(itertools.product((0, O.MAX_SIDE - 1), repeat=3))
    worst = 0
    rng = np.random.default_rng(3)
    picks = [tuple(rng.integers(len(corners), size=3)) for _ in range(160)] + [(0, 7, 3), (7, 0, 5), (1, 6, 2), (6, 1, 4)]
    for a, b, c in picks:
        q = [corners[a], corners[b], corners[c]]
        e = np.asarray(q, dtype=np.int64)
        n64 = np.cross(e[1] - e[0], e[2] - e[1])                              # int64, as the kernel computes it
        for cell in cells:
            terms = []
            got = O.schwarz_seidel(q, cell, terms)
            worst = max(worst, max(abs(t) for t in terms))
            if got is None:
                assert not n64.any()
                continue
            n = [int(x) for x in n64]
            assert all(abs(x) < 1 << 37 for x in n) and n == terms[9:12]
            pc = np.asarray(cell, dtype=np.int64) * O.SUB
            with np.errstate(over="raise"):
                t64 = int((n64 * (pc - e[0])).sum())                          # the plane test against the box's min corner, in int64
            assert t64 == sum(n[k] * (int(pc[k]) - q[0][k]) for k in range(3)) and abs(t64) < 1 << 57
            assert got == bool(O.sat_meets(e[None], np.asarray([cell]))[0])
    assert 1 << 50 < worst < 1 << 57                                          # the bound is nearly reached, and holds
    assert max(abs(a - b) for a in ends for b in ends) < 1 << 18


# ---- fill and dilation -----------------------------------------------------------------------------------------------------------

def _shell(dims, lo, hi, mesh):
    return O.surface(mesh[0], mesh[1], dims, lo, hi)[0]


def test_fill_equals_scipy_binary_fill_holes():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(5)
    cases = [rng.random((7, 9, 11)) < p for p in (0.2, 0.45, 0.6, 0.8)]
    cases += [np.zeros((3, 4, 5), bool), np.ones((3, 4, 5), bool), np.zeros((1, 1, 1), bool), rng.random((1, 6, 7)) < 0.5]
    lo, hi = (-1, -1, -1), (1, 1, 1)
    cases.append(_shell((12, 12, 12), lo, hi, O.icosphere(1, radius=0.7)))
    cases.append(_shell((24, 24, 12), lo, hi, O.torus(0.6, 0.3)))
    cases.append(_shell((14, 14, 14), lo, hi, O.nested_spheres(1, (0, 0, 0), 0.8, 0.35)))
    cases.append(_shell((12, 12, 12), lo, hi, O.hemisphere(1, radius=0.7)))
    for dense in cases:
        assert np.array_equal(O.fill(dense), ndimage.binary_fill_holes(dense)), dense.shape
    sphere, torus, nested, hemi = cases[-4:]
    assert O.fill(sphere)[6, 6, 6] and not sphere[6, 6, 6]
    assert not O.fill(torus)[12, 12, 6] and O.fill(torus).sum() > torus.sum()     # the tube is filled, the hole is not
    assert O.fill(nested)[3:11, 3:11, 3:11].all()                             # filled through the inner shell
    assert np.array_equal(O.fill(hemi), hemi)                                 # open: leaks


def test_dilation_equals_its_definition():
    rng = np.random.default_rng(7)
    dense = rng.random((5, 6, 40)) < 0.03
    for radii in ((0, 0, 0), (1, 2, 3), (0, 0, 33), (2, 0, 0), (9, 9, 90)):
        want = np.zeros_like(dense)
        for i, j, k in np.argwhere(dense):
            want[max(i - radii[0], 0):i + radii[0] + 1, max(j - radii[1], 0):j + radii[1] + 1, max(k - radii[2], 0):k + radii[2] + 1] = True
        assert np.array_equal(O.dilate(dense, radii), want), radii
    words = O.pack(dense)
    assert words.shape == (5, 6, 2) and not (words[:, :, 1] >> 8).any() and np.array_equal(O.unpack(words, 40), dense)


# ---- the guarantees of from_mesh's docstring -----------------------------------------------------------------------------------

def test_guarantee_a_points_within_thickness_of_a_vertex_fall_in_set_cells():
    """The reference's label (datasets/moco_flow_dataset.py:87-142): inside iff within `thickness` of a vertex."""
    rng = np.random.default_rng(13)
    lo, hi, dims, thickness = (-1.3, -0.9, -1.1), (1.2, 1.0, 1.4), (24, 18, 31), 0.2
    verts, tris = O.icosphere(2, center=(0.05, -0.02, 0.1), radius=0.55)
    dense, dropped = O.from_mesh(verts, tris, dims, lo, hi, dilate_cells=1, thickness=thickness, solid=True)
    assert dropped == 0
    lo32, hi32, inv = O.grid_constants(dims, lo, hi)
    d = rng.normal(size=(40000, 3))
    d *= (thickness * rng.random((len(d), 1)) ** (1 / 3)) / np.linalg.norm(d, axis=1, keepdims=True)
    pts = (verts[rng.integers(len(verts), size=len(d))].astype(np.float64) + d).astype(np.float32)
    pts = pts[((pts >= lo32) & (pts <= hi32)).all(1)]
    assert len(pts) > 30000
    c = O.cell_of(pts, lo32, inv, dims)
    assert dense[c[:, 0], c[:, 1], c[:, 2]].all()
    assert O.radii(dims, lo, hi, 1, thickness) == tuple(1 + int(np.ceil(thickness * dims[a] / (np.float64(hi32[a]) - np.float64(lo32[a])))) for a in range(3))
    assert not dense.all()


def test_guarantee_b_the_true_surface_lies_within_a_128th_cell_and_dilate_1_covers_it():
    rng = np.random.default_rng(17)
    lo, hi, dims = (-0.93, -0.51, -1.07), (0.81, 0.62, 1.03), (13, 9, 21)
    lo32, hi32, inv = O.grid_constants(dims, lo, hi)
    verts, tris = O.icosphere(2, center=(-0.05, 0.03, 0.0), radius=0.4)
    q, finite = O.snap(verts, lo32, inv)
    u = (verts.astype(np.float64) - lo32.astype(np.float64)) * dims / (hi32.astype(np.float64) - lo32.astype(np.float64))
    assert finite.all() and np.abs(q / float(O.SUB) - u).max() <= 1 / 128 + 1e-5
    dense, _ = O.from_mesh(verts, tris, dims, lo, hi, dilate_cells=1, thickness=0.0, solid=False)
    w = rng.dirichlet((1, 1, 1), size=30000)
    t = tris[rng.integers(len(tris), size=len(w))]
    pts = (verts[t].astype(np.float64) * w[:, :, None]).sum(1).astype(np.float32)
    c = O.cell_of(pts, lo32, inv, dims)
    assert dense[c[:, 0], c[:, 1], c[:, 2]].all()


# ---- the library ---------------------------------------------------------------------------------------------------------------

def test_library_exports_header_symbols_and_prototypes():
    import moco_flow_amd as M
    import moco_flow_amd._lib as L
    header = open(os.path.join(ROOT, "include", "mocoflow_hip.h")).read()
    declared = set(re.findall(r"^int(?:32|64)_t (mf_\w+)\(", header, re.M))
    lib = L.lib()
    assert lib.mf_version() == 16 and L.MF_ABI_VERSION == 16
    assert "#define MF_ABI_VERSION 16" in header
    additive = header[header.index("additive entries since, version unchanged"):header.index("#define MF_ABI_VERSION")]
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in additive, name
        fn = getattr(lib, name)
        assert fn.restype is L.SYMBOLS[name][0] and list(fn.argtypes) == L.SYMBOLS[name][1]
    assert {n for n in declared if n.startswith("mf_voxel_")} == set(NEW_SYMBOLS)
    for entry in ("mf_voxel_mesh (serves", "mf_voxel_fill (serves", "mf_voxel_dilate (serves"):
        doc = header[header.index(entry):]
        doc = doc[:doc.index("*/")]
        for cite in ("datasets/moco_flow_dataset.py:87-142", "datasets/moco_flow_dataset.py:144-154", "trainer_moco_flow.py:226-268"):
            assert cite in doc, (entry, cite)
    i64, i32, p, f3 = C.c_int64, C.c_int32, C.c_void_p, C.POINTER(C.c_float)
    assert L.SYMBOLS["mf_voxel_mesh"] == (i32, [p, i64, p, i64, i32, i32, i32, f3, f3, f3, p, p, p])
    assert L.SYMBOLS["mf_voxel_fill_scratch_bytes"] == (i64, [i64, i64, i64])
    assert L.SYMBOLS["mf_voxel_fill"] == (i32, [p, i32, i32, i32, p, p, p])
    assert L.SYMBOLS["mf_voxel_dilate_scratch_bytes"] == (i64, [i64, i64, i64])
    assert L.SYMBOLS["mf_voxel_dilate"] == (i32, [p, i32, i32, i32, i32, i32, i32, p, p, p, p])
    for name in ("from_mesh", "from_smpl", "dilated", "filled", "__and__", "__or__"):
        assert callable(getattr(M.OccupancyGrid, name)), name
    assert "mf_voxelize.hip" in open(os.path.join(ROOT, "moco_flow_amd", "csrc", "Makefile")).read()
    unit = open(os.path.join(ROOT, "moco_flow_amd", "csrc", "mf_voxelize.hip")).read()
    assert "2^57" in unit and '#include "mf_unionfind.hpp"' in unit and "#pragma clang fp contract(off)" in unit
    assert f"kVoxSub = {O.SUB};" in unit and f"kVoxMaxSide = {O.MAX_SIDE};" in unit


def _f3(*v):
    return (C.c_float * 3)(*v)


def test_host_side_validation():
    """Grid sides and the cell count, negative radii, T or V, null pointers and an empty box are settled on the host, before
    anything is launched: the fake pointers are never touched."""
    import moco_flow_amd._lib as L
    lib = L.lib()
    fake = C.c_void_p(256)
    lo, hi, inv = _f3(-1, -1, -1), _f3(1, 1, 1), _f3(4, 4, 4)

    def mesh(**k):
        g = k.get("g", (8, 8, 8))
        return lib.mf_voxel_mesh(k.get("verts", fake), k.get("V", 10), k.get("tris", fake), k.get("T", 8), g[0], g[1], g[2],
                                 k.get("lo", lo), k.get("hi", hi), k.get("inv", inv), k.get("bits", fake), None, None)

    for g in ((0, 8, 8), (8, -1, 8), (8, 8, 1025), (1025, 1, 1)):
        assert mesh(g=g) == -1 and b"2^31" in lib.mf_last_error(), g
    assert mesh(V=-1) == -1 and b"V=-1" in lib.mf_last_error()
    assert mesh(T=-1) == -1 and b"T=-1" in lib.mf_last_error()
    assert mesh(V=1 << 31) == -1 and mesh(T=1 << 31) == -1
    for null in ("verts", "tris", "bits", "lo", "hi", "inv"):
        assert mesh(**{null: None}) == -1 and b"null" in lib.mf_last_error(), null
    assert mesh(hi=_f3(1, -1, 1)) == -1 and b"axis 1" in lib.mf_last_error()                   # lo_a >= hi_a
    assert mesh(lo=_f3(-1, -1, 1)) == -1 and b"axis 2" in lib.mf_last_error()
    assert mesh(hi=_f3(float("nan"), 1, 1)) == -1 and mesh(lo=_f3(-float("inf"), -1, -1)) == -1
    assert mesh(inv=_f3(4, 0, 4)) == -1 and b"inv_cell[1]" in lib.mf_last_error()

    size = lib.mf_voxel_fill_scratch_bytes
    big = 1 << 31
    assert size(0, 1, 1) == -1 and size(1, -1, 1) == -1 and b"2^31" in lib.mf_last_error()
    assert size(1 << 11, 1 << 10, 1 << 10) == -1 and size(big, 1, 1) == -1 and size(1 << 20, 1 << 20, 1 << 20) == -1
    assert size(128, 128, 128) == 4 * (128 ** 3 + 1) + 12 and size(1, 1, 1) == 16 and size(1 << 10, 1 << 10, (1 << 11) - 1) > 0
    fill = lambda **k: lib.mf_voxel_fill(k.get("bits", fake), *k.get("g", (8, 8, 8)), k.get("out", fake), k.get("scratch", fake), None)
    assert fill(g=(8, 0, 8)) == -1 and b"2^31" in lib.mf_last_error()
    assert fill(g=(1 << 11, 1 << 10, 1 << 10)) == -1
    for null in ("bits", "out", "scratch"):
        assert fill(**{null: None}) == -1 and b"null" in lib.mf_last_error(), null

    dsize = lib.mf_voxel_dilate_scratch_bytes
    assert dsize(0, 1, 1) == -1 and dsize(1 << 11, 1 << 10, 1 << 10) == -1 and b"2^31" in lib.mf_last_error()
    assert dsize(7, 9, 37) == 2 * 512 + 8                      # 126 words: two slabs of 504 -> 512 bytes, one workgroup's partial
    assert dsize(128, 128, 128) == 2 * 4 * 65536 + 8 * 256
    dil = lambda **k: lib.mf_voxel_dilate(k.get("bits", fake), *k.get("g", (8, 8, 8)), *k.get("r", (1, 1, 1)), k.get("out", C.c_void_p(512)),
                                          None, k.get("scratch", fake), None)
    assert dil(g=(8, 8, 0)) == -1 and b"2^31" in lib.mf_last_error()
    for r in ((-1, 0, 0), (0, -1, 0), (0, 0, -5)):
        assert dil(r=r) == -1 and b"negative" in lib.mf_last_error(), r
    for null in ("bits", "out", "scratch"):
        assert dil(**{null: None}) == -1 and b"null" in lib.mf_last_error(), null
    assert dil(out=fake) == -1 and b"must not be bits" in lib.mf_last_error()


def test_argument_validation_needs_no_gpu():
    import moco_flow_amd as M
    verts, tris = torch.zeros(5, 3), torch.zeros(4, 3, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        M.OccupancyGrid.from_mesh(verts, tris, [[-1, -1, -1], [1, 1, 1]])
