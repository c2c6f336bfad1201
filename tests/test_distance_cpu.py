"""CPU-side checks (-m "not gpu") of the Euclidean shell and the distance field (csrc/mf_distance.hip; OccupancyGrid.euclid_metric,
squared_distance, dilated_euclidean, from_mesh(shell="euclidean")): the oracle's integer metric against the package's and
against a table of values derived by hand; the brute-force distance against the windowed three-pass restatement that the kernels
follow; the guarantee of from_mesh's docstring as a property of the oracle, by sampling; the library's exports and prototypes;
every refusal that is made before a launch.  None of it touches a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import distance_oracle as D
import voxelize_oracle as VO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mf_grid_edt_scratch_bytes", "mf_grid_edt")

# the grids tests/test_gpu_voxelize.py names, the world radius used on each, and (w, R, r) derived by hand from the formula
GRIDS = {
    "tail": ((7, 9, 37), (0.0, 0.0, 0.0), (7.0, 9.0, 37.0)),
    "whole": ((5, 6, 64), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)),
    "aniso": ((3, 4, 70), (-0.9371, -0.4113, -1.2837), (0.7129, 0.5291, 1.1173)),
}
TABLE = {
    "tail": (2.5, (65536, 65536, 65536), 409600, (2, 2, 2)),
    "aniso": (0.31, (65536, 11974, 254), 20820, (0, 1, 9)),
    "whole": (0.45, (65536, 45511, 400), 82944, (1, 1, 14)),
}


def sparse_cells(dims, seed=31):
    """Random cells at 1 %, plus cells at k = 31 / 32 / 36 (a word seam and the tail) and in the grid's corners."""
    dense = np.random.default_rng(seed).random(dims) < 0.01
    hand = np.zeros(dims, dtype=bool)
    for k in (31, 32, 36):
        hand[dims[0] // 2, dims[1] // 2, min(k, dims[2] - 1)] = True
    for corner in np.ndindex(2, 2, 2):
        hand[tuple(-c for c in corner)] = True
    return dense, hand


def test_metric_equals_the_package_and_the_table():
    import moco_flow_amd as M
    for name, (dims, lo, hi) in GRIDS.items():
        t, w, R, r = TABLE[name]
        cell = D.cell_edges(dims, lo, hi)
        assert D.euclid_metric(cell, t) == (w, R, r), name
        got = M.OccupancyGrid.euclid_metric(cell, t)
        assert got == (w, R, r) and all(type(x) is int for x in got[0] + (got[1],) + got[2]), (name, got)
        for radius in (0.0, 0.013, 0.2, 1.7, 127.9 * float(cell.max())):
            assert M.OccupancyGrid.euclid_metric(cell, radius) == D.euclid_metric(cell, radius), (name, radius)
    assert D.euclid_metric((1.0, 1.0, 1.0), 0.0) == ((65536,) * 3, 0, (0, 0, 0))
    # the floor on w and the ceil on R: a superset of the real-valued ellipsoid
    cell = D.cell_edges(*GRIDS["aniso"])
    w, R, _ = D.euclid_metric(cell, 0.31)
    k = np.stack(np.meshgrid(*[np.arange(-12, 13)] * 3, indexing="ij"), -1).reshape(-1, 3)
    inside = ((k * cell) ** 2).sum(1) <= 0.31 ** 2
    assert inside.sum() > 20 and ((k ** 2 * np.asarray(w)).sum(1)[inside] <= R).all()
    for bad in (dict(cell=(1.0, 1.0, 1.0), radius=128.0), dict(cell=(1.0, 1.0, 1.0), radius=-0.1), dict(cell=(1.0, 1.0, 1.0), radius=float("nan")),
                dict(cell=(1.0, 1.0, 1.0), radius=float("inf")), dict(cell=(1.0, 1.0 / 257, 1.0), radius=0.1), dict(cell=(1.0, 0.0, 1.0), radius=0.1),
                dict(cell=(1.0, 1.0), radius=0.1)):
        with pytest.raises(RuntimeError):
            M.OccupancyGrid.euclid_metric(**bad)
    assert M.OccupancyGrid.euclid_metric((1.0, 1.0, 1.0), 127.99)[1] < 1 << 30


def test_brute_force_equals_the_windowed_separable_passes():
    for name, (dims, lo, hi) in GRIDS.items():
        t, w, R, r = TABLE[name]
        random, hand = sparse_cells(dims)
        one = np.zeros(dims, dtype=bool)
        one[0, dims[1] - 1, dims[2] // 2] = True
        for dense in (random, hand, random | hand, one, np.zeros(dims, bool), np.ones(dims, bool)):
            want = D.squared_distance(dense, w, R)
            assert want.dtype == np.int32 and np.array_equal(D.separable_d2(dense, w, R), want), name
            assert np.array_equal(want == 0, dense) and (dense.any() or (want == R + 1).all())
        # a reach beyond every side, and radius 0
        wide = D.euclid_metric(D.cell_edges(dims, lo, hi), 1.05 * float(np.max(np.asarray(hi) - np.asarray(lo))))
        assert all(wide[2][a] >= dims[a] - 1 for a in range(3))
        assert np.array_equal(D.separable_d2(hand, wide[0], wide[1]), D.squared_distance(hand, wide[0], wide[1]))
        far = D.squared_distance(one, wide[0], wide[1]) <= wide[1]          # along each axis the whole line through the cell
        assert far[:, dims[1] - 1, dims[2] // 2].all() and far[0, :, dims[2] // 2].all() and far[0, dims[1] - 1, :].all()
        assert np.array_equal(D.squared_distance(random, w, 0) <= 0, random)
        assert np.array_equal(D.dilate_euclidean(random, D.cell_edges(dims, lo, hi), 0.0), random)
    # cubic cells: the plain Euclidean test in cell units
    dims = (9, 9, 9)
    one = np.zeros(dims, dtype=bool)
    one[4, 4, 4] = True
    ball = D.dilate_euclidean(one, (0.5, 0.5, 0.5), 1.25)                   # 2.5 cells
    k = np.stack(np.meshgrid(*[np.arange(9) - 4] * 3, indexing="ij"), -1)
    assert np.array_equal(ball, (k ** 2).sum(-1) <= 6)


def test_guarantee_points_within_thickness_of_a_set_cell_fall_in_the_shell_grown_by_one_cell():
    """from_mesh(shell="euclidean")'s guarantee, in exact arithmetic (float64 points, the true cell of a point): a point within t
    of a point of a set cell lies in a cell of E(t) + box(1).  ``dilate`` is left to absorb the fp32 cell rule and the snapping,
    which the box path's test already holds it to."""
    rng = np.random.default_rng(19)
    dims, t = (32, 32, 32), 0.2
    lo, hi = (np.array(v, dtype=np.float32).astype(np.float64) for v in ([-0.75, -1.15, -0.55], [0.75, 1.15, 0.55]))    # an fp32 box
    verts, tris = VO.icosphere(2, center=(0.03, -0.05, 0.02), radius=0.3)
    body = VO.fill(VO.surface(verts, tris, dims, lo, hi)[0])
    cell = D.cell_edges(dims, lo, hi)
    assert np.array_equal(cell, (hi - lo) / 32) and len(set(cell.tolist())) == 3
    shell = VO.dilate(D.dilate_euclidean(body, cell, t), (1, 1, 1))
    assert 0 < body.sum() < shell.sum() < shell.size
    cells = np.argwhere(body)
    n = 200000
    p = lo + (cells[rng.integers(len(cells), size=n)] + rng.random((n, 3))) * cell
    d = rng.normal(size=(n, 3))
    d *= (t * rng.random((n, 1)) ** (1 / 3)) / np.linalg.norm(d, axis=1, keepdims=True)
    d[::4] *= t / np.linalg.norm(d[::4], axis=1, keepdims=True)            # a quarter of them at the full length
    d[::4] *= 1.0 - 1e-12
    q = p + d
    q = q[((q >= lo) & (q < hi)).all(1)]
    assert len(q) > 150000
    c = np.floor((q - lo) / cell).astype(np.int64)
    assert ((c >= 0) & (c < 32)).all()
    assert shell[c[:, 0], c[:, 1], c[:, 2]].all()
    # without the extra cell the Euclidean ball of the index metric alone misses some of them: the box(1) is needed
    assert not D.dilate_euclidean(body, cell, t)[c[:, 0], c[:, 1], c[:, 2]].all()


def test_library_exports_header_symbols_and_prototypes():
    import moco_flow_amd as M
    import moco_flow_amd._lib as L
    header = open(os.path.join(ROOT, "include", "mocoflow_hip.h")).read()
    declared = set(re.findall(r"^int(?:32|64)_t (mf_\w+)\(", header, re.M))
    lib = L.lib()
    assert lib.mf_version() == 16 and L.MF_ABI_VERSION == 16 and "#define MF_ABI_VERSION 16" in header
    additive = header[header.index("additive entries since, version unchanged"):header.index("#define MF_ABI_VERSION")]
    for name in NEW_SYMBOLS:
        assert name in declared and name in additive, name
        fn = getattr(lib, name)
        assert fn.restype is L.SYMBOLS[name][0] and list(fn.argtypes) == L.SYMBOLS[name][1]
    i64, i32, p = C.c_int64, C.c_int32, C.c_void_p
    assert L.SYMBOLS["mf_grid_edt_scratch_bytes"] == (i64, [i64, i64, i64])
    assert L.SYMBOLS["mf_grid_edt"] == (i32, [p, i32, i32, i32, C.POINTER(i32), i32, p, p, p, p, p])
    for name in ("euclid_metric", "squared_distance", "dilated_euclidean"):
        assert callable(getattr(M.OccupancyGrid, name)), name
    assert "mf_distance.hip" in open(os.path.join(ROOT, "moco_flow_amd", "csrc", "Makefile")).read()


def test_host_side_validation():
    """Sides, weights, the radius, null pointers and aliasing are settled on the host, before anything is launched: the fake
    pointers are never touched."""
    import moco_flow_amd._lib as L
    lib = L.lib()
    fake, other = C.c_void_p(256), C.c_void_p(512)
    w3 = lambda *v: (C.c_int32 * 3)(*v)

    def edt(**k):
        return lib.mf_grid_edt(k.get("bits", fake), *k.get("g", (8, 8, 8)), k.get("w", w3(65536, 65536, 65536)), k.get("R", 100),
                               k.get("d2", other), k.get("out", other), k.get("count", None), k.get("scratch", fake), None)

    for g in ((0, 8, 8), (8, 0, 8), (8, 8, 0), (1025, 8, 8), (8, 1025, 8), (8, 8, 1025), (8, -1, 8)):
        assert edt(g=g) == -1 and b"each side 1 .. 1024" in lib.mf_last_error(), g
    for a in range(3):
        for bad in (0, 65537, -1):
            w = [65536, 65536, 65536]
            w[a] = bad
            assert edt(w=w3(*w)) == -1 and b"w[%d]=%d" % (a, bad) in lib.mf_last_error(), (a, bad)
    assert edt(w=None) == -1 and b"null w" in lib.mf_last_error()
    for bad in (-1, 1 << 30):
        assert edt(R=bad) == -1 and b"R=%d" % bad in lib.mf_last_error(), bad
    assert edt(d2=None, out=None) == -1 and b"nothing to write" in lib.mf_last_error()
    assert edt(out=fake) == -1 and b"must not be bits" in lib.mf_last_error()
    assert edt(out=None, count=other) == -1 and b"count_out needs bits_out" in lib.mf_last_error()
    for null in ("bits", "scratch"):
        assert edt(**{null: None}) == -1 and b"null" in lib.mf_last_error(), null

    size = lib.mf_grid_edt_scratch_bytes
    for g in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (1025, 1, 1), (1, 1025, 1), (1, 1, 1025), (1, -1, 1), (1 << 40, 1, 1)):
        assert size(*g) == -1 and b"each side 1 .. 1024" in lib.mf_last_error(), g
    # uint16 + int32 per cell, each padded to 16 bytes, and one float64 per workgroup of four 64-cell pieces of a row
    assert size(1, 1, 1) == 16 + 16 + 16
    assert size(7, 9, 37) == 4672 + 9328 + 128                              # 2331 cells, 63 pieces -> 16 workgroups
    assert size(128, 128, 128) == 6 * 128 ** 3 + 8 * (128 * 128 * 2 // 4)
    assert size(1024, 1024, 1024) == 6 * 1024 ** 3 + 8 * (1024 * 1024 * 16 // 4)
    with pytest.raises(RuntimeError, match="each side 1 .. 1024"):
        L.need("mf_grid_edt_scratch_bytes", 8, 8, 2048)


def test_argument_validation_needs_no_gpu():
    import moco_flow_amd as M
    verts, tris = torch.zeros(5, 3), torch.zeros(4, 3, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        M.OccupancyGrid.from_mesh(verts, tris, [[-1, -1, -1], [1, 1, 1]], shell="euclidean")
