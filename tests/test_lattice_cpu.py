"""Sparse lattice queries without a GPU: the header, the ABI version and the ctypes prototypes of mf_lattice_select /
mf_lattice_points / mf_lattice_scatter, their host-side argument validation through the loaded library (every refusal comes
before any launch), the cell-range tables the host builds (moco_flow_amd.points.brick_cell_ranges against
tests/lattice_oracle.py), and the property that makes the feature more than plumbing: on the oracle, the isosurface of a
sparsely filled volume equals the dense one when the grid covers every crossing cell."""
import ctypes
import os

import numpy as np
import pytest
import torch

import lattice_oracle as LO
import mc_oracle
import occupancy_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mf_lattice_select_scratch_bytes", "mf_lattice_select", "mf_lattice_points", "mf_lattice_scatter")


def test_header_lists_the_entries_and_the_abi_stays_16():
    import moco_flow_amd
    import moco_flow_amd._lib as L
    text = open(os.path.join(ROOT, "include", "mocoflow_hip.h")).read()
    additive = text[text.index("additive entries since, version unchanged"):text.index("#define MF_ABI_VERSION")]
    for name in NAMES:
        assert name in additive, name
    assert "#define MF_ABI_VERSION 16" in text
    for entry in ("mf_lattice_select (serves", "mf_lattice_points (serves", "mf_lattice_scatter (serves"):
        doc = text[text.index(entry):]
        doc = doc[:doc.index("*/")]
        for cite in ("trainer_moco_flow.py:490-538", "trainer_nerf.py:200-259"):      # visualize_mesh: each entry cites it
            assert cite in doc, (entry, cite)
    C = ctypes
    i64, i32, vp = C.c_int64, C.c_int32, C.c_void_p
    want = {"mf_lattice_select_scratch_bytes": (i64, [i64, i64, i64]),
            "mf_lattice_select": (i32, [vp, i32, i32, i32, vp, vp, vp, i64, i64, i64, C.POINTER(i32), vp, vp, vp, vp, vp]),
            "mf_lattice_points": (i32, [vp, i64, vp, vp, vp, i64, i64, i64, C.POINTER(i32), vp, vp]),
            "mf_lattice_scatter": (i32, [vp, vp, i64, i64, i64, i64, C.c_float, vp, vp])}
    lib = L.lib()
    for sym, (res, args) in want.items():
        assert L.SYMBOLS[sym] == (res, args), sym
        fn = getattr(lib, sym)
        assert fn.restype is res and list(fn.argtypes) == args, sym
    assert lib.mf_version() == 16 and L.MF_ABI_VERSION == 16
    assert moco_flow_amd.query_sigma_lattice is moco_flow_amd.points.query_sigma_lattice
    assert "query_sigma_lattice" in moco_flow_amd.__all__
    assert "mf_lattice.hip" in open(os.path.join(ROOT, "moco_flow_amd", "csrc", "Makefile")).read()


def _i3(*v):
    return (ctypes.c_int32 * 3)(*v)


def test_entries_validate_on_the_host():
    """Null pointers, sizes <= 0, a permutation that is not one, a K beyond the bricks: all refused before any launch."""
    import moco_flow_amd._lib as L
    lib = L.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    err = lib.mf_last_error

    def select(bits=p, g=(4, 4, 4), r=(p, p, p), n=(9, 9, 9), woa=(0, 1, 2), slot=p, ids=p, count=p, scratch=p):
        return lib.mf_lattice_select(bits, g[0], g[1], g[2], r[0], r[1], r[2], n[0], n[1], n[2], _i3(*woa) if woa else None,
                                     slot, ids, count, scratch, None)

    def points(ids=p, K=1, ax=(p, p, p), n=(9, 9, 9), woa=(0, 1, 2), out=p):
        return lib.mf_lattice_points(ids, K, ax[0], ax[1], ax[2], n[0], n[1], n[2], _i3(*woa) if woa else None, out, None)

    def scatter(sigma=p, slot=p, K=1, n=(9, 9, 9), fill=0.0, vol=p):
        return lib.mf_lattice_scatter(sigma, slot, K, n[0], n[1], n[2], fill, vol, None)

    for bad in ((0, 9, 9), (9, -1, 9), (9, 9, 0), (1 << 31, 9, 9), (1 << 14, 1 << 14, 1 << 14)):       # the last: 2^33 bricks
        assert lib.mf_lattice_select_scratch_bytes(*bad) == -1 and b"each side >= 1" in err(), bad
        for call in (select, points, scatter):
            assert call(n=bad) == -1 and b"each side >= 1" in err(), (call.__name__, bad)
    assert lib.mf_lattice_select_scratch_bytes(1, 1, 1) == 8                           # one int64 per workgroup of 256 bricks
    assert lib.mf_lattice_select_scratch_bytes(19, 13, 21) == 8                        # 3 x 2 x 3 bricks
    assert lib.mf_lattice_select_scratch_bytes(512, 512, 512) == 8 * 1024              # 64^3 bricks
    assert lib.mf_lattice_select_scratch_bytes(57, 57, 57) == 16                       # 8^3 = 512 bricks
    for woa in ((0, 0, 2), (0, 1, 3), (-1, 1, 2), (1, 1, 1)):
        assert select(woa=woa) == -1 and b"not a permutation" in err(), woa
        assert points(woa=woa) == -1 and b"not a permutation" in err(), woa
    assert select(woa=None) == -1 and b"null world_of_axis" in err()
    assert points(woa=None) == -1 and b"null world_of_axis" in err()
    for g in ((0, 4, 4), (4, -1, 4), (4, 4, 0), (1 << 11, 1 << 10, 1 << 10)):
        assert select(g=g) == -1 and b"cells" in err(), g
    assert select(bits=None) == -1 and b"null bits or range" in err()
    for k in range(3):
        r = [p, p, p]
        r[k] = None
        assert select(r=r) == -1 and b"null bits or range" in err(), k
    for out in ("slot", "ids", "count", "scratch"):
        assert select(**{out: None}) == -1 and b"null output" in err(), out
    assert points(K=-1) == -1 and b"K=-1" in err()
    assert points(K=9) == -1 and b"K=9 of 8 bricks" in err()
    for k in range(3):
        ax = [p, p, p]
        ax[k] = None
        assert points(ax=ax) == -1 and b"null axis" in err(), k
    assert points(ids=None) == -1 and b"null brick_ids or points" in err()
    assert points(out=None) == -1 and b"null brick_ids or points" in err()
    assert points(K=0, ids=None, out=None) == 0                                       # K = 0: nothing is launched
    assert scatter(K=-1) == -1 and b"K=-1" in err()
    assert scatter(K=9) == -1 and b"K=9 of 8 bricks" in err()
    assert scatter(slot=None) == -1 and b"null slot or volume" in err()
    assert scatter(vol=None) == -1 and b"null slot or volume" in err()
    assert scatter(sigma=None) == -1 and b"null sigma" in err()


def test_python_layer_refuses_before_any_launch():
    import moco_flow_amd as M
    nerf = M.NeRF(8, 256, 63, [4], "dir", 27)                                         # on the CPU
    emb = M.Embedding(3, 10)
    ax = np.linspace(-1, 1, 9, dtype=np.float32)

    class Grid:                                                                       # never reached
        device = torch.device("cpu")
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        M.query_sigma_lattice((ax, ax, ax), nerf, emb, Grid())
    with pytest.raises(RuntimeError, match="three coordinate arrays"):
        M.query_sigma_lattice((ax, ax), nerf, emb, Grid())
    with pytest.raises(RuntimeError, match="not a permutation"):
        M.query_sigma_lattice((ax, ax, ax), nerf, emb, Grid(), world_of_axis=(0, 0, 1))
    with pytest.raises(RuntimeError, match="margin=-1"):
        M.query_sigma_lattice((ax, ax, ax), nerf, emb, Grid(), margin=-1)
    with pytest.raises(RuntimeError, match="per-point"):
        M.query_sigma_lattice((ax, ax, ax), nerf, emb, Grid(), ind=torch.zeros(9 ** 3))


# ------------------------------------------------------------------------------------------------ the range tables
def _grid_consts(dims, lo, hi):
    lo32, hi32, inv, _ = O.grid_constants(dims, lo, hi, 0.5)
    return lo32, hi32, inv


@pytest.mark.parametrize("margin", [0, 1, 2, 5])
def test_range_tables_are_monotone_clamped_and_empty_outside_the_box(margin):
    from moco_flow_amd.points import brick_cell_ranges
    G = 11
    lo, hi, inv = _grid_consts((G, G, G), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    cases = {"inside": np.linspace(-0.9, 0.95, 37), "exact": np.linspace(-1.0, 1.0, 23),
             "overhang_hi": np.linspace(-0.5, 3.0, 41),                               # the last bricks lie beyond hi
             "overhang_lo": np.linspace(-4.0, 0.25, 50),
             "outside_hi": np.linspace(1.25, 2.0, 19), "outside_lo": np.linspace(-3.0, -1.001, 9),
             "one_point": np.array([0.3]), "around": np.linspace(-5.0, 5.0, 7)}
    for name, x in cases.items():
        X = x.astype(np.float32)
        got = brick_cell_ranges(X, margin, lo[0], hi[0], inv[0], G)
        want = LO.range_table(X, margin, lo[0], hi[0], inv[0], G)
        assert got.dtype == np.int32 and got.shape == ((len(X) + 7) // 8, 2) and np.array_equal(got, want), name
        empty = got[:, 0] > got[:, 1]
        assert (got[empty] == (1, 0)).all()
        live = got[~empty]
        assert (live >= 0).all() and (live <= G - 1).all(), name                      # clamped
        assert (np.diff(live[:, 0]) >= 0).all() and (np.diff(live[:, 1]) >= 0).all(), name   # monotone in the brick
        for b in range(len(got)):                                                     # empty exactly when wholly outside
            i0, i1 = max(8 * b - margin, 0), min(8 * b + 7 + margin, len(X) - 1)
            assert empty[b] == bool(X[i1] < lo[0] or X[i0] > hi[0]), (name, b)
        if name.startswith("outside"):
            assert empty.all(), name
        if name in ("inside", "exact", "around"):
            assert not empty.any(), name
        if name == "overhang_hi" and margin < 5:
            assert not empty[0] and empty[-1] and got[~empty][-1, 1] == G - 1, name
        if name == "overhang_lo" and margin < 5:
            assert empty[0] and not empty[-1] and got[~empty][0, 0] == 0, name
        if name == "around":
            assert got[0, 0] == 0 and got[-1, 1] == G - 1, name                       # the box lies inside one grown brick


def test_select_of_a_lattice_outside_the_box_is_empty():
    dense = np.ones((4, 5, 6), dtype=bool)
    lo, hi, inv = _grid_consts(dense.shape, (-1, -1, -1), (1, 1, 1))
    inside, outside = np.linspace(-1, 1, 19, dtype=np.float32), np.linspace(1.5, 2.5, 13, dtype=np.float32)
    for axes in ((outside, inside, inside), (inside, outside, inside), (inside, inside, outside)):
        n = [len(a) for a in axes]
        slot, ids, K = LO.select(dense, LO.range_tables(axes, 1, dense.shape, lo, hi, inv), n)
        assert K == 0 and len(ids) == 0 and (slot == -1).all()
    axes = (inside, inside, inside)
    slot, ids, K = LO.select(dense, LO.range_tables(axes, 1, dense.shape, lo, hi, inv), [19] * 3)
    assert K == 27 and np.array_equal(ids, np.arange(27)) and np.array_equal(slot, np.arange(27))


def test_select_fast_equals_select():
    """LO.select_fast (all bricks at once, for the large lattices of tests/test_gpu_lattice.py) against the brick-by-brick
    definition: every lattice and grid the select tests use, partly covering and overhanging boxes, empty and full grids,
    a lattice outside the box, and a flat lattice of 129 x 129 bricks."""
    box = ((-0.4, -1.2, -0.1), (0.7, 0.3, 2.0))
    unit = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    lin = lambda n, lo=unit[0], hi=unit[1]: [np.linspace(lo[a], hi[a], n[a]).astype(np.float32) for a in range(3)]
    rng = np.random.default_rng(3)
    cases = [(rng.random((5, 4, 7)) < d, box, lin(n)) for d in (0.0, 0.1, 0.15, 1.0)
             for n in ((19, 13, 21), (8, 16, 8), (2, 2, 2), (9, 2, 65), (70, 60, 50))]
    cases += [(rng.random((40, 40, 40)) < 0.0004, unit, lin((12, 12, 12))), (rng.random((40, 40, 40)) < 0.2, unit, lin((1025, 1025, 1))),
              (rng.random((19, 16, 22)) < 0.05, ((-1.0, -0.8, -1.1), (1.0, 0.9, 1.2)), lin((20, 17, 23), (-1.0, -0.8, -1.1), (1.0, 0.9, 1.2))),
              (np.ones((4, 5, 6), dtype=bool), unit, lin((19, 13, 19), (1.5, -1.0, -1.0), (2.5, 1.0, 1.0)))]
    partial = 0
    for dense, (lo, hi), axes in cases:
        n = [len(a) for a in axes]
        lo32, hi32, inv = _grid_consts(dense.shape, lo, hi)
        for woa in ((0, 1, 2), (1, 0, 2), (2, 0, 1)):
            for margin in (0, 1, 2):
                tables = LO.range_tables(axes, margin, dense.shape, lo32, hi32, inv, woa)
                want, got = LO.select(dense, tables, n, woa), LO.select_fast(dense, tables, n, woa)
                for w, g in zip(want[:2], got[:2]):
                    assert g.dtype == w.dtype and np.array_equal(g, w), (dense.shape, n, woa, margin)
                assert got[2] == want[2]
                partial += 0 < want[2] < len(want[0])
    assert partial > len(cases) * 9 // 3                               # bricks on both sides in more than a third of the runs


def test_points_and_scatter_invert_each_other():
    n = (19, 13, 21)
    rng = np.random.default_rng(5)
    vol = rng.normal(size=n).astype(np.float32)
    nb = LO.n_bricks(n)
    on = rng.random(nb[0] * nb[1] * nb[2]) < 0.5
    ids = np.nonzero(on)[0].astype(np.int32)
    slot = np.where(on, np.cumsum(on) - 1, -1).astype(np.int32)
    back = LO.scatter(LO.gather(vol, ids), slot, n, np.float32(-np.inf))
    mask = LO.active_mask(slot, n)
    assert 0 < mask.sum() < mask.size
    assert np.array_equal(back[mask], vol[mask]) and np.isneginf(back[~mask]).all()
    ax = [np.linspace(-1, 1, v).astype(np.float32) + a for a, v in enumerate(n)]
    pts = LO.points(ids, ax, (1, 0, 2))
    assert pts.shape == (len(ids) * 512, 3)
    b = np.unravel_index(int(ids[-1]), nb)                                            # the last active brick, last local point
    want = [ax[a][min(8 * b[a] + 7, n[a] - 1)] for a in range(3)]
    assert pts[-1, 1] == want[0] and pts[-1, 0] == want[1] and pts[-1, 2] == want[2]


# ------------------------------------------------------------------------------------------------ the guarantee
def test_sparse_isosurface_equals_the_dense_one_on_the_oracle():
    """A ball in a (20, 17, 23) lattice, iso = 2: its grid at tau = iso / 2 (relu, dilate = 0, cells = the lattice cells)
    marks every cell with a corner above tau, hence every cell that crosses iso.  With margin = 1 every corner of such a cell
    lies in an active brick, and the points left at fill = 0 are all below iso: marching cubes of the sparse volume equals
    that of the dense one, vertices and triangles bit for bit.

    margin = 0 is NOT enough even though cells and lattice cells coincide: the cell of X[i] is floor((X[i] - lo) * inv_cell)
    in fp32, and rounding may put X[i] into cell i - 1 -- a brick whose first point is corner i + 1 = 8 b of a crossing cell i
    would then look at cells from i on at best, or, on the other side, a brick ending at point i would stop at cell i - 1.
    One lattice point of margin moves both ends a whole cell outward, which no rounding of a last place undoes."""
    n = (20, 17, 23)
    lo, hi = (-1.0, -0.8, -1.1), (1.0, 0.9, 1.2)
    iso = 2.0
    sigma = O.ball_lattice(n, lo, hi, center=(-0.45, -0.3, -0.5), radius=0.27)       # 5 inside, -5 outside
    words, count = O.build(sigma, "relu", iso / 2, 0)
    dims = (n[0] - 1, n[1] - 1, n[2] - 1)
    dense = O.unpack(words, dims[2])
    assert dense.shape == dims and 0 < count < dense.size
    lo32, hi32, inv = _grid_consts(dims, lo, hi)
    axes = [np.linspace(lo[a], hi[a], n[a]).astype(np.float32) for a in range(3)]
    slot, ids, K = LO.select(dense, LO.range_tables(axes, 1, dims, lo32, hi32, inv), n)
    nb = LO.n_bricks(n)
    assert nb == (3, 3, 3) and 0 < K < 27                                             # bricks on both sides
    assert (slot >= 0).sum() == K and np.array_equal(np.nonzero(slot >= 0)[0], ids)
    sparse = LO.scatter(LO.gather(sigma, ids), slot, n, np.float32(0.0))
    mask = LO.active_mask(slot, n)
    assert np.array_equal(sparse[mask], sigma[mask]) and (sparse[~mask] == 0).all() and (sigma[~mask] == -5).all()
    assert (sigma >= iso).any() and not (sigma[~mask] >= iso).any()
    v_d, t_d = mc_oracle.marching_cubes(sigma, iso)
    v_s, t_s = mc_oracle.marching_cubes(sparse, iso)
    assert len(v_d) >= 24 and len(t_d) >= 24
    assert v_s.dtype == v_d.dtype and np.array_equal(v_s, v_d) and np.array_equal(t_s, t_d)
    v_c, t_c = mc_oracle.marching_cubes(sparse, iso, clamp_zero=True)                 # what extract_mesh meshes
    v_e, t_e = mc_oracle.marching_cubes(sigma, iso, clamp_zero=True)
    assert np.array_equal(v_c, v_e) and np.array_equal(t_c, t_e)
