"""Occupancy grids from a mesh on the MI355X: mf_voxel_mesh, mf_voxel_fill, mf_voxel_dilate (csrc/mf_voxelize.hip) and
OccupancyGrid.from_mesh / from_smpl / filled / dilated / & / | against the numpy oracle of their contracts
(tests/voxelize_oracle.py).  Every result is defined in integers: words (padding bits included), counts and dropped triangles
are compared for equality, with no tolerance and nothing left out.  The kernel decides the surface predicate by Schwarz and
Seidel's test, the oracle by the 13-axis separating-axis test.

Launch bounds: the small-box pass runs at most kVoxMaxBlocks workgroups of kVoxTrisPerBlock triangles, the large-box pass at most
kVoxBigMaxBlocks workgroups of kVoxThreads triangles -- 16 384 triangles per trip of either grid-stride loop; the level-5
icosphere (20 480 triangles, a large triangle appended behind them) takes both loops past their first trip."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import occupancy_oracle as RO
import voxelize_oracle as O
from helpers import build_case

pytestmark = pytest.mark.gpu

_SRC = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "moco_flow_amd", "csrc", "mf_voxelize.hip")).read()


def _const(name):
    return int(re.search(r"\bconstexpr int %s = (\d+);" % name, _SRC).group(1))


THREADS, LANES_PER_TRI = _const("kVoxThreads"), _const("kVoxLanesPerTri")
TRIS_PER_TRIP = _const("kVoxMaxBlocks") * (THREADS // LANES_PER_TRI)
BIG_TRIS_PER_TRIP = _const("kVoxBigMaxBlocks") * THREADS
SMALL_CELLS = _const("kVoxSmallCells")

# (dims, lo, hi): a word tail over unit cells; whole words; an anisotropic box whose corners are no short decimals
GRIDS = {
    "tail": ((7, 9, 37), (0.0, 0.0, 0.0), (7.0, 9.0, 37.0)),
    "whole": ((5, 6, 64), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)),
    "aniso": ((3, 4, 70), (-0.9371, -0.4113, -1.2837), (0.7129, 0.5291, 1.1173)),
}


@pytest.fixture(scope="module")
def M():
    import moco_flow_amd
    assert torch.cuda.is_available()
    moco_flow_amd._lib.lib()
    return moco_flow_amd


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _words(grid):
    return grid.bits.cpu().numpy().view(np.uint32)


def _grid(M, dense, lo, hi):
    return M.OccupancyGrid(_dev(O.pack(dense).view(np.int32)), dense.shape, lo, hi)


def _f3(v):
    return (ctypes.c_float * 3)(*[float(x) for x in v])


def _surface(M, verts, tris, dims, lo, hi):
    """mf_voxel_mesh alone, on bits_out filled with ones beforehand: (OccupancyGrid, dropped)."""
    lo32, hi32, inv = O.grid_constants(dims, lo, hi)
    verts, tris = np.asarray(verts, np.float32).reshape(-1, 3), np.asarray(tris, np.int64).reshape(-1, 3)
    v, t = _dev(verts), _dev(tris)
    bits = torch.full((dims[0], dims[1], (dims[2] + 31) // 32), -1, dtype=torch.int32, device="cuda")
    dropped = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    lib = M._lib.lib()
    rc = lib.mf_voxel_mesh(v.data_ptr() if len(verts) else None, len(verts), t.data_ptr() if len(tris) else None, len(tris), *dims,
                           _f3(lo32), _f3(hi32), _f3(inv), bits.data_ptr(), dropped.data_ptr(), torch.cuda.current_stream().cuda_stream)
    M._lib.check(rc, "mf_voxel_mesh")
    grid = M.OccupancyGrid(bits, dims, lo, hi)
    assert np.array_equal(grid.inv_cell, inv)
    return grid, int(dropped.item())


def _check_surface(M, verts, tris, grid_name, what):
    dims, lo, hi = GRIDS[grid_name] if isinstance(grid_name, str) else grid_name
    want, want_dropped = O.surface(verts, tris, dims, lo, hi)
    grid, dropped = _surface(M, verts, tris, dims, lo, hi)
    got = _words(grid)
    assert np.array_equal(got, O.pack(want)), (what, grid_name, int((got != O.pack(want)).sum()))
    assert dropped == want_dropped, (what, grid_name, dropped, want_dropped)
    return want, want_dropped


def _at(grid_name, ijk):
    """World points (fp32) at grid coordinates ijk (in cells) of a grid."""
    dims, lo, hi = GRIDS[grid_name]
    return O.grid_point(ijk, lo, hi, dims).astype(np.float32)


# ---- surface -------------------------------------------------------------------------------------------------------------------

def _hand_cases(dims):
    """name -> (corners in grid coordinates (n, 3, 3), what the case must show: (min cells, max cells))."""
    g = np.asarray(dims, dtype=np.float64)
    far = g + 5000.0                                                            # beyond the saturation range of 2048 cells
    return {
        "in a cell face": ([[[2.0, 1.25, 1.25], [2.0, 1.75, 1.25], [2.0, 1.25, 1.75]]], (2, 2)),
        "corner on a cell corner": ([[[2.0, 2.0, 2.0], [2.25, 2.0, 2.0], [2.0, 2.25, 2.0]]], (8, 8)),
        "needle": ([[[0.3, 0.3, 0.3], g - 0.3, [0.3 + 1.0 / 32, 0.3, 0.3]]], (max(dims), None)),
        "across the grid": ([[[0.0, 0.0, 0.0], g, [g[0], 0.0, g[2]]]], (max(dims), None)),
        "partly outside": ([[[1.5, 1.5, 1.5], g + [3.0, 2.0, 9.0], [-4.0, 2.5, 3.0]]], (3, None)),
        "wholly outside": ([[g + 2.0, g + [3.0, 2.0, 4.0], g + [2.0, 5.0, 3.0]], [[-3.0, 1.0, 1.0], [-2.0, 2.0, 1.0], [-2.5, 1.0, 4.0]]], (0, 0)),
        "beyond the saturation range": ([[[0.5, 0.5, 0.5], far, [2.5, 0.5, 1.5]], [[1.5, 1.5, 1.5], -far, [0.5, 2.5, 1.5]]], (3, None)),
    }


@pytest.mark.parametrize("grid_name", sorted(GRIDS))
def test_surface_of_hand_placed_triangles(M, grid_name):
    dims = GRIDS[grid_name][0]
    for what, (corners, (least, most)) in _hand_cases(dims).items():
        verts = _at(grid_name, np.asarray(corners, dtype=np.float64).reshape(-1, 3))
        tris = np.arange(len(verts)).reshape(-1, 3)
        dense, dropped = _check_surface(M, verts, tris, grid_name, what)
        assert dropped == 0 and dense.sum() >= least and (most is None or dense.sum() <= most), (what, int(dense.sum()))
    # the box of the triangle across the (7, 9, 37) grid is one of the large ones, the others' boxes are small
    assert np.prod(GRIDS["tail"][0]) > SMALL_CELLS > 8


def test_surface_skips_and_counts_bad_triangles(M):
    for grid_name in sorted(GRIDS):
        verts = np.concatenate([_at(grid_name, [[0.5, 0.5, 0.5], [2.5, 0.5, 0.5], [0.5, 2.5, 0.5], [1.5, 1.5, 1.5]]),
                                np.array([[np.nan, 0, 0], [0, -np.inf, 0]], np.float32)])
        V = len(verts)
        tris = [[0, 1, 2], [0, 1, -1], [V, 1, 2], [0, 4, 1], [5, 1, 2], [0, 0, 1], [3, 3, 3], [1 << 40, 1, 2], [2, 1, 3]]
        dense, dropped = _check_surface(M, verts, tris, grid_name, "bad triangles")
        assert dropped == 7 and dense.any()
        _check_surface(M, verts, np.zeros((0, 3), np.int64), grid_name, "T = 0")
        dense, dropped = _check_surface(M, np.zeros((0, 3), np.float32), tris, grid_name, "V = 0")
        assert dropped == len(tris) and not dense.any()


def test_surface_on_a_grid_of_one_cell(M):
    grid = ((1, 1, 1), (-0.31, 0.17, 2.03), (0.29, 0.83, 2.71))
    lo, hi = np.asarray(grid[1]), np.asarray(grid[2])
    through = lo + (hi - lo) * np.array([[0.2, 0.2, 0.5], [0.9, 0.1, 0.5], [0.4, 0.8, 0.6]])
    beside = through + (hi - lo) * 3.0
    for what, verts, n in (("through", through, 1), ("beside", beside, 0), ("both", np.concatenate([beside, through]), 1)):
        dense, dropped = _check_surface(M, verts, np.arange(len(verts)).reshape(-1, 3), grid, what)
        assert dense.sum() == n and dropped == 0


@functools.lru_cache(maxsize=None)
def _sphere5():
    """The level-5 icosphere in the 'tail' grid's box with one large triangle behind its 20 480: past one trip of both loops."""
    verts, tris = O.icosphere(5, center=(3.4, 4.6, 18.2), radius=3.1)
    big = np.array([[0.2, 0.4, 0.6], [6.8, 8.7, 36.1], [6.5, 0.3, 30.2]], np.float32)
    verts = np.concatenate([verts, big])
    tris = np.concatenate([tris, [[len(verts) - 3, len(verts) - 2, len(verts) - 1]]])
    assert len(tris) - 1 > TRIS_PER_TRIP and len(tris) - 1 >= BIG_TRIS_PER_TRIP and len(tris) < 2 * TRIS_PER_TRIP
    return verts, tris


def test_surface_past_the_first_trip_and_under_shuffled_rows(M):
    verts, tris = _sphere5()
    dims, lo, hi = GRIDS["tail"]
    dense, dropped = _check_surface(M, verts, tris, "tail", "icosphere")
    assert dropped == 0
    last = O.surface(verts, tris[TRIS_PER_TRIP:], dims, lo, hi)[0]
    first = O.surface(verts, tris[:TRIS_PER_TRIP], dims, lo, hi)[0]
    assert (last & ~first).sum() > 50                                          # cells that only the second trip sets
    perm = np.random.default_rng(2).permutation(len(tris))
    shuffled, _ = _surface(M, verts, tris[perm], dims, lo, hi)
    assert np.array_equal(_words(shuffled), O.pack(dense))


def test_from_mesh_is_deterministic(M):
    verts, tris = _sphere5()
    dims, lo, hi = GRIDS["tail"]
    v, t = _dev(verts), _dev(tris)
    a = M.OccupancyGrid.from_mesh(v, t, [lo, hi], dims, dilate=1)
    b = M.OccupancyGrid.from_mesh(v, t, [lo, hi], dims, dilate=1)
    assert torch.equal(a.bits, b.bits) and torch.equal(a._count, b._count)
    s1, s2 = _surface(M, verts, tris, dims, lo, hi)[0], _surface(M, verts, tris, dims, lo, hi)[0]
    assert torch.equal(s1.bits, s2.bits)


# ---- fill ----------------------------------------------------------------------------------------------------------------------

FILL_GRID = ((20, 18, 37), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))


@functools.lru_cache(maxsize=None)
def _fill_shapes():
    c = (0.02, -0.03, 0.01)
    return {
        "icosphere": O.icosphere(2, c, 0.8),
        "torus": O.torus(0.58, 0.3, center=c),
        "nested spheres": O.nested_spheres(2, c, 0.85, 0.4),
        "open hemisphere": O.hemisphere(2, c, 0.8),
        "sphere cut by the box": O.icosphere(2, (0.6, 0.0, 0.0), 0.7),
    }


def _check_fill(M, dense, lo, hi, what):
    want = O.fill(dense)
    got = _grid(M, dense, lo, hi).filled()
    assert np.array_equal(_words(got), O.pack(want)), (what, dense.shape)
    assert got._count is None and got.occupied_fraction() == want.sum() / want.size
    return want


def test_fill_of_closed_open_and_cut_shells(M):
    dims, lo, hi = FILL_GRID
    added = {}
    for what, (verts, tris) in _fill_shapes().items():
        shell = O.surface(verts, tris, dims, lo, hi)[0]
        full = _check_fill(M, shell, lo, hi, what)
        added[what] = int(full.sum() - shell.sum())
        if what == "torus":
            assert not full[10, 9, 18] and not full[10, 9, :].any()             # the hole through the torus stays empty
        if what == "nested spheres":
            assert full[10, 9, 18] and full[6:14, 6:12, 12:25].all()            # filled through the inner shell
    assert added["icosphere"] > 500 and added["torus"] > 50 and added["nested spheres"] > added["icosphere"]
    assert added["open hemisphere"] == 0 and added["sphere cut by the box"] == 0    # both leak


@pytest.mark.parametrize("grid_name", sorted(GRIDS))
def test_fill_on_the_listed_grids(M, grid_name):
    dims, lo, hi = GRIDS[grid_name]
    centre, half = (np.asarray(lo) + np.asarray(hi)) / 2, (np.asarray(hi) - np.asarray(lo)) / 2
    for what, (verts, tris) in _fill_shapes().items():
        shell = O.surface(verts.astype(np.float64) * half + centre, tris, dims, lo, hi)[0]
        _check_fill(M, shell, lo, hi, what)
    rng = np.random.default_rng(23)
    for p in (0.35, 0.6, 0.8):
        _check_fill(M, rng.random(dims) < p, lo, hi, f"random {p}")
    assert not _check_fill(M, np.zeros(dims, bool), lo, hi, "empty").any()
    assert _check_fill(M, np.ones(dims, bool), lo, hi, "full").all()
    box = np.zeros(dims, bool)                                                  # a closed box of cells, one cell thick, hollow
    box[:, :, 1:dims[2] - 1] = True
    box[1:-1, 1:-1, 2:dims[2] - 2] = False
    assert _check_fill(M, box, lo, hi, "hollow box")[:, :, 1:dims[2] - 1].all()
    one = _check_fill(M, np.zeros((1, 1, 1), bool), (0, 0, 0), (1, 1, 1), "one empty cell")
    assert not one.any()


# ---- dilation ------------------------------------------------------------------------------------------------------------------

def _check_dilate(M, dense, lo, hi, radii, what):
    want = O.dilate(dense, radii)
    got = _grid(M, dense, lo, hi).dilated(radii)
    assert np.array_equal(_words(got), O.pack(want)), (what, dense.shape, radii)
    assert int(got._count.item()) == int(want.sum()), (what, radii)
    return want


@pytest.mark.parametrize("grid_name", sorted(GRIDS))
def test_dilation_equals_the_oracle(M, grid_name):
    dims, lo, hi = GRIDS[grid_name]
    rng = np.random.default_rng(31)
    sparse = rng.random(dims) < 0.01
    sparse[dims[0] // 2, dims[1] // 2, 31:33] = True                            # on both sides of a word boundary
    assert np.array_equal(_check_dilate(M, sparse, lo, hi, (0, 0, 0), "identity"), sparse)
    for radii in ((1, 2, 3), (0, 0, 33), (0, 0, 40), (2, 0, 31), (0, 1, 32), (1, 0, 64), 1):
        r3 = (radii,) * 3 if isinstance(radii, int) else radii
        _check_dilate(M, sparse, lo, hi, r3, "sparse")
    for radii in (dims, tuple(g + 5 for g in dims), (1 << 30, 1 << 30, (1 << 31) - 1)):
        one = np.zeros(dims, bool)
        one[0, dims[1] - 1, dims[2] // 2] = True
        assert _check_dilate(M, one, lo, hi, radii, "radii >= every side").all()  # a full grid, padding bits zero (the words are equal)
    for corner in np.ndindex(2, 2, 2):
        one = np.zeros(dims, bool)
        one[tuple(-c for c in corner)] = True                                   # index 0 or -1 on every axis
        for radii in ((1, 2, 3), (0, 0, 33), (0, 0, 40)):
            _check_dilate(M, one, lo, hi, radii, f"corner {corner}")
    assert not _check_dilate(M, np.zeros(dims, bool), lo, hi, (1, 2, 40), "empty").any()
    one = _check_dilate(M, np.ones((1, 1, 1), bool), (0, 0, 0), (1, 1, 1), (3, 3, 3), "one cell")
    assert one.all()


# ---- the Python surface ----------------------------------------------------------------------------------------------------------

def _body():
    """A closed shape well inside the unit box, in normalised coordinates."""
    return O.merge(O.icosphere(2, (0.0, 0.05, 0.1), 0.45), O.icosphere(1, (0.0, 0.0, -0.5), 0.25))


@pytest.mark.parametrize("grid_name", sorted(GRIDS))
def test_from_mesh_equals_its_three_steps_and_the_oracle(M, grid_name):
    dims, lo, hi = GRIDS[grid_name]
    centre, half = (np.asarray(lo) + np.asarray(hi)) / 2, (np.asarray(hi) - np.asarray(lo)) / 2
    verts, tris = _body()
    verts = (verts.astype(np.float64) * half + centre).astype(np.float32)
    tris = np.concatenate([tris, [[0, 0, 1], [0, 1, len(verts)]]])              # two skipped triangles
    v, t = _dev(verts), _dev(tris)
    cell = (np.asarray(hi, np.float32).astype(np.float64) - np.asarray(lo, np.float32).astype(np.float64)) / np.asarray(dims)
    for dilate, thickness, solid in ((1, 0.0, True), (0, 0.0, False), ((1, 0, 2), 0.2 * float(cell.max()) / 0.3, True), (2, float(cell[2]), False)):
        got, dropped = M.OccupancyGrid.from_mesh(v, t, [lo, hi], dims, dilate=dilate, thickness=thickness, solid=solid, return_dropped=True)
        radii = O.radii(dims, lo, hi, dilate, thickness)
        d3 = (dilate,) * 3 if isinstance(dilate, int) else dilate
        assert radii == tuple(d3[a] + int(np.ceil(thickness / cell[a])) for a in range(3))
        by_hand, dropped_by_hand = _surface(M, verts, tris, dims, lo, hi)
        if solid:
            by_hand = by_hand.filled()
        by_hand = by_hand.dilated(radii)
        assert torch.equal(got.bits, by_hand.bits) and torch.equal(got._count, by_hand._count)
        want, want_dropped = O.from_mesh(verts, tris, dims, lo, hi, dilate, thickness, solid)
        assert np.array_equal(_words(got), O.pack(want)) and dropped == dropped_by_hand == want_dropped == 2
        assert got.occupied_fraction() == want.sum() / want.size and got.dims == dims
        assert np.array_equal(got.lo, np.asarray(lo, np.float32)) and np.array_equal(got.hi, np.asarray(hi, np.float32))
    if grid_name == "aniso":                                                    # the thickness reaches further in cells along the short edges
        assert len(set(O.radii(dims, lo, hi, 0, 0.2))) > 1
    plain = M.OccupancyGrid.from_mesh(v, t, [lo, hi], dims)
    assert isinstance(plain, M.OccupancyGrid) and np.array_equal(_words(plain), O.pack(O.from_mesh(verts, tris, dims, lo, hi)[0]))


def test_from_smpl_equals_from_mesh_on_the_posed_vertices(M):
    from moco_flow_amd import smpl as S, synth
    model = synth.smpl_model(1, 6890)                                           # the synthetic body has no faces of its own
    m = S.SMPL(model=dict(model, f=synth.smpl_faces(model["v_template"]))).cuda()
    assert tuple(m.faces.shape) == (13776, 3) and m.faces.dtype == torch.int64
    pose, betas = synth.smpl_pose(5, batch=1, scale=0.6)
    pose, betas = torch.from_numpy(pose).cuda(), torch.from_numpy(betas).cuda()
    verts = m(pose, betas)[0]
    v = verts.cpu().numpy()
    aabb = np.stack([v.min(0) - 0.4, v.max(0) + 0.4])
    kw = dict(dims=(24, 28, 20), dilate=1, thickness=0.05)
    got = M.OccupancyGrid.from_smpl(m, pose, betas, aabb, **kw)
    by_hand = M.OccupancyGrid.from_mesh(verts, m.faces, aabb, **kw)
    assert torch.equal(got.bits, by_hand.bits) and torch.equal(got._count, by_hand._count)
    want, dropped = O.from_mesh(v, m.faces.cpu().numpy(), kw["dims"], aabb[0], aabb[1], kw["dilate"], kw["thickness"])
    assert np.array_equal(_words(got), O.pack(want)) and 0 < want.sum() < want.size
    # guarantee (a) on the body: every vertex's cell, and every cell within the thickness of it, is set
    lo32, hi32, inv = O.grid_constants(kw["dims"], aabb[0], aabb[1])
    c = O.cell_of(v, lo32, inv, kw["dims"])
    assert want[c[:, 0], c[:, 1], c[:, 2]].all()


def test_and_or_equal_dense_logic(M):
    dims, lo, hi = GRIDS["tail"]
    rng = np.random.default_rng(41)
    a, b = rng.random(dims) < 0.4, rng.random(dims) < 0.4
    ga, gb = _grid(M, a, lo, hi), _grid(M, b, lo, hi)
    both, either = ga & gb, ga | gb
    assert torch.equal(both.to_dense(), ga.to_dense() & gb.to_dense()) and np.array_equal(_words(both), O.pack(a & b))
    assert torch.equal(either.to_dense(), ga.to_dense() | gb.to_dense()) and np.array_equal(_words(either), O.pack(a | b))
    assert both._count is None and both.occupied_fraction() == (a & b).sum() / a.size
    assert both.dims == dims and np.array_equal(both.lo, ga.lo) and np.array_equal(either.hi, ga.hi)
    other_dims = _grid(M, np.zeros((7, 9, 36), bool), lo, hi)
    other_box = _grid(M, b, lo, (7.0, 9.0, 37.5))
    for bad in (other_dims, other_box, 3):
        with pytest.raises(RuntimeError):
            ga & bad
        with pytest.raises(RuntimeError):
            ga | bad


def test_refusals(M):
    dims, lo, hi = GRIDS["tail"]
    v, t = torch.zeros(4, 3, device="cuda"), torch.zeros(2, 3, dtype=torch.int64, device="cuda")
    G = M.OccupancyGrid
    for bad in dict(dims=0), dict(dims=(4, 4)), dict(dims=1025), dict(dims=2.5), dict(dilate=-1), dict(dilate=(1, 1)), dict(thickness=-0.1), \
            dict(thickness=float("nan")), dict(thickness=float("inf")):
        with pytest.raises(RuntimeError):
            G.from_mesh(v, t, [lo, hi], **bad)
    for args in ((v.double(), t), (v, t.int()), (v[:, :2], t), (v, t[:, :2]), (v.cpu(), t), (v, t.cpu())):
        with pytest.raises(RuntimeError):
            G.from_mesh(*args, [lo, hi])
    with pytest.raises(RuntimeError):
        G.from_mesh(v, t, [lo, lo])
    with pytest.raises(RuntimeError):
        G.from_mesh(v, t, [lo, hi, hi])
    grid = _grid(M, np.zeros(dims, bool), lo, hi)
    for bad in (-1, (1, 2), (1, -2, 3), 1.5, None):
        with pytest.raises(RuntimeError):
            grid.dilated(bad)


# ---- consumers -----------------------------------------------------------------------------------------------------------------

def _aimed_rays(R, lo, hi, seed):
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    target = rng.uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), (R, 3))
    o = rng.normal(0.0, 1.0, (R, 3))
    o = (lo + hi) / 2 + o / np.linalg.norm(o, axis=1, keepdims=True) * np.linalg.norm(hi - lo) * rng.uniform(0.6, 2.0, (R, 1))
    o[3::7] = rng.uniform(lo, hi, (len(o[3::7]), 3))                            # origins inside the box
    d = target - o
    dist = np.linalg.norm(d, axis=1)
    d32 = (d / dist[:, None]).astype(np.float32)
    d32 /= np.linalg.norm(d32, axis=1, keepdims=True)
    near, far = np.zeros(R), dist + np.linalg.norm(hi - lo)
    near[1::5] = (dist * rng.uniform(0.7, 1.2, R))[1::5]
    far[2::5] = (dist * rng.uniform(0.8, 1.3, R))[2::5]
    return np.concatenate([o, d32, near[:, None], far[:, None], np.full((R, 1), 0.25)], 1).astype(np.float32)


@pytest.mark.parametrize("grid_name", ["aniso", "whole"])
def test_clip_rays_on_a_mesh_grid_equals_the_march_on_the_oracles_bits(M, grid_name):
    dims, lo, hi = GRIDS[grid_name]
    centre, half = (np.asarray(lo) + np.asarray(hi)) / 2, (np.asarray(hi) - np.asarray(lo)) / 2
    verts, tris = _body()
    verts = (verts.astype(np.float64) * half * 0.7 + centre).astype(np.float32)
    grid = M.OccupancyGrid.from_mesh(_dev(verts), _dev(tris), [lo, hi], dims, dilate=1)
    dense = O.from_mesh(verts, tris, dims, lo, hi)[0]
    assert np.array_equal(_words(grid), O.pack(dense)) and 0 < dense.sum() < dense.size
    rays = _aimed_rays(3000, lo, hi, 7)
    lo32, hi32, inv, dt = RO.grid_constants(dims, grid.lo, grid.hi, 0.5)
    assert np.array_equal(inv, grid.inv_cell) and float(dt) == grid.step_length(0.5)
    want = RO.clip(rays, dense, lo32, hi32, inv, dt)
    got = grid.clip_rays(_dev(rays))
    assert 0 < want[2].sum() < len(rays)
    for g, w, name in zip(got, want, ("t_first", "t_last", "hit")):
        assert np.array_equal(g.cpu().numpy(), w, equal_nan=name != "hit"), name


def test_from_field_within_a_mesh_grid_equals_its_two_steps(M):
    case = dict(n=8, S=8, M=0, extra="dir", regime="dense", nof="none")
    embs, nerfs, _ = build_case(M, case, 0, device="cuda")
    aabb = np.array([[-0.9, -0.5, -1.1], [0.8, 0.6, 1.0]])
    n = (17, 14, 34)
    with torch.no_grad():
        sigma = M.query_sigma(M.OccupancyGrid.lattice(n, aabb, "cuda")[0], nerfs[0], embs[0], precision="f32")
    tau = float(np.median(np.log1p(np.exp(sigma.cpu().numpy().astype(np.float64)))))          # half the points active
    verts, tris = O.icosphere(2, (0.25, 0.2, -0.5), 0.28)
    mesh_grid = M.OccupancyGrid.from_mesh(_dev(verts), _dev(tris), aabb, (6, 5, 9), dilate=1)
    assert np.array_equal(_words(mesh_grid), O.pack(O.from_mesh(verts, tris, (6, 5, 9), aabb[0], aabb[1])[0]))
    axes = M.OccupancyGrid.lattice_axes(n, aabb)[0]
    vol, (K, nbk) = M.query_sigma_lattice(axes, nerfs[0], embs[0], mesh_grid, fill=float("-inf"), precision="f32", return_stats=True)
    assert 0 < K < nbk
    by_hand = M.OccupancyGrid.from_sigma(vol, aabb[0], aabb[1], tau, "softplus", 1)
    got = M.OccupancyGrid.from_field(nerfs[0], embs[0], aabb, N_grid=n, sigma_threshold=tau, precision="f32", within=mesh_grid)
    dense = M.OccupancyGrid.from_field(nerfs[0], embs[0], aabb, N_grid=n, sigma_threshold=tau, precision="f32")
    assert torch.equal(got.bits, by_hand.bits) and got.occupied_fraction() == by_hand.occupied_fraction()
    assert 0 < got.occupied_fraction() < dense.occupied_fraction()
    assert bool(((got.bits & ~dense.bits) == 0).all())                          # nothing the dense build does not have
