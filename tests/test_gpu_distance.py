"""The Euclidean shell and the distance field on the MI355X: mf_grid_edt (csrc/mf_distance.hip) and OccupancyGrid.squared_distance /
dilated_euclidean / from_mesh(shell="euclidean") / from_smpl against the numpy oracle of their contract (tests/distance_oracle.py:
brute force over the set cells).  Every result is defined in integers: words (padding bits included), d2 and counts are compared
for equality, with no tolerance and nothing left out.

Launch shape: none of the unit's kernels has a grid-stride loop -- a wave owns 64 consecutive cells of one row, a workgroup
kEdtThreads / 64 such pieces -- so there is no second trip to reach; the (40, 40, 70) grid runs 800 workgroups, rows of two pieces
with a tail, and a count gathered from more partials than the finishing workgroup has threads."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import distance_oracle as D
import occupancy_oracle as RO
import voxelize_oracle as VO
from test_distance_cpu import GRIDS, TABLE, sparse_cells
from test_gpu_voxelize import _aimed_rays, _surface

pytestmark = pytest.mark.gpu

_SRC = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "moco_flow_amd", "csrc", "mf_distance.hip")).read()
THREADS = int(re.search(r"\bconstexpr int kEdtThreads = (\d+);", _SRC).group(1))
BIG = (40, 40, 70)


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
    return M.OccupancyGrid(_dev(VO.pack(dense).view(np.int32)), dense.shape, lo, hi)


def _edt(M, dense, w, R, d2=True, bits=True, count=True):
    """mf_grid_edt alone, on outputs filled with ones beforehand: (d2 int32 array, words uint32 array, count int), None where
    the output was not asked for."""
    dims = dense.shape
    src = _dev(VO.pack(dense).view(np.int32))
    lib = M._lib.lib()
    scratch = torch.full((int(lib.mf_grid_edt_scratch_bytes(*dims)),), 0xFF, dtype=torch.uint8, device="cuda")
    d2_t = torch.full(dims, -1, dtype=torch.int32, device="cuda") if d2 else None
    out_t = torch.full(tuple(src.shape), -1, dtype=torch.int32, device="cuda") if bits else None
    cnt_t = torch.full((1,), -7, dtype=torch.int64, device="cuda") if count else None
    ptr = lambda t: None if t is None else t.data_ptr()
    rc = lib.mf_grid_edt(src.data_ptr(), *dims, (ctypes.c_int32 * 3)(*w), R, ptr(d2_t), ptr(out_t), ptr(cnt_t), scratch.data_ptr(),
                         torch.cuda.current_stream().cuda_stream)
    M._lib.check(rc, "mf_grid_edt")
    return (None if d2_t is None else d2_t.cpu().numpy(), None if out_t is None else out_t.cpu().numpy().view(np.uint32),
            None if cnt_t is None else int(cnt_t.item()))


def _check(M, dense, w, R, what):
    want = D.squared_distance(dense, w, R)
    d2, words, count = _edt(M, dense, w, R)
    assert d2.dtype == np.int32 and np.array_equal(d2, want), (what, dense.shape, int((d2 != want).sum()))
    assert np.array_equal(words, VO.pack(want <= R)), (what, dense.shape)
    assert count == int((want <= R).sum()), (what, count)
    return want


@functools.lru_cache(maxsize=None)
def _wide(name):
    """A metric whose reach exceeds every side of the grid."""
    dims, lo, hi = GRIDS[name]
    m = D.euclid_metric(D.cell_edges(dims, lo, hi), 1.05 * float(np.max(np.asarray(hi) - np.asarray(lo))))
    assert all(m[2][a] >= dims[a] for a in range(3))
    return m


@pytest.mark.parametrize("name", sorted(GRIDS))
def test_d2_words_and_count_equal_the_oracle(M, name):
    dims, lo, hi = GRIDS[name]
    t, w, R, r = TABLE[name]
    assert D.euclid_metric(D.cell_edges(dims, lo, hi), t) == (w, R, r)
    random, hand = sparse_cells(dims)
    for what, dense in (("random", random), ("hand-placed", hand), ("both", random | hand)):
        want = _check(M, dense, w, R, what)
        assert 0 < (want <= R).sum() < want.size and (want == R + 1).any()
    for corner in np.ndindex(2, 2, 2):
        one = np.zeros(dims, dtype=bool)
        one[tuple(-c for c in corner)] = True
        _check(M, one, w, R, f"corner {corner}")
    # an empty grid: R + 1 everywhere, zero words, count 0; a full grid: 0 everywhere
    want = _check(M, np.zeros(dims, bool), w, R, "empty")
    assert (want == R + 1).all()
    want = _check(M, np.ones(dims, bool), w, R, "full")
    assert (want == 0).all()
    # radius 0 is the identity
    want = _check(M, random | hand, w, 0, "radius 0")
    assert np.array_equal(want == 0, random | hand) and (want <= 1).all()
    # a reach beyond every side
    ww, wR, wr = _wide(name)
    _check(M, hand, ww, wR, "wide")
    _check(M, random, ww, wR, "wide")
    one = np.zeros(dims, dtype=bool)
    one[0, dims[1] - 1, dims[2] // 2] = True
    _check(M, one, ww, wR, "wide, one cell")


def test_a_grid_of_one_cell(M):
    for dense in (np.ones((1, 1, 1), bool), np.zeros((1, 1, 1), bool)):
        for R in (0, 5, (1 << 30) - 1):
            want = _check(M, dense, (65536, 1, 300), R, "one cell")
            assert want[0, 0, 0] == (0 if dense.any() else R + 1)


def test_either_output_alone_equals_both(M):
    dims, lo, hi = GRIDS["tail"]
    t, w, R, r = TABLE["tail"]
    random, hand = sparse_cells(dims)
    dense = random | hand
    d2, words, count = _edt(M, dense, w, R)
    only_d2 = _edt(M, dense, w, R, bits=False, count=False)
    assert np.array_equal(only_d2[0], d2) and only_d2[1] is None and only_d2[2] is None
    only_bits = _edt(M, dense, w, R, d2=False)
    assert only_bits[0] is None and np.array_equal(only_bits[1], words) and only_bits[2] == count
    no_count = _edt(M, dense, w, R, d2=False, count=False)
    assert np.array_equal(no_count[1], words) and no_count[2] is None


@functools.lru_cache(maxsize=None)
def _big_case():
    lo, hi = (-0.9371, -0.4113, -1.2837), (0.7129, 0.5291, 1.1173)
    dense = np.random.default_rng(5).random(BIG) < 0.003
    dense[20, 20, 63:66] = True                                              # across the seam between a row's two pieces
    dense[0, 0, 69] = dense[39, 39, 0] = True
    w, R, r = D.euclid_metric(D.cell_edges(BIG, lo, hi), 0.21)
    assert min(r) >= 3 and len(set(w)) == 3
    return dense, lo, hi, w, R, D.squared_distance(dense, w, R)


def test_many_workgroups_two_runs_and_a_side_stream(M):
    dense, lo, hi, w, R, want = _big_case()
    pieces = BIG[0] * BIG[1] * ((BIG[2] + 63) // 64)
    assert pieces // (THREADS // 64) > THREADS                               # more partial counts than one thread each in the finish
    first = _edt(M, dense, w, R)
    assert np.array_equal(first[0], want) and np.array_equal(first[1], VO.pack(want <= R)) and first[2] == int((want <= R).sum())
    assert 0 < first[2] < want.size
    second = _edt(M, dense, w, R)
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1]) and first[2] == second[2]
    grid = _grid(M, dense, lo, hi)
    d2_main, w_main, R_main = grid.squared_distance(0.21)
    shell_main = grid.dilated_euclidean(0.21)
    assert (w_main, R_main) == (w, R) and np.array_equal(d2_main.cpu().numpy(), want)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        d2_side = grid.squared_distance(0.21)[0]
        shell_side = grid.dilated_euclidean(0.21)
    side.synchronize()
    assert torch.equal(d2_side, d2_main) and torch.equal(shell_side.bits, shell_main.bits) and torch.equal(shell_side._count, shell_main._count)
    assert np.array_equal(_words(shell_main), first[1]) and int(shell_main._count.item()) == first[2]


@pytest.mark.parametrize("name", sorted(GRIDS))
def test_python_methods_equal_the_oracle(M, name):
    dims, lo, hi = GRIDS[name]
    t, w, R, r = TABLE[name]
    random, hand = sparse_cells(dims)
    dense = random | hand
    grid = _grid(M, dense, lo, hi)
    d2, gw, gR = grid.squared_distance(t)
    assert (gw, gR) == (w, R) and d2.dtype == torch.int32 and tuple(d2.shape) == dims and d2.device == grid.device
    want = D.squared_distance(dense, w, R)
    assert np.array_equal(d2.cpu().numpy(), want)
    shell = grid.dilated_euclidean(t)
    assert np.array_equal(_words(shell), VO.pack(want <= R)) and int(shell._count.item()) == int((want <= R).sum())
    assert shell.dims == dims and np.array_equal(shell.lo, grid.lo) and np.array_equal(shell.hi, grid.hi)
    assert shell.occupied_fraction() == (want <= R).sum() / want.size
    same = grid.dilated_euclidean(0.0)
    assert torch.equal(same.bits, grid.bits) and int(same._count.item()) == int(dense.sum())
    # re-thresholding the field at a smaller radius is the dilation at that radius
    w2, R2, _ = D.euclid_metric(grid.cell, 0.6 * t)
    assert w2 == w and np.array_equal(VO.pack(d2.cpu().numpy() <= R2), _words(grid.dilated_euclidean(0.6 * t)))


# ---- from_mesh ---------------------------------------------------------------------------------------------------------------------

def _shapes():
    return {"icosphere": VO.icosphere(2, (0.0, 0.05, 0.1), 0.45), "torus": VO.torus(0.42, 0.2, center=(0.02, -0.03, 0.01))}


def _placed(verts, lo, hi, scale=0.7):
    centre, half = (np.asarray(lo) + np.asarray(hi)) / 2, (np.asarray(hi) - np.asarray(lo)) / 2
    return (verts.astype(np.float64) * half * scale + centre).astype(np.float32)


@pytest.mark.parametrize("name", sorted(GRIDS))
def test_from_mesh_euclidean_equals_its_four_steps_and_the_oracle(M, name):
    dims, lo, hi = GRIDS[name]
    t, w, R, r = TABLE[name]
    G = M.OccupancyGrid
    for what, (verts, tris) in _shapes().items():
        verts = _placed(verts, lo, hi)
        v, f = _dev(verts), _dev(tris)
        for dilate, thickness, solid in ((1, t, True), ((1, 0, 2), 0.5 * t, False), (0, 0.0, True)):
            got, dropped = G.from_mesh(v, f, [lo, hi], dims, dilate=dilate, thickness=thickness, solid=solid, return_dropped=True,
                                       shell="euclidean")
            d3 = (dilate,) * 3 if isinstance(dilate, int) else dilate
            by_hand, dropped_by_hand = _surface(M, verts, tris, dims, lo, hi)                       # mf_voxel_mesh alone
            filled = by_hand.filled() if solid else by_hand
            by_hand = filled.dilated_euclidean(thickness).dilated(tuple(d + 1 for d in d3))
            assert torch.equal(got.bits, by_hand.bits) and torch.equal(got._count, by_hand._count), (what, dilate)
            want, want_dropped = D.from_mesh_euclidean(verts, tris, dims, lo, hi, dilate, thickness, solid)
            assert np.array_equal(_words(got), VO.pack(want)) and dropped == dropped_by_hand == want_dropped == 0, (what, dilate)
            assert got.occupied_fraction() == want.sum() / want.size and want.any()
            # contained in the box dilation by r_a + dilate_a + 1 of the filled surface
            reach = G.euclid_metric(got.cell, thickness)[2]
            outer = filled.dilated(tuple(reach[a] + d3[a] + 1 for a in range(3)))
            assert bool(((got.bits & ~outer.bits) == 0).all()), (what, dilate)


@pytest.mark.parametrize("name", sorted(GRIDS))
def test_the_box_shell_is_the_default_and_unchanged(M, name):
    dims, lo, hi = GRIDS[name]
    t = TABLE[name][0]
    for what, (verts, tris) in _shapes().items():
        verts = _placed(verts, lo, hi)
        v, f = _dev(verts), _dev(tris)
        for kw in (dict(), dict(dilate=1, thickness=t), dict(dilate=(1, 0, 2), thickness=0.5 * t, solid=False)):
            plain = M.OccupancyGrid.from_mesh(v, f, [lo, hi], dims, **kw)
            box = M.OccupancyGrid.from_mesh(v, f, [lo, hi], dims, shell="box", **kw)
            want = VO.from_mesh(verts, tris, dims, lo, hi, kw.get("dilate", 1), kw.get("thickness", 0.0), kw.get("solid", True))[0]
            assert torch.equal(plain.bits, box.bits) and torch.equal(plain._count, box._count), (what, kw)
            assert np.array_equal(_words(plain), VO.pack(want)), (what, kw)


def test_from_smpl_passes_the_shell_on(M):
    from moco_flow_amd import smpl as S, synth
    model = synth.smpl_model(1, 6890)
    m = S.SMPL(model=dict(model, f=synth.smpl_faces(model["v_template"]))).cuda()
    pose, betas = synth.smpl_pose(5, batch=1, scale=0.6)
    pose, betas = torch.from_numpy(pose).cuda(), torch.from_numpy(betas).cuda()
    verts = m(pose, betas)[0]
    v = verts.cpu().numpy()
    aabb = np.stack([v.min(0) - 0.4, v.max(0) + 0.4])
    kw = dict(dims=(24, 28, 20), dilate=1, thickness=0.2, shell="euclidean")
    got = M.OccupancyGrid.from_smpl(m, pose, betas, aabb, **kw)
    by_hand = M.OccupancyGrid.from_mesh(verts, m.faces, aabb, **kw)
    assert torch.equal(got.bits, by_hand.bits) and torch.equal(got._count, by_hand._count)
    want, _ = D.from_mesh_euclidean(v, m.faces.cpu().numpy(), kw["dims"], aabb[0], aabb[1], 1, 0.2)
    assert np.array_equal(_words(got), VO.pack(want)) and 0 < want.sum() < want.size
    box = M.OccupancyGrid.from_smpl(m, pose, betas, aabb, dims=kw["dims"], dilate=1, thickness=0.2)
    assert not torch.equal(box.bits, got.bits)


@pytest.mark.parametrize("name", ["aniso", "whole"])
def test_clip_rays_on_a_euclidean_grid_equals_the_march_on_the_oracles_bits(M, name):
    dims, lo, hi = GRIDS[name]
    verts, tris = _shapes()["icosphere"]
    verts = _placed(verts, lo, hi, 0.5)
    thickness = 0.5 * TABLE[name][0]
    grid = M.OccupancyGrid.from_mesh(_dev(verts), _dev(tris), [lo, hi], dims, dilate=1, thickness=thickness, shell="euclidean")
    dense = D.from_mesh_euclidean(verts, tris, dims, lo, hi, 1, thickness)[0]
    assert np.array_equal(_words(grid), VO.pack(dense)) and 0 < dense.sum() < dense.size
    rays = _aimed_rays(3000, lo, hi, 7)
    lo32, hi32, inv, dt = RO.grid_constants(dims, grid.lo, grid.hi, 0.5)
    assert np.array_equal(inv, grid.inv_cell) and float(dt) == grid.step_length(0.5)
    want = RO.clip(rays, dense, lo32, hi32, inv, dt)
    got = grid.clip_rays(_dev(rays))
    assert 0 < want[2].sum() < len(rays)
    for g, w, what in zip(got, want, ("t_first", "t_last", "hit")):
        assert np.array_equal(g.cpu().numpy(), w, equal_nan=what != "hit"), what


def test_refusals(M):
    dims, lo, hi = GRIDS["tail"]
    v, t = torch.zeros(4, 3, device="cuda"), torch.zeros(2, 3, dtype=torch.int64, device="cuda")
    G = M.OccupancyGrid
    for bad in ("ball", "Euclidean", "", None, 1):
        with pytest.raises(RuntimeError):
            G.from_mesh(v, t, [lo, hi], dims, shell=bad)
    with pytest.raises(RuntimeError):
        G.from_mesh(v, t, [lo, hi], dims, thickness=128.0, shell="euclidean")                  # R = 2^30 on unit cells
    grid = _grid(M, np.zeros(dims, bool), lo, hi)
    for bad in (-0.1, float("nan"), float("inf"), -float("inf"), 128.0, 1e30):
        with pytest.raises(RuntimeError):
            grid.squared_distance(bad)
        with pytest.raises(RuntimeError):
            grid.dilated_euclidean(bad)
    assert grid.squared_distance(127.99)[2] < 1 << 30
