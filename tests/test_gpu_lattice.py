"""Sparse lattice queries on the device (-m gpu): mf_lattice_select / _points / _scatter against tests/lattice_oracle.py, exactly
-- integer decisions on host-built tables and copies, so there is no tolerance --, query_sigma_lattice against the dense
query_sigma on the same lattice (bit-identical in the active bricks: every point-query kernel computes a sample's column
independently of its place in the batch; `fill` everywhere else), and the callers: extract_mesh / extract_colored_mesh behind a
grid and OccupancyGrid.from_field(within=...) against their dense runs.  The shapes of the "past" tests are derived from the
launch constants of csrc/mf_lattice.hip: select where the scan over the workgroups' counts crosses a wave and gives a thread
several entries (up to the 512^3 lattice), scatter past one trip of either loop, one query with all of them at once."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import lattice_oracle as LO
import occupancy_oracle as O
from helpers import build_case
from streams_util import HOLD_MS, first_done, hold, independent_streams, poison

pytestmark = pytest.mark.gpu

IND_SCALAR = -0.25
UNTOUCHED = -7

_SRC = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "moco_flow_amd", "csrc", "mf_lattice.hip")).read()


def _const(name):
    """An integer launch constant of csrc/mf_lattice.hip, `N` or `1 << N`."""
    m = re.search(r"\bconstexpr int %s = (?:(\d+) << )?(\d+);" % name, _SRC)
    return int(m.group(2)) if m.group(1) is None else int(m.group(1)) << int(m.group(2))


LAT_THREADS = _const("kLatThreads")                                     # bricks per workgroup of select, lanes per row of scatter
SCATTER_MAX_BLOCKS = _const("kLatScatterMaxBlocks")                     # rows of the volume per trip of scatter


@pytest.fixture(scope="module")
def M():
    import moco_flow_amd
    assert torch.cuda.is_available()
    moco_flow_amd._lib.lib()
    return moco_flow_amd


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _grid(M, dense, lo, hi):
    """The OccupancyGrid that holds the bool array ``dense`` (Gx, Gy, Gz)."""
    return M.OccupancyGrid(_dev(O.pack(dense).view(np.int32)), dense.shape, lo, hi)


def _i3(v):
    return (ctypes.c_int32 * 3)(*v)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _select(M, grid, axes, woa, margin):
    """mf_lattice_select through the raw entry, on the tables the package builds: (slot, brick_ids (all nb entries), K)."""
    from moco_flow_amd.points import brick_cell_ranges
    L = M._lib
    lib = L.lib()
    n = [len(a) for a in axes]
    tabs = [_dev(brick_cell_ranges(axes[a], margin, grid.lo[w], grid.hi[w], grid.inv_cell[w], grid.dims[w])) for a, w in enumerate(woa)]
    nbk = int(np.prod(LO.n_bricks(n)))
    slot = torch.full((nbk,), UNTOUCHED, dtype=torch.int32, device="cuda")
    ids = torch.full((nbk,), UNTOUCHED, dtype=torch.int32, device="cuda")
    count = torch.full((1,), UNTOUCHED, dtype=torch.int64, device="cuda")
    scratch = torch.empty(int(lib.mf_lattice_select_scratch_bytes(*n)), dtype=torch.uint8, device="cuda")
    L.check(lib.mf_lattice_select(grid.bits.data_ptr(), *grid.dims, *(t.data_ptr() for t in tabs), *n, _i3(woa), slot.data_ptr(),
                                  ids.data_ptr(), count.data_ptr(), scratch.data_ptr(), _stream()), "mf_lattice_select")
    return slot.cpu().numpy(), ids.cpu().numpy(), int(count.item())


def _oracle_select(dense, lo, hi, axes, woa, margin, select=LO.select):
    lo32, hi32, inv, _ = O.grid_constants(dense.shape, lo, hi, 0.5)
    return select(dense, LO.range_tables(axes, margin, dense.shape, lo32, hi32, inv, woa), [len(a) for a in axes], woa)


def _check_select(M, dense, lo, hi, axes, woa, margin, what, want=None):
    grid = _grid(M, dense, lo, hi)
    want_slot, want_ids, want_K = _oracle_select(dense, lo, hi, axes, woa, margin) if want is None else want
    slot, ids, K = _select(M, grid, axes, woa, margin)
    assert K == want_K, (what, K, want_K)
    assert np.array_equal(slot, want_slot), what
    assert np.array_equal(ids[:K], want_ids) and (ids[K:] == UNTOUCHED).all(), what
    return K, len(slot)


def _axes(n, lo=(-1.0, -1.0, -1.0), hi=(1.0, 1.0, 1.0)):
    return [np.linspace(lo[a], hi[a], n[a]).astype(np.float32) for a in range(3)]


# ------------------------------------------------------------------------------------------------ select
BOX_LO, BOX_HI = (-0.4, -1.2, -0.1), (0.7, 0.3, 2.0)                # covers the lattice [-1, 1]^3 only partly, overhangs it in y and z


@pytest.mark.parametrize("woa", [(0, 1, 2), (1, 0, 2)])
def test_select_equals_the_oracle(M, woa):
    """Lattice (19, 13, 21) -- distinct sides, a partial brick on every axis -- against a grid of (5, 4, 7) cells over a box that
    covers it partly: slot, brick_ids and K at densities 0, 0.1 and 1 and margins 0, 1, 2."""
    axes = _axes((19, 13, 21))
    seen = set()
    for density in (0.0, 0.1, 1.0):
        rng = np.random.default_rng(int(density * 10) + 17)
        dense = rng.random((5, 4, 7)) < density
        for margin in (0, 1, 2):
            K, nbk = _check_select(M, dense, BOX_LO, BOX_HI, axes, woa, margin, (woa, density, margin))
            assert nbk == 3 * 2 * 3
            seen.add((density, K))
            if density == 0.0:
                assert K == 0
            if density == 1.0:
                assert 0 < K <= nbk and (margin > 0 or K < nbk)         # margin 0: the bricks outside the box stay inactive
    assert any(0 < K < 18 for d, K in seen if d == 0.1)


@pytest.mark.parametrize("n", [(8, 16, 8), (2, 2, 2), (9, 2, 65), (70, 60, 50)])
def test_select_on_further_lattice_shapes(M, n):
    """Whole bricks only; one brick; a single-point last brick with 9 bricks along the fast axis; and 9 x 8 x 7 = 504 bricks:
    two workgroups, eight waves, the scan over more than one count."""
    rng = np.random.default_rng(sum(n))
    dense = rng.random((5, 4, 7)) < 0.15
    for woa in ((0, 1, 2), (2, 0, 1)):
        for margin in (0, 1):
            K, nbk = _check_select(M, dense, BOX_LO, BOX_HI, _axes(n), woa, margin, (n, woa, margin))
    if n == (70, 60, 50):
        assert nbk == 504 and 0 < K < nbk


def test_select_under_a_grid_finer_than_the_lattice(M):
    """40^3 cells over a 12^3 lattice: a brick's cell box spans two words along z and many rows."""
    rng = np.random.default_rng(40)
    dense = rng.random((40, 40, 40)) < 0.0004
    assert 8 < dense.sum() < 60
    lo, hi = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
    for margin in (0, 1):
        for woa in ((0, 1, 2), (1, 0, 2)):
            K, nbk = _check_select(M, dense, lo, hi, _axes((12, 12, 12)), woa, margin, (margin, woa))
            assert nbk == 8
    one = np.zeros((40, 40, 40), dtype=bool)
    one[39, 0, 33] = True                                               # the second word of a row, the last x, the first y
    K, _ = _check_select(M, one, lo, hi, _axes((12, 12, 12)), (0, 1, 2), 0, "one cell")
    assert K == 1
    K, _ = _check_select(M, one, lo, hi, _axes((12, 12, 12)), (1, 0, 2), 0, "one cell, xy")
    assert K == 1


# ------------------------------------------------------------------------------------------------ select: the scan's tiers
# lat_scan_kernel scans one count per workgroup of LAT_THREADS bricks with LAT_THREADS threads (scan_totals<kLatThreads, 1>,
# csrc/mf_scan.hpp): thread t owns `per` = ceil(counts / LAT_THREADS) entries from t * per on.  The shapes follow from the
# constant; each case asserts the tier it was built for, so another constant fails the case and does not empty it.
T_ = LAT_THREADS
SELECT_TIERS = {
    # name: (lattice, thin, counts, per); thin: the short axis covers one or two cells and not the whole grid
    "wave": ((4 * T_ + 1, 4 * T_ + 1, 1), False, None, 1),             # more counts than a wave has lanes: the waves-in-front term
    "full": ((8 * T_, 8 * T_, 8), True, T_, 1),                         # every scan thread holds exactly one count
    "odd": ((8 * T_ - 7, 8 * T_ + 1, 3), True, T_ + 1, 2),              # two per thread, the last owner holds a single one
    "idle": ((8 * T_ + 1, 8 * T_ + 1, 1), False, None, 2),              # two per thread, the upper threads own nothing
    "512": ((2 * T_, 2 * T_, 2 * T_), False, 4 * T_, 4),                # the 512^3 lattice of a fine extraction
}
SELECT_WOA = ((0, 1, 2), (2, 0, 1))


@functools.lru_cache(maxsize=None)
def select_tier_case(name, woa, margin):
    """(dense, lo, hi, axes, the oracle's (slot, brick_ids, K)) of one tier, with the properties the case is for asserted on
    the ORACLE's result: nothing here has seen the device."""
    n, thin, counts, per = SELECT_TIERS[name]
    dense = np.random.default_rng(40).random((40, 40, 40)) < 0.2
    lo, hi = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
    axes = _axes(n, (-1.0, -1.0, -0.02 if thin else -1.0), (1.0, 1.0, 0.02 if thin else 1.0))
    bricks = int(np.prod(LO.n_bricks(n)))
    nblocks = -(-bricks // LAT_THREADS)
    assert nblocks > 64 and -(-nblocks // LAT_THREADS) == per and (counts is None or nblocks == counts), (name, bricks, nblocks)
    owners = -(-nblocks // per)                                         # scan threads with at least one entry
    if name == "wave":
        assert nblocks <= LAT_THREADS
    if name == "full":
        assert bricks == LAT_THREADS * LAT_THREADS and owners == LAT_THREADS
    if name == "odd":
        assert nblocks % 2 == 1 and bricks % LAT_THREADS == 0
    if name == "idle":
        assert owners < LAT_THREADS - 64 and bricks % LAT_THREADS != 0  # a whole wave of idle threads, a ragged last workgroup
    if name == "512":
        assert n == (512, 512, 512) and owners == LAT_THREADS
    slot, ids, K = want = _oracle_select(dense, lo, hi, axes, woa, margin, LO.select_fast)
    on = np.zeros(nblocks * LAT_THREADS, dtype=np.int64)
    on[:bricks] = slot >= 0
    per_group = on.reshape(nblocks, LAT_THREADS).sum(1)
    assert per_group.sum() == K and len(slot) == bricks
    assert 0.1 < K / bricks < 0.9, (name, woa, margin, K / bricks)
    assert (per_group > 0).sum() >= 0.75 * nblocks, (name, woa, margin)
    assert len(np.unique(per_group)) >= 16, (name, woa, margin)
    return dense, lo, hi, axes, want


@pytest.mark.parametrize("name", list(SELECT_TIERS))
def test_select_past_one_count_per_lane_wave_and_thread(M, name):
    """slot, brick_ids and K where the scan over the workgroups' counts crosses a wave (more than 64 counts), fills every
    thread (LAT_THREADS counts), gives a thread several entries (more than LAT_THREADS: an odd number of counts, idle upper
    threads) and at the 512^3 lattice's 1024 counts, under two world_of_axis and margins 0 and 1.  The flat lattices cost
    nothing: select reads the per-axis tables only.  The oracle is LO.select_fast, which tests/test_lattice_cpu.py holds to
    LO.select."""
    for woa in SELECT_WOA:
        for margin in (0, 1):
            dense, lo, hi, axes, want = select_tier_case(name, woa, margin)
            K, nbk = _check_select(M, dense, lo, hi, axes, woa, margin, (name, woa, margin), want=want)
            print(f"\nselect tier {name} {woa} margin {margin}: {K} of {nbk} bricks")


# ------------------------------------------------------------------------------------------------ points and scatter
def _points(M, ids, axes, woa):
    L = M._lib
    n = [len(a) for a in axes]
    K = len(ids)
    out = torch.full((K * 512, 3), float("nan"), device="cuda")
    ax = [_dev(a) for a in axes]
    L.check(L.lib().mf_lattice_points(_dev(ids).data_ptr() if K else None, K, *(t.data_ptr() for t in ax), *n, _i3(woa),
                                      out.data_ptr() if K else None, _stream()), "mf_lattice_points")
    return out.cpu().numpy()


def _scatter(M, sigma, slot, K, n, fill):
    L = M._lib
    vol = torch.full(tuple(n), float("nan"), device="cuda")
    sig = _dev(sigma) if K else None
    L.check(L.lib().mf_lattice_scatter(sig.data_ptr() if K else None, _dev(slot).data_ptr(), K, *n, fill, vol.data_ptr(), _stream()),
            "mf_lattice_scatter")
    return vol.cpu().numpy()


def _points_and_scatter(M, n, woas):
    rng = np.random.default_rng(sum(n) + 1)
    nb = LO.n_bricks(n)
    on = rng.random(nb[0] * nb[1] * nb[2]) < 0.5
    on[-1] = True                                                       # the brick that is partial on every axis
    on[0] = False
    ids = np.nonzero(on)[0].astype(np.int32)
    slot = np.where(on, np.cumsum(on) - 1, -1).astype(np.int32)
    K = len(ids)
    axes = [np.sort(rng.normal(size=v)).astype(np.float32) for v in n]   # uneven spacing
    for woa in woas:
        got, want = _points(M, ids, axes, woa), LO.points(ids, axes, woa)
        assert got.shape == want.shape and np.array_equal(got.view(np.int32), want.view(np.int32)), woa
    sigma = rng.normal(size=K * 512).astype(np.float32)
    sigma[::97] = np.nan
    sigma[5::101] = -0.0
    mask = LO.active_mask(slot, n)
    for fill in (float("-inf"), 0.0):
        got, want = _scatter(M, sigma, slot, K, n, fill), LO.scatter(sigma, slot, n, np.float32(fill))
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), fill
        assert 0 < mask.sum() < mask.size and (got[~mask].view(np.int32) == np.float32(fill).view(np.int32)).all()
    return K


@pytest.mark.parametrize("n", [(19, 13, 21), (9, 2, 65), (8, 16, 8)])
def test_points_and_scatter_equal_the_oracle_bit_for_bit(M, n):
    _points_and_scatter(M, n, ((0, 1, 2), (1, 0, 2), (2, 1, 0)))


# lat_scatter_kernel: one workgroup per (i0, i1) row and trip, at most SCATTER_MAX_BLOCKS workgroups, LAT_THREADS lanes along i2
SCATTER_LONG = (9, 10, 2 * LAT_THREADS + 91)                            # three trips along i2, the last ragged, on a few rows
SCATTER_ROWS = (SCATTER_MAX_BLOCKS // 258 + 3, 258, 9)                  # a second trip over the rows for some workgroups only
SCATTER_BOTH = (SCATTER_MAX_BLOCKS // 250 + 3, 250, LAT_THREADS + 3)


@pytest.mark.parametrize("n", [SCATTER_LONG, SCATTER_ROWS, SCATTER_BOTH], ids=["long_rows", "many_rows", "both"])
def test_points_and_scatter_past_their_first_trips(M, n):
    """The same check where a row of the volume is longer than the workgroup (a second and third trip of the i2 loop), where
    the volume has more rows than the grid has workgroups (a second trip of the row loop, taken by the first workgroups
    only), and both at once; every side ends in a partial brick."""
    rows, trips2 = n[0] * n[1], -(-n[2] // LAT_THREADS)
    assert all(v % 8 for v in n), n
    if n == SCATTER_LONG:
        assert trips2 == 3 and n[2] % LAT_THREADS and rows < SCATTER_MAX_BLOCKS
    if n == SCATTER_ROWS:
        assert SCATTER_MAX_BLOCKS < rows < 2 * SCATTER_MAX_BLOCKS and trips2 == 1
    if n == SCATTER_BOTH:
        assert SCATTER_MAX_BLOCKS < rows < 2 * SCATTER_MAX_BLOCKS and trips2 == 2
    K = _points_and_scatter(M, n, ((2, 0, 1),))
    assert K > 0.4 * np.prod(LO.n_bricks(n))


def test_a_launch_with_no_active_brick(M):
    n = (19, 13, 21)
    dense = np.zeros((5, 4, 7), dtype=bool)
    slot, ids, K = _select(M, _grid(M, dense, BOX_LO, BOX_HI), _axes(n), (0, 1, 2), 1)
    assert K == 0 and (slot == -1).all() and (ids == UNTOUCHED).all()
    assert _points(M, ids[:0], _axes(n), (0, 1, 2)).shape == (0, 3)
    for fill in (float("-inf"), 0.0, 2.5):
        vol = _scatter(M, None, slot, 0, n, fill)
        assert vol.shape == n and (vol == np.float32(fill)).all()


# ------------------------------------------------------------------------------------------------ query_sigma_lattice
LATTICE = (19, 13, 21)


def _ball_grid(M, dims=(16, 16, 16), lo=(-1.0, -1.0, -1.0), hi=(1.0, 1.0, 1.0), center=(-0.3, 0.25, -0.4), radius=0.35):
    s = O.ball_lattice(tuple(d + 1 for d in dims), lo, hi, center, radius)
    dense = O.build_dense(s, "relu", 1.0, 0)
    assert 0 < dense.sum() < dense.size
    return _grid(M, dense, lo, hi), dense


def _dense_points(axes, woa):
    g = np.meshgrid(*axes, indexing="ij")
    pts = np.zeros(g[0].shape + (3,), dtype=np.float32)
    for a in range(3):
        pts[..., woa[a]] = g[a]
    return pts.reshape(-1, 3)


@pytest.mark.parametrize("prec,nof,woa", [("f32", "none", (0, 1, 2)), ("f32", "bw", (1, 0, 2)), ("bf16", "none", (1, 0, 2)),
                                           ("bf16x3", "none", (0, 1, 2))])
def test_query_sigma_lattice_equals_the_dense_query_in_active_bricks(M, prec, nof, woa):
    """Points of active bricks: bit-identical to query_sigma on the whole lattice (the same networks, the same precision);
    all other points: fill.  Also through two-brick chunks (several query_sigma calls), bit for bit the same volume."""
    case = dict(n=8, S=8, M=0, extra="ind" if nof == "bw" else "dir", regime="dense", nof=nof)
    embs, nerfs, kw = build_case(M, case, 0, device="cuda")
    flow = dict(bw_nof=kw["nof_models"][0], nof_embeddings=kw["nof_embeddings"], ind=IND_SCALAR) if nof == "bw" else {}
    grid, dense = _ball_grid(M)
    axes = _axes(LATTICE, (-0.9, -1.0, -0.8), (0.8, 0.7, 1.0))
    with torch.no_grad():
        want = M.query_sigma(_dev(_dense_points(axes, woa)), nerfs[0], embs[0], precision=prec, **flow).view(*LATTICE)
    lo32, hi32, inv, _ = O.grid_constants(dense.shape, grid.lo, grid.hi, 0.5)
    slot, ids, K = LO.select(dense, LO.range_tables(axes, 1, dense.shape, lo32, hi32, inv, woa), LATTICE, woa)
    mask = _dev(LO.active_mask(slot, LATTICE))
    for fill in (float("-inf"), 0.0):
        vol, (k, nbk) = M.query_sigma_lattice(axes, nerfs[0], embs[0], grid, world_of_axis=woa, margin=1, fill=fill, precision=prec,
                                              return_stats=True, **flow)
        assert (k, nbk) == (K, 18) and 0 < K < 18                      # bricks on both sides
        assert tuple(vol.shape) == LATTICE and vol.dtype == torch.float32 and vol.is_contiguous()
        diff = int((_bits(vol)[mask] != _bits(want)[mask]).sum())
        print(f"\nquery_sigma_lattice {prec} {nof} fill {fill}: {K} of {nbk} bricks, {int(mask.sum())} active points, {diff} differ from the dense query")
        assert diff == 0
        assert bool((vol[~mask] == fill).all()) and int((~mask).sum()) > 0
    old = M.points.LATTICE_CHUNK_BRICKS
    M.points.LATTICE_CHUNK_BRICKS = 2
    try:
        chunked = M.query_sigma_lattice(axes, nerfs[0], embs[0], grid, world_of_axis=woa, fill=0.0, precision=prec, **flow)
    finally:
        M.points.LATTICE_CHUNK_BRICKS = old
    assert K > 2 and torch.equal(_bits(chunked), _bits(vol))
    cuda_axes = [_dev(a) for a in axes]                                 # device tensors as axes: the same volume
    assert torch.equal(_bits(M.query_sigma_lattice(cuda_axes, nerfs[0], embs[0], grid, world_of_axis=woa, fill=0.0, precision=prec, **flow)),
                       _bits(vol))


FLAT = (8 * LAT_THREADS + 1, 8 * LAT_THREADS + 1, 1)                    # SELECT_TIERS["idle"]: two counts per scan thread


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_query_sigma_lattice_past_65536_bricks(M, prec):
    """The documented guarantee on a flat lattice where select scans more counts than it has threads and scatter takes a second
    trip over the rows: K and the brick total are the oracle's; the volume is, bit for bit, query_sigma on the oracle's
    points of the active bricks laid out by the oracle's scatter -- a point's sigma does not depend on its place in the batch
    --, which also says that every other point is `fill`."""
    woa, fill = (0, 1, 2), float("-inf")
    case = dict(n=8, S=8, M=0, extra="dir", regime="dense", nof="none")
    embs, nerfs, _ = build_case(M, case, 0, device="cuda")
    grid, dense = _ball_grid(M)
    axes = _axes(FLAT, (-1.0, -1.0, -0.4), (1.0, 1.0, -0.4))             # the one z is the ball centre's
    bricks = int(np.prod(LO.n_bricks(FLAT)))
    assert bricks > LAT_THREADS * LAT_THREADS and FLAT[0] * FLAT[1] > SCATTER_MAX_BLOCKS
    slot, ids, K = _oracle_select(dense, grid.lo, grid.hi, axes, woa, 1, LO.select_fast)
    assert 0.02 * bricks < K < 0.5 * bricks
    with torch.no_grad():
        vol, stats = M.query_sigma_lattice(axes, nerfs[0], embs[0], grid, world_of_axis=woa, margin=1, fill=fill, precision=prec,
                                           return_stats=True)
        rows = M.query_sigma(_dev(LO.points(ids, axes, woa)), nerfs[0], embs[0], precision=prec)
    assert stats == (K, bricks)
    assert tuple(vol.shape) == FLAT and vol.dtype == torch.float32 and vol.is_contiguous()
    want = LO.scatter(rows.cpu().numpy(), slot, FLAT, np.float32(fill))
    mask = LO.active_mask(slot, FLAT)
    got = vol.cpu().numpy()
    diff = int((got.view(np.int32) != want.view(np.int32)).sum())
    print(f"\nquery_sigma_lattice {prec} on {FLAT}: {K} of {bricks} bricks, {int(mask.sum())} active points, {diff} words differ")
    assert diff == 0
    assert np.isfinite(got[mask]).all() and np.isneginf(got[~mask]).all() and 0 < mask.sum() < mask.size


# ------------------------------------------------------------------------------------------------ the callers
def _load(module, sd):
    module.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return module.cuda()


@pytest.fixture(scope="module")
def mesh_models(M):
    """The NeRF of tests/test_gpu_mesh.py (raw sigma crosses 10), its dense 20^3 volume and the grids of the tests below."""
    from moco_flow_amd import synth
    Ng = 20
    sd = synth.nerf_state(0, extra_feat_type="ind", extra_feat_dim=5, regime="dense")
    sd["sigma.weight"] = sd["sigma.weight"] * np.float32(3.0)
    nerf = _load(M.NeRF(8, 256, 63, [4], "ind", 5), sd)
    embs = [M.Embedding(3, 10), M.Embedding(1, 2), None]
    with torch.no_grad():
        sigma = M.query_sigma(M.mesh.lattice(Ng, "cuda"), nerf, embs[0], ind=IND_SCALAR, precision="f32").view(Ng, Ng, Ng)
    lo, hi = (-1.5,) * 3, (1.5,) * 3
    world = sigma.permute(1, 0, 2).contiguous()                        # the volume's axes are (y, x, z): the grid's are (x, y, z)
    own = M.OccupancyGrid.from_sigma(world, lo, hi, 5.0, "relu", 1)     # tau = sigma_threshold / 2
    return dict(Ng=Ng, nerf=nerf, embs=embs, sigma=sigma, own=own, full=_grid(M, np.ones((4, 3, 5), dtype=bool), lo, hi),
                empty=_grid(M, np.zeros((4, 3, 5), dtype=bool), lo, hi))


def test_extract_mesh_behind_a_grid(M, mesh_models):
    m = mesh_models
    kw = dict(N_grid=m["Ng"], sigma_threshold=10, ind=IND_SCALAR, precision="f32")
    with torch.no_grad():
        v0, t0 = M.extract_mesh(m["nerf"], m["embs"][0], **kw)
        assert len(v0) > 0 and len(t0) > 0
        v, t = M.extract_mesh(m["nerf"], m["embs"][0], occupancy=m["full"], **kw)
        assert torch.equal(_bits(v), _bits(v0)) and torch.equal(t, t0)             # a full grid: the dense call, bit for bit
        v, t = M.extract_mesh(m["nerf"], m["embs"][0], occupancy=m["empty"], **kw)
        assert tuple(v.shape) == (0, 3) and tuple(t.shape) == (0, 3) and v.dtype == torch.float32 and t.dtype == torch.int64
        v, t = M.extract_mesh(m["nerf"], m["embs"][0], occupancy=m["own"], **kw)
        assert torch.equal(_bits(v), _bits(v0)) and torch.equal(t, t0)             # its own grid at tau = threshold / 2
        ax = np.linspace(-1.5, 1.5, m["Ng"]).astype(np.float32)
        vol, (K, nbk) = M.query_sigma_lattice((ax, ax, ax), m["nerf"], m["embs"][0], m["own"], world_of_axis=(1, 0, 2), fill=0.0,
                                              ind=IND_SCALAR, precision="f32", return_stats=True)
        print(f"\nextract_mesh behind its own grid: {K} of {nbk} bricks, V {len(v0)} T {len(t0)}")
        assert 0 < K <= nbk == 27
        # a ball that leaves bricks on both sides: the volume is the dense one ('xy' order: axis 0 carries y) in the active
        # bricks and 0 elsewhere, and the mesh is marching cubes of exactly that volume
        ball, dense = _ball_grid(M, (12, 12, 12), (-1.5,) * 3, (1.5,) * 3, center=(-0.6, 0.5, -0.7), radius=0.4)
        vol, (K, nbk) = M.query_sigma_lattice((ax, ax, ax), m["nerf"], m["embs"][0], ball, world_of_axis=(1, 0, 2), fill=0.0,
                                              ind=IND_SCALAR, precision="f32", return_stats=True)
        lo32, hi32, inv, _ = O.grid_constants(dense.shape, ball.lo, ball.hi, 0.5)
        slot, _, want_K = LO.select(dense, LO.range_tables((ax, ax, ax), 1, dense.shape, lo32, hi32, inv, (1, 0, 2)), (20,) * 3, (1, 0, 2))
        mask = _dev(LO.active_mask(slot, (20,) * 3))
        assert 0 < K < nbk and K == want_K
        assert torch.equal(_bits(vol)[mask], _bits(m["sigma"])[mask]) and bool((vol[~mask] == 0).all())
        raw, tris = M.marching_cubes(vol, 10, clamp_zero=True)
        v, t = M.extract_mesh(m["nerf"], m["embs"][0], occupancy=ball, **kw)
        assert 0 < len(v) < len(v0)
        assert torch.equal(_bits(v), _bits(raw[:, [1, 0, 2]] / m["Ng"] * 3.0 - 1.5)) and torch.equal(t, tris[:, [0, 2, 1]])


def test_extract_colored_mesh_behind_a_grid(M, mesh_models):
    m = mesh_models
    kw = dict(N_grid=m["Ng"], sigma_threshold=10, ind=IND_SCALAR, precision="f32")
    with torch.no_grad():
        want = M.extract_colored_mesh(m["nerf"], m["embs"], **kw)
        got = M.extract_colored_mesh(m["nerf"], m["embs"], occupancy=m["own"], **kw)
        none = M.extract_colored_mesh(m["nerf"], m["embs"], occupancy=m["empty"], **kw)
    assert len(want[0]) > 0
    for g, w, name in zip(got, want, ("verts", "tris", "normals", "colors")):
        assert torch.equal(_bits(g), _bits(w)), name
    assert [tuple(x.shape) for x in none] == [(0, 3)] * 4


@pytest.fixture(scope="module")
def field(M):
    case = dict(n=8, S=8, M=0, extra="dir", regime="dense", nof="none")
    embs, nerfs, _ = build_case(M, case, 0, device="cuda")
    aabb = np.array([[-0.9, -0.5, -1.1], [0.8, 0.6, 1.0]])
    n = (9, 6, 34)
    with torch.no_grad():
        sigma = M.query_sigma(M.OccupancyGrid.lattice(n, aabb, "cuda")[0], nerfs[0], embs[0], precision="f32")
    tau = float(np.median(np.log1p(np.exp(sigma.cpu().numpy().astype(np.float64)))))          # half the points active
    return dict(nerf=nerfs[0], emb=embs[0], aabb=aabb, n=n, tau=tau)


def test_from_field_within_a_full_grid_equals_the_dense_build(M, field):
    f = field
    kw = dict(N_grid=f["n"], sigma_threshold=f["tau"], precision="f32")
    dense = M.OccupancyGrid.from_field(f["nerf"], f["emb"], f["aabb"], **kw)
    full = _grid(M, np.ones((3, 2, 4), dtype=bool), f["aabb"][0], f["aabb"][1])
    got = M.OccupancyGrid.from_field(f["nerf"], f["emb"], f["aabb"], within=full, **kw)
    assert got.dims == dense.dims == (8, 5, 33) and torch.equal(got.bits, dense.bits)
    assert 0 < dense.occupied_fraction() == got.occupied_fraction()
    assert np.array_equal(got.lo, dense.lo) and np.array_equal(got.hi, dense.hi)


def test_from_field_within_a_ball_equals_its_two_steps(M, field):
    f = field
    lo, hi = f["aabb"][0], f["aabb"][1]
    ball, _ = _ball_grid(M, (4, 3, 8), lo, hi, center=(0.3, 0.2, -0.6), radius=0.3)
    axes = _axes(f["n"], lo, hi)
    vol, (K, nbk) = M.query_sigma_lattice(axes, f["nerf"], f["emb"], ball, fill=float("-inf"), precision="f32", return_stats=True)
    assert 0 < K < nbk == 2 * 1 * 5
    by_hand = M.OccupancyGrid.from_sigma(vol, lo, hi, f["tau"], "softplus", 1)
    got = M.OccupancyGrid.from_field(f["nerf"], f["emb"], f["aabb"], N_grid=f["n"], sigma_threshold=f["tau"], precision="f32", within=ball)
    dense = M.OccupancyGrid.from_field(f["nerf"], f["emb"], f["aabb"], N_grid=f["n"], sigma_threshold=f["tau"], precision="f32")
    assert torch.equal(got.bits, by_hand.bits) and got.occupied_fraction() == by_hand.occupied_fraction()
    assert 0 < got.occupied_fraction() < dense.occupied_fraction()
    assert bool(((got.bits & ~dense.bits) == 0).all())                            # nothing the dense build does not have


# ------------------------------------------------------------------------------------------------ streams
def test_query_on_a_side_stream_equals_the_serial_result(M, field):
    """query_sigma_lattice on stream B behind a hold: the grid's words are zero until a copy ON B, behind the hold, fills them,
    and the blocks the outputs take were filled with 0xFF on B behind the hold.  A select on any other stream reads an empty
    grid (K = 0, a volume of fill); a query or a scatter on another stream is overwritten or reads 0xFF."""
    f = field
    lo, hi = f["aabb"][0], f["aabb"][1]
    ball, _ = _ball_grid(M, (4, 3, 8), lo, hi, center=(0.3, 0.2, -0.6), radius=0.3)
    axes = _axes(f["n"], lo, hi)
    fn = lambda grid: M.query_sigma_lattice(axes, f["nerf"], f["emb"], grid, fill=0.0, precision="f32", return_stats=True)
    want, (K, nbk) = fn(ball)
    want = want.clone()
    assert 0 < K < nbk
    torch.cuda.synchronize()
    _, b = independent_streams()
    late = M.OccupancyGrid(torch.zeros_like(ball.bits), ball.dims, lo, hi)
    torch.cuda.synchronize()
    b.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(b):
        hold(b, HOLD_MS)
        late.bits.copy_(ball.bits)
        filled, marker = torch.cuda.Event(), torch.cuda.Event()
        filled.record(b)
        marker.record(torch.cuda.default_stream())
        poison([want.numel() * 4, K * 512 * 4, K * 512 * 12, nbk * 4])
        assert first_done(marker, filled), "producer was not delayed: the default stream did not run while B was held"
        delayed = filled.query() is False                              # read before the call: its count read-back waits for B
        got, stats = fn(late)
    b.synchronize()
    assert delayed, "producer was not delayed"
    assert stats == (K, nbk) and torch.equal(_bits(got), _bits(want))


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(M, field):
    f = field
    lo, hi = f["aabb"][0], f["aabb"][1]
    grid = _grid(M, np.ones((3, 2, 4), dtype=bool), lo, hi)
    axes = _axes(f["n"], lo, hi)
    q = lambda ax=axes, g=grid, **kw: M.query_sigma_lattice(ax, f["nerf"], f["emb"], g, **kw)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        q(ax=[torch.from_numpy(a) for a in axes])                       # a CPU tensor

    class Elsewhere:                                                    # the grid on another device: refused before it is touched
        device = torch.device("cuda", torch.cuda.current_device() + 1)
    with pytest.raises(RuntimeError, match="the grid on"):
        q(g=Elsewhere())
    case = dict(n=8, S=8, M=0, extra="ind", regime="dense", nof="bw")
    embs, nerfs, kw = build_case(M, case, 0, device="cuda")
    with pytest.raises(RuntimeError, match="per-point"):
        M.query_sigma_lattice(axes, nerfs[0], embs[0], grid, bw_nof=kw["nof_models"][0], nof_embeddings=kw["nof_embeddings"],
                              ind=torch.zeros(int(np.prod(f["n"])), device="cuda"))
    with pytest.raises(RuntimeError, match="margin=-1"):
        q(margin=-1)
    with pytest.raises(RuntimeError, match="ascending"):
        q(ax=[axes[0], axes[1][::-1].copy(), axes[2]])                  # descending
    with pytest.raises(RuntimeError, match="not a permutation"):
        q(world_of_axis=(0, 2, 2))
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        M.extract_mesh(M.NeRF(8, 256, 63, [4], "dir", 27), M.Embedding(3, 10), N_grid=20, occupancy=grid)
