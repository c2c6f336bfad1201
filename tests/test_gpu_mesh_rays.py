"""Ray casts on the MI355X: mf_surface_corners / mf_surface_cast (csrc/mf_mesh_rays.hip) and MeshIndex.corners / cast_rays /
visible_from against the numpy restatement of their contract (tests/mesh_rays_oracle.py: np.float32, brute force).  Every
comparison is equality, with no tolerance and nothing left out (np.array_equal: a NaN fails it; the sign of a zero is the one
thing it does not see, mesh_distance_oracle.py says why); where no oracle is run (the mesh at size) the culled search is
held to the full sweep, byte for byte.

Launch shape: the cast has no grid-stride loop -- a wave per 64 rays, a workgroup per kSurfThreads -- so there is no second trip to
reach; Q = 300 and the 10 700-ray case run several workgroups."""
import numpy as np
import pytest
import torch

import mesh_rays_oracle as O

pytestmark = pytest.mark.gpu
F = np.float32
INF = F(np.inf)


@pytest.fixture(scope="module")
def M():
    import moco_flow_amd
    assert torch.cuda.is_available()
    moco_flow_amd._lib.lib()
    return moco_flow_amd


@pytest.fixture(scope="module")
def blob():
    verts, tris = O.blob()
    assert len(tris) == 1280
    return verts, tris


@pytest.fixture(scope="module")
def inside(blob):
    """The watertightness case: every ray family from inside the blob, and the oracle's answer, computed once."""
    verts, tris = blob
    d = np.concatenate(list(O.ray_families(verts, tris, O.blob_interior()).values()))
    o = np.ascontiguousarray(np.broadcast_to(O.blob_interior(), d.shape))
    assert len(d) == 10700
    return o, d, O.cast(O.records(verts, tris), o, d)


@pytest.fixture(scope="module")
def outside(blob):
    """Rays that cross the whole blob (two hits and more) or pass it by: from a point outside towards its vertices and around."""
    verts, tris = blob
    rng = np.random.default_rng(3)
    o = (O.BLOB_CENTER + np.array([0.4, -0.3, 4.0])).astype(F)
    d = np.concatenate([verts - o, (verts[:200] - o) + rng.normal(size=(200, 3)).astype(F) * F(0.8)]).astype(F)
    o = np.ascontiguousarray(np.broadcast_to(o, d.shape))
    want = O.cast(O.records(verts, tris), o, d)
    assert 0 < want[3][642:].sum() < 200 and 600 < want[3][:642].sum() < 642      # a vertex on the silhouette may be missed
    return o, d, want


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()                   # a copy: a broadcast view is not writable


def _np(t):
    return t.cpu().numpy()


def _index(M, verts, tris, order="morton"):
    return M.MeshIndex(_dev(verts), _dev(tris), order=order)


def _records(index, verts, tris):
    return O.records(verts, tris, None if index.order is None else _np(index.order))


def _raw(M, index, o, d, t_min=0.0, t_max=np.inf, mode=0, cull=1, qorder=None, start=None):
    """mf_surface_cast alone, on outputs filled with a sentinel beforehand, so that an unwritten row shows -> (t, tri, bary, hit,
    visited); the outputs the mode does not write keep the sentinel."""
    L = M._lib
    o, d = _dev(o), _dev(d)
    Q = o.shape[0]
    lo, hi = (_dev(b) for b in O.bounds(Q, t_min, t_max))
    t = torch.full((Q,), -7.0, dtype=torch.float32, device="cuda")
    tri = torch.full((Q,), -9, dtype=torch.int32, device="cuda")
    bary = torch.full((Q, 3), -7.0, dtype=torch.float32, device="cuda")
    hit = torch.full((Q,), 77, dtype=torch.uint8, device="cuda")
    visited = torch.full(((Q + 63) // 64,), -5, dtype=torch.int32, device="cuda")
    qo = None if qorder is None else _dev(np.asarray(qorder, dtype=np.int32))
    st = None if start is None else _dev(np.asarray(start, dtype=np.int32))
    L.launch(o.device, "mf_surface_cast", L.ptr0(index.corners), L.ptr0(index.slot_tri), L.ptr0(index.tile_box), index.T, L.ptr0(o), L.ptr0(d), 3,
             L.ptr0(lo), L.ptr0(hi), 1, Q, L.ptr0(qo), L.ptr0(st), mode, cull, L.ptr0(t), L.ptr0(tri), L.ptr0(bary), L.ptr0(hit), L.ptr0(visited))
    return tuple(_np(x) for x in (t, tri, bary, hit, visited))


def _same(got, want, what=""):
    """first: (t, tri, bary) against the oracle's first three"""
    for g, w, name in zip(got, want, ("t", "tri", "bary")):
        g = _np(g) if isinstance(g, torch.Tensor) else g
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, name, int((g != w).sum()))


def _same_hit(got, want, what=""):
    g = _np(got) if isinstance(got, torch.Tensor) else got
    assert g.dtype == np.uint8 and np.array_equal(g, want[3]), (what, "hit", int((g != want[3]).sum()))


def _check_all(M, index, R, o, d, want, t_min=0.0, t_max=np.inf, what=""):
    """both modes, cull on and off, through the ABI and through cast_rays"""
    lo, hi = O.bounds(len(o), t_min, t_max)
    scalar = np.isscalar(t_min) and np.isscalar(t_max)                       # floats go to cast_rays as floats, arrays as tensors
    bounds = dict(t_min=float(t_min), t_max=float(t_max)) if scalar else dict(t_min=_dev(lo), t_max=_dev(hi))
    for cull in (0, 1):
        got = _raw(M, index, o, d, t_min, t_max, 0, cull)
        _same(got, want, (what, "raw first", cull))
        assert (got[3] == 77).all()
        got = _raw(M, index, o, d, t_min, t_max, 1, cull)
        _same_hit(got[3], want, (what, "raw any", cull))
        assert (got[1] == -9).all()
        _same(M.cast_rays(index, _dev(o), _dev(d), cull=bool(cull), **bounds), want, (what, "first", cull))
        _same_hit(M.cast_rays(index, _dev(o), _dev(d), mode="any", cull=bool(cull), **bounds), want, (what, "any", cull))


@pytest.mark.parametrize("T", [1, 63, 64, 65, 130])
def test_tiling_edges(M, blob, T):
    verts, tris = blob
    tris = tris[:T]
    rng = np.random.default_rng(T)
    index = _index(M, verts, tris)
    R = _records(index, verts, tris)
    corners = _np(index.corners)
    assert corners.shape == (index.n_tiles * 64, 16) and np.array_equal(corners, O.corners(R))
    assert np.array_equal(corners[:, 9:15], np.where(R["slot_tri"][:, None] >= 0, R["edges"][:, 6:12], 0))
    for Q in (1, 63, 65, 300):
        w = rng.random((Q - Q // 2, 3))
        w /= w.sum(1, keepdims=True)
        k = rng.integers(T, size=len(w))
        aimed = sum(verts[tris[k, c]].astype(np.float64) * w[:, c:c + 1] for c in range(3))
        d = np.concatenate([aimed - O.blob_interior(), rng.normal(size=(Q // 2, 3))]).astype(F)
        o = np.ascontiguousarray(np.broadcast_to(O.blob_interior(), d.shape))
        want = O.cast(R, o, d)
        assert want[3][:len(w)].sum() >= len(w) - 1                          # the aimed rays hit, give or take one on an open border
        _check_all(M, index, R, o, d, want, what=(T, Q))


def test_watertight(M, blob, inside):
    verts, tris = blob
    o, d, want = inside
    assert want[3].all() and (want[1] >= 0).all() and np.isfinite(want[0]).all()
    index = _index(M, verts, tris)
    assert int(index.dropped_count) == 0
    got = M.cast_rays(index, _dev(o), _dev(d))
    assert (_np(got[1]) >= 0).all() and np.isfinite(_np(got[0])).all()        # all hit
    _same(got, want)
    _same_hit(M.cast_rays(index, _dev(o), _dev(d), mode="any"), want)
    _same(M.cast_rays(index, _dev(o), _dev(d), cull=False), want)


def test_ties_resolve_to_the_lowest_index(M, blob, inside):
    verts, tris = blob
    o, d, want = inside
    o, d = o[::7], d[::7]
    twice = np.concatenate([tris, tris])                                     # the mesh listed twice: every hit is a tie of two
    for order in ("morton", "identity", _dev(np.arange(len(twice), dtype=np.int32)[::-1].copy())):
        got = M.cast_rays(_index(M, verts, twice, order), _dev(o), _dev(d))
        _same(got, tuple(w[::7] for w in want), "twice")
        assert (_np(got[1]) < len(tris)).all()
    # a ray exactly through the edge two triangles share: Sx = Sy = 0, the shear is exact, the edge function 0 in both
    v = np.array([[0, -1, 1], [0, 1, 1], [1, 0, 1], [-1, 0, 1]], dtype=F)
    o1, d1 = np.zeros((1, 3), F), np.array([[0, 0, 2]], F)
    for t in (np.array([[0, 1, 2], [1, 0, 3]]), np.array([[1, 0, 3], [0, 1, 2]])):
        R = O.records(v, t)
        assert O.evaluate(R, O.setup(o1, d1))[6].sum() == 2                   # both accept it
        for order in ("identity", _dev(np.array([1, 0], dtype=np.int32))):
            got = M.cast_rays(_index(M, v, t, order), _dev(o1), _dev(d1))
            _same(got, O.cast(R, o1, d1))
            assert _np(got[1]).tolist() == [0] and _np(got[0]).tolist() == [0.5]


def _schedules(M, index, o, d):
    """The four ray schedules the walk is pinned under, as (qorder, start) in numpy: as cast_rays derives them (the Morton order
    of the point each ray reaches at the distance of the mesh's centre); none (identity, tile 0); that order with every wave
    starting at the last tile; starts out of range on both sides."""
    o, d = _dev(o), _dev(d)
    reach = ((index.lo + index.hi) * 0.5 - o).norm(dim=1, keepdim=True) / d.norm(dim=1, keepdim=True)
    qorder, start = (_np(x) for x in M.mesh._schedule(index, o + d * reach))
    n_waves, n = len(start), index.n_tiles
    return ((qorder, start), (None, None), (qorder, np.full(n_waves, n - 1)), (qorder, np.where(np.arange(n_waves) % 2, n + 5, -3)))


@pytest.mark.parametrize("T", [65, 130, 1280])
def test_the_walk_is_the_oracles(M, blob, inside, outside, T):
    """The tiles each wave evaluates, and every output, are cast_culled's, exactly: both modes, cull on and off, four schedules.
    The visiting order, the clamped start, the early exit and the one decision per wave and tile are the oracle's.  (2, 3 and 20
    tiles; two full waves and one of 2 rays.)"""
    verts, tris = blob
    tris = tris[:T]
    index = _index(M, verts, tris)
    R = _records(index, verts, tris)
    n = index.n_tiles
    rng = np.random.default_rng(T)
    pick_in, pick_out = rng.choice(len(inside[0]), 100, replace=False), rng.choice(len(outside[0]), 30, replace=False)
    perm = rng.permutation(130)
    o = np.concatenate([inside[0][pick_in], outside[0][pick_out]])[perm]
    d = np.concatenate([inside[1][pick_in], outside[1][pick_out]])[perm]
    want = O.cast(R, o, d)
    culled, fewer_any = [], False
    for k, (qorder, start) in enumerate(_schedules(M, index, o, d)):
        per_mode = {}
        for mode in (0, 1):
            for cull in (1, 0):
                ref = O.cast_culled(R, o, d, 0.0, np.inf, mode, qorder, start, bool(cull))
                if mode == 0:
                    _same(ref, want, ("oracle", T, k, cull))
                else:
                    _same_hit(ref[3], want, ("oracle", T, k, cull))
                got = _raw(M, index, o, d, mode=mode, cull=cull, qorder=qorder, start=start)
                _same(got, want, (T, k, cull)) if mode == 0 else _same_hit(got[3], want, (T, k, cull))
                assert got[4].dtype == np.int32 and np.array_equal(got[4], ref[4]), (T, k, mode, cull, got[4], ref[4])
                if not cull:
                    assert (ref[4] == n).all()
                    continue
                per_mode[mode] = ref[4]
                if k == 3:                                                   # out of range behaves as clamped
                    assert np.array_equal(ref[4], O.cast_culled(R, o, d, 0.0, np.inf, mode, qorder, np.clip(start, 0, n - 1))[4])
        print(f"T={T} schedule {k}: tiles evaluated per wave of {n}: first {per_mode[0]}, any {per_mode[1]}")
        culled += [per_mode[0], per_mode[1]]
        fewer_any = fewer_any or bool((per_mode[1] < per_mode[0]).any())
    culled = np.concatenate(culled)
    assert ((culled > 0) & (culled < n)).any()                               # not vacuous: the oracle itself culls here,
    assert fewer_any == (T > 65)                                             # any hit more (of 65 triangles, never a whole wave's rays)
    # a wave of dead rays (zero directions) evaluates nothing under the cull, and every tile under the sweep
    dead = np.zeros((64, 3), F)
    for mode in (0, 1):
        for cull in (1, 0):
            ref = O.cast_culled(R, o[:64], dead, 0.0, np.inf, mode, cull=bool(cull))
            got = _raw(M, index, o[:64], dead, mode=mode, cull=cull)
            assert ref[4].tolist() == got[4].tolist() == [0 if cull else n]
            assert (got[1] == -1).all() and np.isinf(got[0]).all() if mode == 0 else not got[3].any()


def test_cull_equals_sweep_at_size(M):
    n = 48
    ax = torch.linspace(0, 1, n, device="cuda")
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    vol = (torch.sin(6.0 * x + 2.0 * y * y) + torch.sin(5.0 * y + 3.0 * z) + torch.sin(7.0 * z + 4.0 * x * y)).contiguous()
    verts, tris = M.marching_cubes(vol, 0.3)
    index = M.MeshIndex(verts, tris)
    assert index.T > 10000 and index.n_tiles > 150
    rng = np.random.default_rng(47)
    u, v = np.meshgrid(np.linspace(-0.5, 0.5, 64), np.linspace(-0.5, 0.5, 64))
    cam_d = np.stack([u.ravel(), v.ravel(), np.ones(4096)], -1).astype(F)   # a 64 x 64 pinhole frame looking along +z
    cam_o = np.broadcast_to(np.array([23.5, 23.5, -40.0], F), cam_d.shape)
    rnd_o = (rng.random((4096, 3)) * 47).astype(F)
    rnd_d = rng.normal(size=(4096, 3)).astype(F)
    o, d = _dev(np.concatenate([cam_o, rnd_o])), _dev(np.concatenate([cam_d, rnd_d]))
    sweep = M.cast_rays(index, o, d, cull=False, return_visited=True)
    cull = M.cast_rays(index, o, d, return_visited=True)
    for a, b in zip(sweep[:3], cull[:3]):
        assert a.dtype == b.dtype and _np(a).tobytes() == _np(b).tobytes()
    any_sweep = M.cast_rays(index, o, d, mode="any", cull=False, return_visited=True)
    any_cull = M.cast_rays(index, o, d, mode="any", return_visited=True)
    assert torch.equal(any_sweep[0], any_cull[0]) and torch.equal(any_cull[0], torch.isfinite(cull[0]).to(torch.uint8))
    hits = float(any_cull[0].float().mean())
    assert 0.3 < hits < 1.0
    assert (_np(sweep[3]) == index.n_tiles).all() and (_np(any_sweep[1]) == index.n_tiles).all()
    mean_first, mean_any = float(cull[3].float().mean()), float(any_cull[1].float().mean())
    print(f"tiles evaluated per wave of {index.n_tiles}: first {mean_first:.1f}, any {mean_any:.1f}; {hits:.3f} of the rays hit")
    assert mean_first < index.n_tiles and mean_any < index.n_tiles           # the cull does cull


def test_order_independence(M, blob, inside, outside):
    verts, tris = blob
    rng = np.random.default_rng(31)
    T = len(tris)
    o = np.concatenate([inside[0][::9], outside[0]])
    d = np.concatenate([inside[1][::9], outside[1]])
    want = tuple(np.concatenate([a[::9], b]) for a, b in zip(inside[2], outside[2]))
    qperm = rng.permutation(len(o))
    for order in ("morton", "identity", _dev(rng.permutation(T).astype(np.int32))):
        index = _index(M, verts, tris, order)
        assert int(index.dropped_count) == 0
        for cull in (True, False):
            _same(M.cast_rays(index, _dev(o), _dev(d), cull=cull), want, cull)
        _same(M.cast_rays(index, _dev(o[qperm]), _dev(d[qperm])), tuple(w[qperm] for w in want))       # the caller's rows in another order
        _same_hit(M.cast_rays(index, _dev(o[qperm]), _dev(d[qperm]), mode="any"), tuple(w[qperm] for w in want))
        n_waves = (len(o) + 63) // 64
        for qorder, start in ((None, None), (qperm, None), (qperm[::-1], rng.integers(-3, index.n_tiles + 3, size=n_waves))):
            for mode in (0, 1):
                got = _raw(M, index, o, d, mode=mode, qorder=qorder, start=start)          # any visiting order, any first tile
                _same(got, want) if mode == 0 else _same_hit(got[3], want)
    # an order that is no permutation drops what it loses and cannot fault: the oracle on the kept set
    bad = np.arange(T, dtype=np.int32)
    bad[5], bad[7], bad[70], bad[200:264] = 9, T, -1, 300
    index = _index(M, verts, tris, _dev(bad))
    Rb = O.records(verts, tris, bad)
    assert int(index.dropped_count) == Rb["dropped_count"] == 67
    wb = O.cast(Rb, o, d)
    assert not np.array_equal(wb[1], want[1]) and not Rb["dropped"][wb[1][wb[1] >= 0]].any()
    _check_all(M, index, Rb, o, d, wb, what="bad order")


def test_t_range(M, blob, outside):
    verts, tris = blob
    o, d, first = outside
    o, d, first = o[:642], d[:642], tuple(w[:642] for w in first)
    index = _index(M, verts, tris)
    R = _records(index, verts, tris)
    past = np.nextafter(first[0], INF)                                       # just past the first hit: the second
    second = O.cast(R, o, d, past, np.inf)
    assert second[3].sum() > 600 and (second[0] > first[0])[first[3] == 1].all() and (second[1] != first[1])[second[3] == 1].all()
    _check_all(M, index, R, o, d, second, t_min=past, what="second")
    below = np.nextafter(first[0], F(0))                                     # t_max below the first hit: a miss
    miss = O.cast(R, o, d, 0.0, below)
    assert not miss[3].any()
    _check_all(M, index, R, o, d, miss, t_max=below, what="miss")
    exact = O.cast(R, o, d, first[0], first[0])                              # [t, t]: the bounds are inclusive
    _same(exact, first)
    _check_all(M, index, R, o, d, exact, t_min=first[0], t_max=first[0], what="exact")
    # one tensor bound and one float
    _same(M.cast_rays(index, _dev(o), _dev(d), t_min=_dev(past)), second)
    _same(M.cast_rays(index, _dev(o), _dev(d), t_max=_dev(below)), miss)
    # (Q, 8) rows in the package's layout, and wider rows, give the same bytes as the split form
    rows = np.concatenate([o, d, past[:, None], np.full((642, 1), 50, F), np.full((642, 3), np.nan, F)], 1).astype(F)
    want = O.cast(R, o, d, past, 50.0)
    split = M.cast_rays(index, _dev(o), _dev(d), t_min=_dev(past), t_max=50.0)
    _same(split, want)
    for rays in (_dev(rows[:, :8]), _dev(rows), _dev(rows)[:, :9]):
        got = M.cast_rays(index, rays=rays)
        for a, b in zip(got, split):
            assert _np(a).tobytes() == _np(b).tobytes()
        assert torch.equal(M.cast_rays(index, rays=rays, mode="any"), M.cast_rays(index, _dev(o), _dev(d), t_min=_dev(past), t_max=50.0, mode="any"))


def test_degenerate_input(M, blob, inside):
    verts, tris = blob
    rng = np.random.default_rng(53)
    V = len(verts)
    # the blob with a NaN vertex (its ring of triangles is dropped) and, shuffled in, triangles without area or with bad indices
    v = np.concatenate([verts, [[np.nan, 0, 0], [np.inf, 0, 0]]]).astype(F)
    extra = np.array([[0, 0, 1], [3, 3, 3], [0, 1, V + 2], [-1, 2, 3], [4, 1 << 40, 5], [0, 1, V], [2, V + 1, 3]], dtype=np.int64)
    t = np.concatenate([tris, extra])[rng.permutation(len(tris) + len(extra))]
    v[17] = np.nan
    index = _index(M, v, t)
    R = _records(index, v, t)
    assert R["dropped_count"] == int(index.dropped_count) and len(extra) < R["dropped_count"] <= len(extra) + 7
    assert np.array_equal(_np(index.corners), O.corners(R))
    o, d = inside[0][::5].copy(), inside[1][::5].copy()
    d[3], d[4, 1], d[5, 2], o[6, 0], o[7, 1] = 0, np.nan, np.inf, np.nan, -np.inf               # dead rays
    t_min, t_max = np.zeros(len(o), F), np.full(len(o), np.inf, F)
    t_min[8], t_max[8] = 2, 1                                                 # t_min > t_max
    t_min[9] = np.nan
    want = O.cast(R, o, d, t_min, t_max)
    assert not want[3][3:10].any() and 0 < (want[3] == 0).sum() < 60        # the hole around vertex 17 lets a few out
    assert not R["dropped"][want[1][want[1] >= 0]].any()
    _check_all(M, index, R, o, d, want, t_min=t_min, t_max=t_max, what="degenerate")
    # an origin exactly on a vertex: q = 0 for it, and the triangles around it accept at t = 0
    index = _index(M, verts, tris)
    R = _records(index, verts, tris)
    o = verts[::3].copy()
    d = (O.BLOB_CENTER.astype(F) - o).astype(F)
    want = O.cast(R, o, d)
    assert want[3].all() and (want[0] == 0).all() and (tris[want[1]] == np.arange(V)[::3, None]).any(1).all()
    _check_all(M, index, R, o, d, want, what="on a vertex")


def test_any_hit(M, blob, inside, outside):
    verts, tris = blob
    index = _index(M, verts, tris)
    for o, d, want in (inside, outside):
        t = M.cast_rays(index, _dev(o), _dev(d))[0]
        hit = M.cast_rays(index, _dev(o), _dev(d), mode="any")
        assert hit.dtype == torch.uint8 and torch.equal(hit, torch.isfinite(t).to(torch.uint8))
        _same_hit(hit, want)
    # 64 rays that all hit in the tile their wave starts at: nothing else is evaluated
    R = _records(index, verts, tris)
    tile = 7
    k = R["slot_tri"][tile * 64:(tile + 1) * 64]
    assert (k >= 0).all()
    d = ((verts[tris[k, 0]] + verts[tris[k, 1]] + verts[tris[k, 2]]) * F(1 / 3) - O.blob_interior()).astype(F)
    o = np.ascontiguousarray(np.broadcast_to(O.blob_interior(), d.shape))
    want = O.cast(R, o, d)
    assert np.array_equal(want[1], k)
    got = _raw(M, index, o, d, mode=1, start=[tile])
    _same_hit(got[3], want)
    assert got[4].tolist() == [1]
    got = _raw(M, index, o, d, mode=0, start=[tile])
    _same(got, want)
    assert 1 <= got[4][0] < index.n_tiles
    assert _raw(M, index, o, d, mode=1, cull=0, start=[tile])[4].tolist() == [index.n_tiles]


def test_visible_from(M, blob):
    verts, tris = blob
    index = _index(M, verts, tris)
    R = _records(index, verts, tris)
    eye = (O.BLOB_CENTER + np.array([3.0, 1.0, 2.0])).astype(F)
    want = O.visible(R, verts, eye, 1e-3)
    assert 0.25 < want.mean() < 0.75                                         # both values occur: the near side is seen
    got = M.visible_from(index, _dev(verts), _dev(eye), 1e-3)
    assert got.dtype == torch.uint8 and np.array_equal(_np(got), want)
    assert torch.equal(M.visible_from(index, _dev(verts), _dev(np.broadcast_to(eye, verts.shape)), 1e-3), got)
    toward = ((verts - O.BLOB_CENTER.astype(F)) * (eye - O.BLOB_CENTER.astype(F))).sum(1)
    assert want[toward > 1.0].mean() > 0.75 and want[toward < -1.0].mean() < 0.1       # (the blob is not convex)
    # without a bias the surface a vertex sits on hides it
    assert not O.visible(R, verts, eye, 0.0).any() and not _np(M.visible_from(index, _dev(verts), _dev(eye), 0.0)).any()


def test_empty(M, blob):
    verts, tris = blob
    o = _dev(np.broadcast_to(O.blob_interior(), (70, 3)))
    d = _dev(np.random.default_rng(1).normal(size=(70, 3)).astype(F))
    for t in (np.zeros((0, 3), np.int64), np.array([[0, 0, 1], [0, 1, 9999]], dtype=np.int64)):     # T = 0, and nothing kept
        index = _index(M, verts, t)
        assert index.corners.shape == (index.n_tiles * 64, 16) and not _np(index.corners).any()
        for cull in (True, False):
            tt, tri, bary, visited = M.cast_rays(index, o, d, cull=cull, return_visited=True)
            assert (_np(tt) == np.inf).all() and (_np(tri) == -1).all() and (_np(bary) == 0).all()
            assert (_np(visited) == (0 if cull else index.n_tiles)).all()
            assert not _np(M.cast_rays(index, o, d, mode="any", cull=cull)).any()
        assert _np(M.visible_from(index, o, o[0] + 1, 0.0)).all()
    index = _index(M, verts, tris)
    tt, tri, bary = M.cast_rays(index, o[:0], d[:0])                          # Q = 0
    assert tt.shape == (0,) and tri.shape == (0,) and bary.shape == (0, 3) and tri.dtype == torch.int32 and tt.dtype == torch.float32
    hit, visited = M.cast_rays(index, rays=torch.zeros((0, 8), device="cuda"), mode="any", return_visited=True)
    assert hit.shape == (0,) and hit.dtype == torch.uint8 and visited.shape == (0,)


def test_on_another_stream(M, blob, outside):
    verts, tris = blob
    o, d, want = outside
    index = _index(M, verts, tris)
    serial = M.cast_rays(index, _dev(o), _dev(d))
    serial_seen = M.visible_from(index, _dev(verts), _dev(o[0]), 1e-3)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        index_s = _index(M, verts, tris)
        got = M.cast_rays(index_s, _dev(o), _dev(d))
        hit = M.cast_rays(index_s, _dev(o), _dev(d), mode="any")
        seen = M.visible_from(index_s, _dev(verts), _dev(o[0]), 1e-3)
    side.synchronize()
    _same(got, tuple(_np(t) for t in serial))
    _same(got, want)
    _same_hit(hit, want)
    assert torch.equal(seen, serial_seen)
