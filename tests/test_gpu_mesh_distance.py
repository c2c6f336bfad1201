"""Mesh distances on the MI355X: mf_surface_records / mf_surface_closest / mf_surface_weights / mf_surface_sample / mf_surface_stats
(csrc/mf_mesh_distance.hip) and MeshIndex / closest_point / sample_surface / surface_distance against the numpy restatement of
their contract (tests/mesh_distance_oracle.py: np.float32, brute force).  Every comparison is equality, with no tolerance and
nothing left out (np.array_equal: a NaN fails it; the sign of a zero is the one thing it does not see, mesh_distance_oracle.py
says why) -- but for the float64 sums, which are held to the bound of ANY summation order, n 2^-52 of the sum of the absolute
terms, and to being identical from run to run.

Launch shape: the closest-point kernel has no grid-stride loop -- a wave per 64 queries, a workgroup per kMdThreads -- so there is
no second trip to reach; md_stats has one, and its case runs past kMdStatBlocks workgroups, read from the source."""
import os
import re

import numpy as np
import pytest
import torch

import mesh_distance_oracle as O

pytestmark = pytest.mark.gpu

_SRC = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "moco_flow_amd", "csrc", "mf_mesh_distance.hip")).read()
THREADS = int(re.search(r"\bconstexpr int kMdThreads = (\d+);", _SRC).group(1))
STAT_BLOCKS = int(re.search(r"\bconstexpr int kMdStatBlocks = (\d+);", _SRC).group(1))
F = np.float32


@pytest.fixture(scope="module")
def M():
    import moco_flow_amd
    assert torch.cuda.is_available()
    moco_flow_amd._lib.lib()
    return moco_flow_amd


@pytest.fixture(scope="module")
def sphere():
    verts, tris = O.uv_sphere()
    assert len(tris) == 4900
    return verts, tris


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.cpu().numpy()


def _index(M, verts, tris, order="morton"):
    return M.MeshIndex(_dev(verts), _dev(tris), order=order)


def _raw(M, index, q, mode, qorder=None, start=None):
    """mf_surface_closest alone, on outputs filled with a sentinel beforehand, so that an unwritten row shows -> (d2, tri, point,
    region, visited)."""
    L = M._lib
    q = _dev(q)
    Q = q.shape[0]
    visited = torch.full(((Q + 63) // 64,), -5, dtype=torch.int32, device="cuda")
    d2 = torch.full((Q,), -7.0, dtype=torch.float32, device="cuda")
    tri = torch.full((Q,), -9, dtype=torch.int32, device="cuda")
    point = torch.full((Q, 3), -7.0, dtype=torch.float32, device="cuda")
    region = torch.full((Q,), 77, dtype=torch.uint8, device="cuda")
    qo = None if qorder is None else _dev(np.asarray(qorder, dtype=np.int32))
    st = None if start is None else _dev(np.asarray(start, dtype=np.int32))
    L.launch(q.device, "mf_surface_closest", L.ptr0(index.records), L.ptr0(index.edges), L.ptr0(index.slot_tri), L.ptr0(index.tile_box), index.T,
             L.ptr0(q), Q, L.ptr0(qo), L.ptr0(st), mode, L.ptr0(d2), L.ptr0(tri), L.ptr0(point), L.ptr0(region), L.ptr0(visited))
    return tuple(_np(t) for t in (d2, tri, point, region, visited))


def _same(got, want, what=""):
    for g, w, name in zip(got, want, ("d2", "tri", "point", "region")):
        g = _np(g) if isinstance(g, torch.Tensor) else g
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, name, int((g != w).sum()))


def _near(verts, tris, n, rng, spread):
    t = rng.integers(len(tris), size=n)
    w = rng.random((n, 3))
    w /= w.sum(1, keepdims=True)
    p = sum(verts[tris[t, k]].astype(np.float64) * w[:, k:k + 1] for k in range(3))
    return (p + rng.normal(size=(n, 3)) * spread).astype(F)


def _records_match(index, R):
    for name in ("records", "edges", "slot_tri", "tile_box", "tri_slot", "area2", "normal", "dropped"):
        got = _np(getattr(index, name))
        assert got.dtype == R[name].dtype and got.shape == R[name].shape and np.array_equal(got, R[name]), name
    assert int(index.dropped_count) == R["dropped_count"]


@pytest.mark.parametrize("T", [1, 63, 64, 65, 130])
def test_tiling_edges(M, sphere, T):
    verts, tris = sphere
    tris = tris[:T]
    rng = np.random.default_rng(T)
    index = _index(M, verts, tris)
    R = O.records(verts, tris, _np(index.order))
    _records_match(index, R)
    for Q in (1, 63, 65, 257):
        q = np.concatenate([_near(verts, tris, Q - Q // 2, rng, 0.05), (rng.random((Q // 2, 3)) * 4 - 2).astype(F)])
        want = O.closest(R, q)
        assert (want[1] >= 0).all()
        for mode in (0, 1):
            _same(_raw(M, index, q, mode), want, (T, Q, mode))
        _same(M.closest_point(_dev(q), index, return_region=True), want, (T, Q))


def test_ties_resolve_to_the_lowest_index(M):
    for verts, tris in (O.cube(), O.octahedron()):
        edges = {tuple(sorted(e)) for t in tris for e in ((t[0], t[1]), (t[1], t[2]), (t[0], t[2]))}
        q = np.concatenate([verts, [(verts[a] + verts[b]) * F(0.5) for a, b in sorted(edges)], verts[tris].mean(1), np.zeros((1, 3))]).astype(F)
        for order in ("identity", "morton", _dev(np.arange(len(tris), dtype=np.int32)[::-1].copy())):
            index = _index(M, verts, tris, order)
            R = O.records(verts, tris, None if index.order is None else _np(index.order))
            want = O.closest(R, q)
            s = R["tri_slot"]
            val = O.tri_value(R["records"][s][None], R["edges"][s][None], q[:, None, :])[0]
            ties = (val == want[0][:, None]).sum(1)
            assert (ties >= 2).sum() >= len(verts) and ties[-1] >= 4                  # every vertex, and the body centre
            assert np.array_equal(want[1], (val == want[0][:, None]).argmax(1))       # the lowest caller's index
            for mode in ("cull", "sweep"):
                _same(M.closest_point(_dev(q), index, mode=mode, return_region=True), want, mode)


@pytest.fixture(scope="module")
def soup_case():
    verts, tris = O.soup()
    rng = np.random.default_rng(29)
    R = O.records(verts, tris)
    kept = np.flatnonzero(R["dropped"] == 0)
    on = _near(verts, tris[kept], 1000, rng, 0.0)
    q = np.concatenate([(rng.random((1500, 3)) * 3).astype(F), on, verts[tris[kept[:500], 0]]]).astype(F)
    assert len(tris) == 2525 and len(q) == 3000
    return verts, tris, R, q, O.closest(R, q)


def test_degenerate_input(M, soup_case):
    verts, tris, R, q, want = soup_case
    assert 25 <= R["dropped_count"] < 525
    index = _index(M, verts, tris)
    _records_match(index, O.records(verts, tris, _np(index.order)))
    assert np.array_equal(_np(index.dropped), R["dropped"]) and int(index.dropped_count) == R["dropped_count"]
    got = M.closest_point(_dev(q), index, return_region=True)
    _same(got, want)
    tri = _np(got[1])
    assert (tri >= 0).all() and not R["dropped"][tri].any() and np.isfinite(_np(got[0])).all() and np.isfinite(_np(got[2])).all()
    sliver_rows = np.flatnonzero((R["area2"] > 0) & (R["area2"] < 1e-5))
    assert len(sliver_rows) > 100 and np.isin(tri, sliver_rows).any()                  # slivers are kept, and win


def test_order_independence(M, soup_case):
    verts, tris, R, q, want = soup_case
    rng = np.random.default_rng(31)
    T = len(tris)
    perm = rng.permutation(T).astype(np.int32)
    qperm = rng.permutation(len(q))
    for order in ("identity", "morton", _dev(perm), _dev(np.arange(T, dtype=np.int32)[::-1].copy())):
        index = _index(M, verts, tris, order)
        assert int(index.dropped_count) == R["dropped_count"]
        for mode in ("cull", "sweep"):
            _same(M.closest_point(_dev(q), index, mode=mode, return_region=True), want, mode)
        got = M.closest_point(_dev(q[qperm]), index, return_region=True)               # the caller's rows in another order
        _same(got, tuple(w[qperm] for w in want))
        n_waves = (len(q) + 63) // 64
        for qorder, start in ((None, None), (qperm, None), (qperm[::-1], rng.integers(-3, index.n_tiles + 3, size=n_waves))):
            _same(_raw(M, index, q, 1, qorder, start), want)                           # any visiting order, any first tile
    # an order that is no permutation drops what it loses and cannot fault
    bad = np.arange(T, dtype=np.int32)
    bad[5], bad[7], bad[70] = 9, T, -1
    index = _index(M, verts, tris, _dev(bad))
    Rb = O.records(verts, tris, bad)
    _records_match(index, Rb)
    _same(M.closest_point(_dev(q), index, return_region=True), O.closest(Rb, q))


def _schedules(M, index, anchors):
    """The four query schedules the walk is pinned under, as (qorder, start) in numpy: as the package derives them; none
    (identity, tile 0); the package's order with every wave starting at the last tile; starts out of range on both sides."""
    qorder, start = (_np(x) for x in M.mesh._schedule(index, anchors))
    n_waves, n = len(start), index.n_tiles
    return ((qorder, start), (None, None), (qorder, np.full(n_waves, n - 1)), (qorder, np.where(np.arange(n_waves) % 2, n + 5, -3)))


@pytest.mark.parametrize("T", [65, 130, 1000])
def test_the_walk_is_the_oracles(M, sphere, T):
    """The tiles each wave evaluates under the cull are closest_culled's, exactly, in four schedules: the visiting order, the
    clamped start and the one decision per wave and tile are the oracle's.  (2, 3 and 16 tiles; two full waves and one of 2.)"""
    verts, tris = sphere
    tris = tris[:T]
    index = _index(M, verts, tris)
    R = O.records(verts, tris, _np(index.order))
    q = _near(verts, tris, 130, np.random.default_rng(T), 0.02)
    want = O.closest(R, q)
    n, counts = index.n_tiles, []
    assert n == -(-T // 64)
    for k, (qorder, start) in enumerate(_schedules(M, index, _dev(q))):
        d2, tri, slot, visited = O.closest_culled(R, q, qorder, start)
        assert np.array_equal(d2, want[0]) and np.array_equal(tri, want[1])
        if k == 3:                                                                     # out of range behaves as clamped
            assert np.array_equal(visited, O.closest_culled(R, q, qorder, np.clip(start, 0, n - 1))[3])
        print(f"T={T} schedule {k}: tiles evaluated per wave {visited} of {n}")
        counts.append(visited)
        got = _raw(M, index, q, 1, qorder, start)
        _same(got, want, (T, k))
        assert got[4].dtype == np.int32 and np.array_equal(got[4], visited), (T, k, got[4], visited)
        assert (_raw(M, index, q, 0, qorder, start)[4] == n).all()
    counts = np.concatenate(counts)
    assert ((counts > 0) & (counts < n)).any()                                         # not vacuous: the oracle itself culls here


def test_cull_equals_sweep_at_size(M):
    verts, tris = O.uv_sphere(110, 100)
    assert len(tris) >= 20000
    rng = np.random.default_rng(37)
    far = rng.normal(size=(10000, 3))
    far = (far / np.linalg.norm(far, axis=1, keepdims=True) * rng.uniform(5, 50, size=(10000, 1))).astype(F)
    q = np.concatenate([far, _near(verts, tris, 10000, rng, 1e-3 / 3)])
    index = _index(M, verts, tris)
    assert int(index.dropped_count) == 0
    sweep = M.closest_point(_dev(q), index, mode="sweep", return_region=True, return_visited=True)
    cull = M.closest_point(_dev(q), index, mode="cull", return_region=True, return_visited=True)
    _same(cull[:4], tuple(_np(t) for t in sweep[:4]))
    assert (_np(sweep[4]) == index.n_tiles).all() and _np(cull[4]).mean() < index.n_tiles / 2      # the cull does cull
    d = np.sqrt(_np(cull[0])[10000:])
    assert d.max() < 5e-3 and np.sqrt(_np(cull[0])[:10000]).min() > 3.5


def test_empty_and_missing(M):
    verts = np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2], [np.nan, 0, 0]], dtype=F)
    q = _dev(np.random.default_rng(1).random((70, 3)).astype(F))
    for tris in (np.array([[0, 1, 2], [0, 0, 1], [0, 1, 9], [0, 1, 3]], dtype=np.int64), np.zeros((0, 3), np.int64)):
        index = _index(M, verts, tris)
        assert int(index.dropped_count) == len(tris) and _np(index.dropped).all() and int(index.cum[-1] if len(tris) else 0) == 0
        for mode in ("cull", "sweep"):
            d2, tri, point, region = M.closest_point(q, index, mode=mode, return_region=True)
            assert (_np(d2) == np.inf).all() and (_np(tri) == -1).all() and (_np(point) == 0).all() and (_np(region) == 0).all()
        points, tri = M.sample_surface(index, 5, draws=(_dev(np.arange(5, dtype=np.int64)), _dev(np.zeros((5, 2), F))))
        assert (_np(tri) == -1).all() and (_np(points) == 0).all()
        d2, tri, point = M.closest_point(q[:0], index)
        assert d2.shape == (0,) and tri.shape == (0,) and point.shape == (0, 3) and tri.dtype == torch.int32


def test_sampling(M, soup_case):
    verts, tris, R, q, _ = soup_case
    rng = np.random.default_rng(41)
    index = _index(M, verts, tris)
    W = O.weights(R["area2"], R["dropped"])
    cum = np.cumsum(W)
    assert np.array_equal(_np(index.weights), W) and np.array_equal(_np(index.cum), cum)
    total = int(cum[-1])
    for n in (1, 63, 65, 1000):
        r = rng.integers(0, 1 << 53, size=n, dtype=np.int64)
        r[0] = (1 << 53) - 1 if n > 1 else 0
        u = rng.random((n, 2)).astype(F)
        want = O.sample(verts, tris, cum, r, u)
        points, tri = M.sample_surface(index, n, draws=(_dev(r), _dev(u)))
        assert np.array_equal(_np(tri), want[1]) and np.array_equal(_np(points), want[0]) and not R["dropped"][want[1]].any(), n
    # the first and the last unit of a triangle's interval
    kept = np.flatnonzero(W > 0)[[0, 1, 100, -1]]
    targets = [t for k in kept for t in (int(cum[k] - W[k]), int(cum[k]) - 1)]
    r = np.array([-(-(t << 53) // total) for t in targets], dtype=np.int64)
    assert O.targets(r, total) == targets
    u = rng.random((len(r), 2)).astype(F)
    points, tri = M.sample_surface(index, len(r), draws=(_dev(r), _dev(u)))
    assert np.array_equal(_np(tri), np.repeat(kept, 2)) and np.array_equal(_np(points), O.sample(verts, tris, cum, r, u)[0])
    # max(1, .): one huge and many tiny triangles
    v = np.array([[0, 0, 0], [1000, 0, 0], [0, 1000, 0]] + [[0, 0, 0], [1e-3, 0, 0], [0, 1e-3, 0]], dtype=F)
    t = np.array([[0, 1, 2]] + [[3, 4, 5]] * 50, dtype=np.int64)
    index = _index(M, v, t)
    Wt = _np(index.weights)
    assert Wt[0] == 1 << 20 and (Wt[1:] == 1).all() and int(index.cum[-1]) == (1 << 20) + 50
    r = np.array([-(-(k << 53) // int(index.cum[-1])) for k in ((1 << 20) - 1, 1 << 20, (1 << 20) + 49)], dtype=np.int64)
    points, tri = M.sample_surface(index, 3, draws=(_dev(r), _dev(np.full((3, 2), 0.25, F))))
    assert _np(tri).tolist() == [0, 1, 50]
    # torch's own draws: every sample on a kept triangle
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    points, tri = M.sample_surface(_index(M, verts, tris), 4096, generator=g)
    assert (_np(tri) >= 0).all() and not R["dropped"][_np(tri)].any() and np.isfinite(_np(points)).all()


def _check_stats(f64, i64, want, n):
    f64, i64 = _np(f64), _np(i64)
    assert i64[:8].tolist() == want["within"] and i64[8] == want["finite"] and i64[9] == want["left_out"] and f64[2] == want["max_d"]
    bound = n * 2.0 ** -52
    for got, key in ((f64[0], "sum_d"), (f64[1], "sum_d2"), (f64[3], "sum_nn")):
        assert abs(got - want[key]) <= bound * abs(want[key]), (key, got, want[key])    # every term is >= 0: the sum of |terms|


@pytest.mark.parametrize("n", [1, 300, STAT_BLOCKS * THREADS + 77])
def test_statistics(M, sphere, n):
    verts, tris = sphere
    rng = np.random.default_rng(n % 1000)
    R = O.records(verts, tris)
    d2 = (rng.random(n) ** 2).astype(F)
    ts = rng.integers(0, len(tris), size=n).astype(np.int32)
    td = rng.integers(0, len(tris), size=n).astype(np.int32)
    if n > 1:
        d2[rng.integers(n, size=n // 50 + 1)] = np.inf
        d2[rng.integers(n, size=n // 50 + 1)] = np.nan
        ts[rng.integers(n, size=n // 40 + 1)] = -1
        td[rng.integers(n, size=n // 40 + 1)] = -1
    tau = (0.0, 0.1, 0.5, 2.0)
    want = O.stats(d2, tau, ts, td, R["normal"], R["normal"])
    normal = _dev(R["normal"])
    runs = [M.surface_stats(_dev(d2), tau, _dev(ts), _dev(td), normal, normal) for _ in range(2)]
    _check_stats(*runs[0], want, n)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    f64, i64 = M.surface_stats(_dev(d2))                                               # no triangle rows, no thresholds
    plain = O.stats(d2)
    _check_stats(f64, i64, plain, n)
    assert plain["left_out"] == 0 and plain["sum_nn"] == 0.0 and plain["finite"] >= want["finite"]
    f64, i64 = M.surface_stats(_dev(d2[:0]))
    assert not _np(f64).any() and not _np(i64).any()


def test_surface_distance(M, sphere):
    verts, tris = sphere
    vb = ((verts - verts.mean(0)) * F(1.01) + verts.mean(0)).astype(F)
    n, tau = 2000, (0.005, 0.0101, 0.02)
    rng = np.random.default_rng(43)
    draws = [(rng.integers(0, 1 << 53, size=n, dtype=np.int64), rng.random((n, 2)).astype(F)) for _ in range(2)]
    a, b = _index(M, verts, tris), _index(M, vb, tris)
    out = M.surface_distance(a, b, n=n, thresholds=tau, draws=tuple((_dev(r), _dev(u)) for r, u in draws))
    Ra, Rb = O.records(verts, tris), O.records(vb, tris)
    want = {}
    for key, (src, dst, (r, u)) in (("a2b", (Ra, Rb, draws[0])), ("b2a", (Rb, Ra, draws[1]))):
        cum = np.cumsum(O.weights(src["area2"], src["dropped"]))
        points, ts = O.sample(src["verts"], src["tris"], cum, r, u)
        d2, td, _, _ = O.closest(dst, points)
        s = O.stats(d2, tau, ts, td, src["normal"], dst["normal"])
        want[key] = s
        got = out[key]
        assert np.array_equal(_np(got["d"]), np.sqrt(d2)) and got["d"].dtype == torch.float32
        _check_stats(got["sums"], torch.cat([got["within"], torch.zeros(8 - len(tau), dtype=torch.int64, device="cuda"), got["finite"].reshape(1),
                                             got["left_out"].reshape(1)]), s, n)
        sums, fin = _np(got["sums"]), float(s["finite"])
        assert s["finite"] == n and s["left_out"] == 0
        assert float(got["mean"]) == sums[0] / fin and float(got["max"]) == s["max_d"]
        assert abs(float(got["rms"]) - np.sqrt(sums[1] / fin)) <= 2.0 ** -52 * np.sqrt(sums[1] / fin)      # one ulp: torch's float64 sqrt
        assert float(got["normal_consistency"]) == sums[3] / fin and float(got["normal_consistency"]) > 0.99
        assert 0.005 < float(got["mean"]) < 0.0101 and s["within"][0] < n and s["within"][2] == n
    assert float(out["chamfer"]) == (float(out["a2b"]["mean"]) + float(out["b2a"]["mean"])) / 2
    P = np.array(want["a2b"]["within"][:3], dtype=np.float64) / want["a2b"]["finite"]
    Rc = np.array(want["b2a"]["within"][:3], dtype=np.float64) / want["b2a"]["finite"]
    assert np.array_equal(_np(out["fscore"]), np.where(P + Rc > 0, 2 * P * Rc / np.where(P + Rc > 0, P + Rc, 1), 0.0))
    pairs = M.surface_distance((_dev(verts), _dev(tris)), b, n=n, thresholds=tau, draws=tuple((_dev(r), _dev(u)) for r, u in draws))
    assert torch.equal(pairs["a2b"]["d"], out["a2b"]["d"]) and torch.equal(pairs["fscore"], out["fscore"])


def test_on_another_stream(M, soup_case):
    verts, tris, R, q, want = soup_case
    index = _index(M, verts, tris)
    serial = M.closest_point(_dev(q), index, return_region=True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        index_s = _index(M, verts, tris)
        got = M.closest_point(_dev(q), index_s, return_region=True)
        r, u = _dev(np.arange(500, dtype=np.int64) << 40), _dev(np.random.default_rng(2).random((500, 2)).astype(F))
        points = M.sample_surface(index_s, 500, draws=(r, u))
        f64, i64 = M.surface_stats(got[0], (0.1,), got[1], got[1], index_s.normal, index_s.normal)
    side.synchronize()
    _same(got, tuple(_np(t) for t in serial))
    _same(got, want)
    ref = M.sample_surface(index, 500, draws=(r, u))
    ref_stats = M.surface_stats(serial[0], (0.1,), serial[1], serial[1], index.normal, index.normal)
    torch.cuda.synchronize()
    assert torch.equal(points[0], ref[0]) and torch.equal(points[1], ref[1])
    assert torch.equal(f64, ref_stats[0]) and torch.equal(i64, ref_stats[1])
