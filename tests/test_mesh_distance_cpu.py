"""CPU-side checks (-m "not gpu") of the mesh distances (csrc/mf_mesh_distance.hip; MeshIndex, closest_point, sample_surface,
surface_distance): the fp32 contract against its float64 evaluation; the ordering of the bounds that lets a tile be skipped
without slack; the culled search, restated in numpy, against brute force; the integer sampling rules; the library's exports and
prototypes; every refusal that is made before a launch.  None of it touches a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import mesh_distance_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mf_surface_records", "mf_surface_closest", "mf_surface_weights", "mf_surface_sample", "mf_surface_stats_scratch_bytes", "mf_surface_stats")
F = np.float32
SIDE = 3.0


def morton(points, lo, hi):
    c = np.clip((points - lo) / (hi - lo) * 1024, 0, 1023).astype(np.int64)
    code = np.zeros(len(points), np.int64)
    for bit in range(10):
        for axis in range(3):
            code |= ((c[:, axis] >> bit) & 1) << (3 * bit + 2 - axis)
    return code


@pytest.fixture(scope="module")
def soup():
    verts, tris = O.soup()
    R = O.records(verts, tris)
    rng = np.random.default_rng(3)
    kept = np.flatnonzero(R["dropped"] == 0)
    tk = kept[rng.integers(len(kept), size=900)]
    a, b, c = (verts[tris[tk, k]] for k in range(3))
    w = rng.random((300, 3)).astype(F)
    w /= w.sum(1, keepdims=True)
    q = np.concatenate([rng.random((1500, 3)).astype(F) * F(SIDE), a[:300], (a[300:600] + b[300:600]) * F(0.5),
                        a[600:] * w[:, :1] + b[600:] * w[:, 1:2] + c[600:] * w[:, 2:]]).astype(F)     # in space, on vertices, edges, faces
    return verts, tris, R, q


def test_fp32_contract_against_its_float64_evaluation(soup):
    """Measured on the soup (2 000 random triangles, 500 slivers of width 1e-6, side L = 3; 1 500 queries in space, 300 on
    vertices, 300 on edge midpoints, 300 on faces): the fp32 distance lies within -0.59 .. +1.41 eps L of the float64
    evaluation of the same expressions.  RECORDED = 1.41; the assertion allows four times that."""
    RECORDED = 1.41
    verts, tris, R, q = soup
    assert R["T"] == 2525 and 25 <= R["dropped_count"] < 525
    d2, tri, point, region = O.closest(R, q)
    assert np.isfinite(d2).all() and (tri >= 0).all() and np.isfinite(point).all() and not R["dropped"][tri].any()
    assert set(np.unique(region)) == {0, 1, 2, 3}
    err = (np.sqrt(d2.astype(np.float64)) - np.sqrt(O.closest_f64(R, q))) / (np.finfo(F).eps * SIDE)
    print("fp32 - float64 distance, in eps L:", err.min(), err.max())
    assert np.abs(err).max() <= 4 * RECORDED


def test_bounds_are_ordered_under_rounding(soup):
    """lb(wave box, tile box) <= lb(q, tile box) <= lb(q, triangle box) <= value, with equality allowed and no violation: what
    lets a wave skip a tile on the strict test with no slack."""
    verts, tris, R, q = soup
    rng = np.random.default_rng(11)
    n = len(R["tile_box"])
    checked = 0
    for trial in range(40):
        t = int(rng.integers(n))
        centre = q[rng.integers(len(q))]
        qq = (centre + rng.normal(size=(64, 3)).astype(F) * F(rng.choice([1e-3, 0.1, 2.0]))).astype(F)
        qlo, qhi = qq.min(0), qq.max(0)
        tlo, thi = R["tile_box"][t, 0:3], R["tile_box"][t, 3:6]
        g = np.fmax(np.fmax(tlo - qhi, qlo - thi), F(0))
        lb_wave = O.dot(g, g)
        lb_lane = O.box_lb(qq, tlo, thi)
        sl = slice(t * 64, t * 64 + 64)
        keep = R["slot_tri"][sl] >= 0
        val, _, _, lb_tri = O.tri_value(R["records"][sl][keep][None], R["edges"][sl][keep][None], qq[:, None, :])
        assert lb_wave.dtype == lb_lane.dtype == lb_tri.dtype == val.dtype == F
        assert (lb_wave <= lb_lane).all() and (lb_lane[:, None] <= lb_tri).all() and (lb_tri <= val).all()
        checked += val.size
    assert checked > 100000
    # and the clamp seldom binds: the value is the least candidate but for rounding
    val, _, _, lb = O.tri_value(R["records"][:640][None], R["edges"][:640][None], q[:200, None, :])
    keep = R["slot_tri"][:640] >= 0
    assert (lb[:, keep] <= val[:, keep]).all()


def test_culled_search_equals_brute_force_for_three_orders(soup):
    verts, tris, R, q = soup
    rng = np.random.default_rng(17)
    T = R["T"]
    vv = np.concatenate([verts, np.zeros((1, 3), F)])
    cen = vv[np.clip(tris, 0, len(verts))].mean(1)
    lo, hi = cen.min(0), cen.max(0)
    codes = morton(cen, lo, hi)
    qq = q[rng.permutation(len(q))[:320]]
    qcodes = morton(qq, lo, hi)
    qorder = np.argsort(qcodes, kind="stable")
    want = O.closest(R, qq)
    skipped = False
    for name, order in (("morton", np.argsort(codes, kind="stable")), ("identity", None), ("random", rng.permutation(T))):
        Ro = O.records(verts, tris, order)
        assert Ro["dropped_count"] == R["dropped_count"] and np.array_equal(Ro["dropped"], R["dropped"])
        slot_codes = codes if order is None else codes[order]
        start = np.clip(np.searchsorted(slot_codes[::64], qcodes[qorder][::64], side="right") - 1, 0, len(Ro["tile_box"]) - 1)
        for kw in (dict(qorder=qorder, start=start), dict()):
            d2, tri, slot, visited = O.closest_culled(Ro, qq, **kw)
            assert np.array_equal(d2, want[0]) and np.array_equal(tri, want[1]), name
            assert np.array_equal(Ro["slot_tri"][slot], tri)
            skipped |= bool((visited < len(Ro["tile_box"])).any())
        d2, tri, _, visited = O.closest_culled(Ro, qq, cull=False)
        assert np.array_equal(d2, want[0]) and np.array_equal(tri, want[1]) and (visited == len(Ro["tile_box"])).all()
    assert skipped                                                           # the cull did cull: the case is not vacuous
    # a bad order drops triangles and nothing else: repeats keep the lowest slot, an entry out of range leaves its slot empty
    order = np.arange(T)
    order[5], order[7], order[70] = 9, T, -1
    Rb = O.records(verts, tris, order)
    lost = {5, 7, 70}
    assert all(Rb["dropped"][t] for t in lost) and Rb["slot_tri"][5] in (9, -1) and Rb["slot_tri"][7] == -1 and Rb["slot_tri"][9] == -1
    assert Rb["dropped_count"] == int((R["dropped"] | np.isin(np.arange(T), list(lost))).sum())


def test_dropped_triangles_have_no_weight_and_are_never_sampled(soup):
    verts, tris, R, q = soup
    W = O.weights(R["area2"], R["dropped"])
    assert W.dtype == np.int64 and (W[R["dropped"] != 0] == 0).all() and (W[R["dropped"] == 0] >= 1).all() and W.max() == O.WEIGHT_ONE
    cum = np.cumsum(W)
    rng = np.random.default_rng(23)
    r = rng.integers(0, 1 << 53, size=20000, dtype=np.int64)
    r[:2] = 0, (1 << 53) - 1
    u = rng.random((20000, 2)).astype(F)
    points, tri = O.sample(verts, tris, cum, r, u)
    assert (tri >= 0).all() and not R["dropped"][tri].any() and np.isfinite(points).all()
    # max(1, .): one huge and many tiny triangles
    v = np.array([[0, 0, 0], [1000, 0, 0], [0, 1000, 0]] + [[0, 0, 0], [1e-3, 0, 0], [0, 1e-3, 0]], dtype=F)
    t = np.array([[0, 1, 2]] + [[3, 4, 5]] * 50, dtype=np.int64)
    Rt = O.records(v, t)
    Wt = O.weights(Rt["area2"], Rt["dropped"])
    assert Wt[0] == O.WEIGHT_ONE and (Wt[1:] == 1).all()
    # the first and the last unit of a triangle's interval: target = cum[t - 1] and cum[t] - 1 both pick t
    total = int(cum[-1])
    kept = np.flatnonzero(W > 0)[[0, 5, -1]]
    for t_ in kept:
        for target in (int(cum[t_] - W[t_]), int(cum[t_]) - 1):
            r1 = -(-(target << 53) // total)                                 # the least r with floor(r total / 2^53) = target
            assert O.targets([r1], total) == [target]
            assert O.sample(verts, tris, cum, [r1], np.zeros((1, 2), F))[1][0] == t_


def test_target_stays_below_total():
    for total in (1, 2, 3, 1 << 20, (1 << 20) + 1, (1 << 51) - 1, 1 << 51):
        top = O.targets([(1 << 53) - 1, -1, 1 << 53], total)                 # -1 and 2^53 are masked to 2^53 - 1 and 0
        assert top[0] == top[1] == total - 1 < total and top[2] == 0
        assert O.targets([0], total) == [0]


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
    assert L.SYMBOLS["mf_surface_records"] == (i32, [p, i64, p, i64] + [p] * 11)
    assert L.SYMBOLS["mf_surface_closest"] == (i32, [p, p, p, p, i64, p, i64, p, p, i32, p, p, p, p, p, p])
    assert L.SYMBOLS["mf_surface_weights"] == (i32, [p, p, i64, p, p, p])
    assert L.SYMBOLS["mf_surface_sample"] == (i32, [p, i64, p, i64, p, p, p, i64, p, p, p])
    assert L.SYMBOLS["mf_surface_stats_scratch_bytes"] == (i64, [i64])
    assert L.SYMBOLS["mf_surface_stats"] == (i32, [p, i64, p, p, p, i64, p, i64, C.POINTER(C.c_float), i32, p, p, p, p])
    for name in ("MeshIndex", "closest_point", "sample_surface", "surface_distance", "surface_stats"):
        assert name in M.__all__ and callable(getattr(M, name)), name
    make = open(os.path.join(ROOT, "moco_flow_amd", "csrc", "Makefile")).read()
    assert "mf_mesh_distance.hip" in re.search(r"^SRCS = (.*)$", make, re.M).group(1).split()
    unit = open(os.path.join(ROOT, "moco_flow_amd", "csrc", "mf_mesh_distance.hip")).read()
    assert "#pragma clang fp contract(off)" in unit
    for name in ("kMdThreads", "kMdTile", "kMdStatBlocks"):
        assert re.search(rf"constexpr int {name} = \d+;", unit), name
    assert "atomicAdd(float" not in unit and "atomicAdd(double" not in unit


def test_host_side_validation():
    """Counts, the mode, null pointers and aliasing are settled on the host, before anything is launched: the fake pointers are
    never touched."""
    import moco_flow_amd._lib as L
    lib = L.lib()
    ptrs = [C.c_void_p(256 * (k + 1)) for k in range(16)]
    big = (1 << 31) - 1

    def rec(**k):
        a = dict(verts=ptrs[0], V=8, tris=ptrs[1], T=4, order=None, out=ptrs[2:11])
        a.update(k)
        return lib.mf_surface_records(a["verts"], a["V"], a["tris"], a["T"], a["order"], *a["out"], None)

    for bad in (dict(V=-1), dict(T=-1), dict(V=big), dict(T=big), dict(V=1 << 40)):
        assert rec(**bad) == -1 and b"2^31 - 1" in lib.mf_last_error(), bad
    assert rec(tris=None) == -1 and b"null" in lib.mf_last_error()
    assert rec(verts=None) == -1 and b"null verts" in lib.mf_last_error()
    for k in range(9):
        out = list(ptrs[2:11])
        out[k] = None
        assert rec(out=out) == -1 and b"null" in lib.mf_last_error(), k
        out[k] = ptrs[0] if k != 8 else ptrs[1]
        assert rec(out=out) == -1 and b"aliases" in lib.mf_last_error(), k
    assert rec(order=ptrs[2]) == -1 and b"aliases" in lib.mf_last_error()

    def closest(**k):
        a = dict(index=ptrs[0:4], T=4, query=ptrs[4], Q=5, qorder=ptrs[5], start=ptrs[6], mode=1, out=ptrs[7:12])
        a.update(k)
        return lib.mf_surface_closest(*a["index"], a["T"], a["query"], a["Q"], a["qorder"], a["start"], a["mode"], *a["out"], None)

    for bad in (dict(T=-1), dict(Q=-1), dict(T=big), dict(Q=big)):
        assert closest(**bad) == -1 and b"2^31 - 1" in lib.mf_last_error(), bad
    for mode in (-1, 2):
        assert closest(mode=mode) == -1 and b"mode=%d" % mode in lib.mf_last_error()
    assert closest(Q=0, query=None, out=[None] * 5) == 0                    # nothing to launch, nothing looked at
    for k in range(4):
        index = list(ptrs[0:4])
        index[k] = None
        assert closest(index=index) == -1 and b"null" in lib.mf_last_error(), k
    assert closest(query=None) == -1 and b"null" in lib.mf_last_error()
    for k in range(3):
        out = list(ptrs[7:12])
        out[k] = None
        assert closest(out=out) == -1 and b"null" in lib.mf_last_error(), k
    for k in range(5):
        out = list(ptrs[7:12])
        out[k] = ptrs[4]
        assert closest(out=out) == -1 and b"aliases" in lib.mf_last_error(), k

    assert lib.mf_surface_weights(ptrs[0], ptrs[1], -1, ptrs[2], ptrs[3], None) == -1 and b"T=-1" in lib.mf_last_error()
    assert lib.mf_surface_weights(ptrs[0], ptrs[1], 4, None, ptrs[3], None) == -1 and b"null" in lib.mf_last_error()
    assert lib.mf_surface_weights(ptrs[0], ptrs[1], 4, ptrs[2], ptrs[0], None) == -1 and b"aliases" in lib.mf_last_error()
    assert lib.mf_surface_weights(None, None, 0, None, None, None) == 0

    def sample(**k):
        a = dict(verts=ptrs[0], V=8, tris=ptrs[1], T=4, cum=ptrs[2], r=ptrs[3], u=ptrs[4], n=6, points=ptrs[5], tri=ptrs[6])
        a.update(k)
        return lib.mf_surface_sample(a["verts"], a["V"], a["tris"], a["T"], a["cum"], a["r"], a["u"], a["n"], a["points"], a["tri"], None)

    for bad in (dict(V=-1), dict(T=big), dict(n=-1), dict(n=big)):
        assert sample(**bad) == -1 and b"2^31 - 1" in lib.mf_last_error(), bad
    for null in ("verts", "tris", "cum", "r", "u", "points", "tri"):
        assert sample(**{null: None}) == -1 and b"null" in lib.mf_last_error(), null
    assert sample(points=ptrs[0]) == -1 and b"aliases" in lib.mf_last_error()
    assert sample(n=0, points=None, tri=None) == 0

    def stats(**k):
        a = dict(d2=ptrs[0], n=9, tau=(C.c_float * 8)(), k=2, f64=ptrs[1], i64=ptrs[2], scratch=ptrs[3])
        a.update(k)
        return lib.mf_surface_stats(a["d2"], a["n"], None, None, None, 0, None, 0, a["tau"], a["k"], a["f64"], a["i64"], a["scratch"], None)

    for bad in (dict(n=-1), dict(n=big)):
        assert stats(**bad) == -1 and b"2^31 - 1" in lib.mf_last_error(), bad
    for bad in (dict(k=-1), dict(k=9), dict(tau=None)):
        assert stats(**bad) == -1 and b"n_thresholds" in lib.mf_last_error(), bad
    for null in ("d2", "f64", "i64", "scratch"):
        assert stats(**{null: None}) == -1 and b"null" in lib.mf_last_error(), null
    size = lib.mf_surface_stats_scratch_bytes
    assert size(-1) == -1 and size(big) == -1 and b"2^31 - 1" in lib.mf_last_error()
    # 13 float64 sums and one maximum per workgroup of 256 rows, at most 1024 workgroups
    assert size(0) == 0 and size(1) == 112 + 16 and size(257) == 208 + 16 and size(1 << 30) == 1024 * (104 + 8)
    with pytest.raises(RuntimeError, match="2\\^31 - 1"):
        L.need("mf_surface_stats_scratch_bytes", -5)


def test_argument_validation_needs_no_gpu():
    import moco_flow_amd as M
    verts, tris = torch.zeros(5, 3), torch.zeros(4, 3, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        M.MeshIndex(verts, tris)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        M.surface_distance((verts, tris), (verts, tris))
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        M.surface_stats(torch.zeros(4))
    with pytest.raises(RuntimeError, match="int64"):
        M.MeshIndex(verts, tris.int())
    with pytest.raises(RuntimeError, match="MeshIndex"):
        M.closest_point(torch.zeros(3, 3), (verts, tris))
    with pytest.raises(RuntimeError, match="MeshIndex"):
        M.sample_surface((verts, tris), 4)
