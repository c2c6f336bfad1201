"""The ray-cast contract of csrc/mf_mesh_rays.hip judged on the CPU, through its numpy restatement alone
(tests/mesh_rays_oracle.py; no GPU): that it is watertight where a plain fp32 Moeller-Trumbore is not, that the tile predicate
never rejects the tile of an accepted triangle (P1), and that what it returns is the float64 answer to fp32 accuracy.  The
kernels are held to the oracle bit for bit in tests/test_gpu_mesh_rays.py, so the float64 bound here only guards the contract's
sanity.  Plus the ABI bookkeeping of the two new entry points."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mesh_rays_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mf_surface_corners", "mf_surface_cast")
F = np.float32


@pytest.fixture(scope="module")
def case():
    verts, tris = O.blob()
    assert len(tris) == 1280 and len(verts) == 642
    R = O.records(verts, tris)
    assert R["dropped_count"] == 0 and len(R["tile_box"]) == 20
    families = O.ray_families(verts, tris, O.blob_interior())
    d = np.concatenate(list(families.values()))
    assert {k: len(v) for k, v in families.items()} == dict(vertices=642, edges=5760, centroids=1280, random=3000, axes=18)
    o = np.broadcast_to(O.blob_interior(), d.shape)
    return dict(R=R, families=families, o=o, d=d, cast=O.cast(R, o, d))


def test_every_ray_from_inside_hits(case):
    t, tri, bary, hit = case["cast"]
    assert hit.all() and (tri >= 0).all() and np.isfinite(t).all() and (t > 0).all()
    assert np.abs(bary.sum(1) - 1).max() < 1e-5 and bary.min() > -1e-5
    # the thing the contract replaces loses rays between triangles on the same input
    _, tri32, _ = O.moller_trumbore(case["R"], case["o"], case["d"], dtype=np.float32)
    print("plain fp32 Moeller-Trumbore missed", int((tri32 < 0).sum()), "of", len(tri32))
    assert (tri32 < 0).sum() > 0


def test_tile_predicate_passes_every_accepted_triangle(case):
    R = case["R"]
    ray = O.setup(case["o"], case["d"])
    t_first = case["cast"][0]
    wanted = O.tile_wanted(R, ray)                                          # best = +inf: before anything is found
    wanted_late = O.tile_wanted(R, ray, best=t_first)                       # best = the final answer: the tightest it gets
    z0 = O.tile_intervals(R, ray)[4]
    accepted = 0
    for i in range(0, ray["Q"], 800):
        kept, _, _, _, _, t, acc = O.evaluate(R, O._rows(ray, slice(i, i + 800)))
        q, k = np.nonzero(acc)
        tile = R["tri_slot"][kept[k]] // O.TILE
        assert wanted[i + q, tile].all() and (z0[i + q, tile] <= t[q, k]).all()
        win = t[q, k] == t_first[i + q]                                     # every accepted triangle at the winning t, ties included
        assert wanted_late[i + q[win], tile[win]].all()
        accepted += len(q)
    assert accepted >= ray["Q"]
    assert wanted.sum(1).mean() < len(R["tile_box"]) / 2                    # and it does reject


def test_the_culled_cast_equals_the_brute_force():
    """cast_culled -- the walk of a wave, tile by tile -- returns what cast does: cull on and off, both modes, the rays in
    identity order from tile 0, and sorted as the slots are from the tile in the middle."""
    verts, tris = O.blob()
    lo, hi = verts.min(0), verts.max(0)

    def cell(p):                                                            # a 6-bit Morton code: 4 cells per axis over the mesh's box
        g = np.clip((p - lo) / (hi - lo) * 4, 0, 3).astype(np.int64)
        return sum(((g[:, a] >> b) & 1) << (3 * b + 2 - a) for a in range(3) for b in range(2))
    R = O.records(verts, tris, np.argsort(cell(verts[tris].mean(1)), kind="stable"))      # compact tiles
    n = len(R["tile_box"])
    assert n == 20
    rng = np.random.default_rng(61)
    d = rng.normal(size=(150, 3)).astype(F)
    o = np.tile(O.blob_interior(), (150, 1))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o[128:] += d[128:] * F(4)                                               # the last wave: from outside, looking back or past
    d[128:] = -d[128:] + rng.normal(size=(22, 3)).astype(F) * F(0.3)
    d[7] = 0                                                                # a dead ray
    want = O.cast(R, o, d, 0.0, np.inf)
    assert 128 < want[3].sum() < 149
    n_waves = 3
    by_cell = np.concatenate([np.argsort(cell(o[:128] + d[:128]), kind="stable"), np.arange(128, 150)])
    for qorder, start in ((None, None), (by_cell, np.full(n_waves, n // 2))):
        counts = {}
        for cull in (True, False):
            for mode in (0, 1):
                got = O.cast_culled(R, o, d, 0.0, np.inf, mode, qorder, start, cull)
                counts[cull, mode] = got[4]
                if mode == 0:
                    assert all(g.dtype == w.dtype and np.array_equal(g, w) for g, w in zip(got[:3], want[:3])), (cull, mode)
                else:
                    assert np.array_equal(got[3], want[3])
            assert cull or all((counts[cull, mode] == n).all() for mode in (0, 1))
    print("tiles evaluated per wave, rays sorted: first", counts[True, 0], "any", counts[True, 1])
    assert counts[True, 1].sum() < counts[True, 0].sum() < n * n_waves      # sorted rays: the cull does cull, any hit more so


def test_against_float64(case):
    n = len(case["families"]["random"])
    sl = slice(len(case["d"]) - n - 18, len(case["d"]) - 18)                # the 3 000 random rays
    o, d = case["o"][sl], case["d"][sl]
    assert n == 3000 and np.array_equal(d, case["families"]["random"])
    t, tri, bary = (x[sl] for x in case["cast"][:3])
    t64, tri64, uv = O.moller_trumbore(case["R"], o, d)
    assert (tri64 >= 0).all()
    b64 = np.stack([1 - uv.sum(1), uv[:, 0], uv[:, 1]], -1)
    near = b64.min(1) < 1e-4                                                # the float64 hit within 1e-4 of an edge: either side may win
    print("left out", int(near.sum()), "of", n)
    assert near.sum() <= n // 100
    assert np.array_equal(tri[~near], tri64[~near])
    rel = (np.abs(t.astype(np.float64) - t64) / t64)[~near].max()
    print("largest relative error of t", rel, "of bary", np.abs(bary - b64)[~near].max())
    assert rel <= 4 * 2.7314e-7                                             # observed on this input: 2.73e-7
    assert np.abs(bary - b64)[~near].max() <= 4 * 5.01e-7                   # observed: 5.01e-7


def test_dead_rays_and_ranges():
    verts, tris = O.blob(1)
    R = O.records(verts, tris)
    o = np.tile(O.blob_interior(), (8, 1))
    d = np.tile(np.array([[0.3, -0.2, 1.0]], F), (8, 1))
    first = O.cast(R, o[:1], d[:1])[0][0]
    d[1] = 0
    d[2, 1] = np.nan
    o[3, 0] = np.inf
    t_min = np.array([0, 0, 0, 0, 1, 0, np.nextafter(first, F(np.inf)), np.nan], F)
    t_max = np.array([np.inf, np.inf, np.inf, np.inf, 0.5, np.nextafter(first, F(0)), np.inf, np.inf], F)
    t, tri, bary, hit = O.cast(R, o, d, t_min, t_max)
    assert hit.tolist() == [1, 0, 0, 0, 0, 0, 0, 0] and (tri[1:] == -1).all() and np.isinf(t[1:]).all() and not bary[1:].any()
    back = O.cast(R, o[:1], -d[:1], -np.inf, 0.0)                           # behind the origin, with the range opened to it
    assert back[3][0] == 1 and back[0][0] < 0


def test_abi_is_additive():
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
    assert L.SYMBOLS["mf_surface_corners"] == (i32, [p, i64, p, i64, p, p, p])
    assert L.SYMBOLS["mf_surface_cast"] == (i32, [p, p, p, i64, p, p, i64, p, p, i64, i64, p, p, i32, i32, p, p, p, p, p, p])
    # refusals are settled before any launch: none of these reaches the device
    one = (C.c_float * 16)()
    for args in ((None, 1, None, -1, None, None), (None, 0, None, 1, None, None)):
        assert lib.mf_surface_corners(*args, None) == -1 and b"mf_surface_corners" in lib.mf_last_error()
    ok = [one, one, one, 1, one, one, 3, one, one, 0, 1, None, None, 0, 1, None, None, None, None, None]
    for k, bad in ((13, 2), (14, -1), (6, 2), (9, -1), (10, -1), (4, None)):
        args = list(ok)
        args[k] = bad
        assert lib.mf_surface_cast(*args, None) == -1 and b"mf_surface_cast" in lib.mf_last_error(), k
    assert lib.mf_surface_cast(*ok, None) == -1 and b"null t, tri or bary" in lib.mf_last_error()
