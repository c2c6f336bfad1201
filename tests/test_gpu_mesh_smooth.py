"""Vertex rings and mesh smoothing on the MI355X: vertex_rings (mf_rings_mesh_plan / mf_rings_mesh_emit) and smooth_mesh
(mf_smooth_mesh) against the numpy oracle of their contracts (tests/mesh_smooth_oracle.py), bit for bit (torch.equal on every
output: the rings are integers, a step is a fixed sequence of singly rounded float32 operations, no tolerance is needed):
hand-made meshes, the marching-cubes mesh of a rippled sphere, a height field past the first trip of every kernel, a fan of
long segments whose fill races, a hub at and above the valence cap, one bad index, empty meshes, side streams, and the
``smooth`` keyword of extract_mesh / extract_colored_mesh.  tests/test_mesh_smooth_cpu.py pins on the CPU what these fixtures
hold."""
import numpy as np
import pytest
import torch

import mesh_smooth_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M():
    import moco_flow_amd
    return moco_flow_amd


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def assert_rings(got, want, what=""):
    for name, g, w in zip(("offsets", "ring", "boundary"), got, want):
        w = torch.from_numpy(np.ascontiguousarray(w))
        assert g.is_cuda and g.dtype == w.dtype and tuple(g.shape) == tuple(w.shape), (what, name, g.dtype, tuple(g.shape), tuple(w.shape))
        assert torch.equal(g.cpu(), w), (what, name, int((g.cpu() != w).sum()))


def assert_bits(got, want, what=""):
    want = torch.from_numpy(np.ascontiguousarray(want))
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape), (what, got.dtype, tuple(got.shape))
    g, w = got.cpu().view(torch.int32), want.view(torch.int32)
    assert torch.equal(g, w), (what, int((g != w).any(1).sum()))


# ---------------------------------------------------------------- 1. hand-made meshes
@pytest.mark.parametrize("name", sorted(O.hand_meshes()))
def test_hand_made_meshes(M, name):
    verts, tris = O.hand_meshes()[name]
    want = O.rings(tris, len(verts))
    assert_rings(M.vertex_rings(dev(tris), len(verts)), want, name)
    for iterations in (1, 3):
        for boundary in ("fixed", "free"):
            for mu in (O.MU, None):
                got = M.smooth_mesh(dev(verts), dev(tris), iterations=iterations, mu=mu, boundary=boundary)
                assert_bits(got, O.smooth(verts, tris, iterations, O.LAM, mu, boundary, rings_=want), (name, iterations, boundary, mu))
    got = M.smooth_mesh(dev(verts), dev(tris), iterations=2, lam=0.33, mu=-0.34)
    assert_bits(got, O.smooth(verts, tris, 2, 0.33, -0.34, rings_=want), (name, "lam 0.33"))


# ---------------------------------------------------------------- 2. the sphere
def test_sphere(M):
    verts, tris = O.sphere()
    want = O.expected_rings("sphere")
    rings = M.vertex_rings(dev(tris), len(verts))
    assert_rings(rings, want, "sphere")
    assert not bool(rings[2].any())
    v, t = dev(verts), dev(tris)
    own = M.smooth_mesh(v, t)                                            # 10 iterations at the defaults, rings built inside
    assert_bits(own, O.expected_smooth("sphere", 10), "sphere, defaults")
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")                              # with rings=, nothing is read from the device
    try:
        given = M.smooth_mesh(v, t, rings=rings)
    finally:
        torch.cuda.set_sync_debug_mode(old)
    assert torch.equal(given, own)
    assert v.data_ptr() != own.data_ptr() and torch.equal(v.cpu(), torch.from_numpy(verts))     # the input is left alone


# ---------------------------------------------------------------- 3. past the first trip of every kernel
def test_sheet_past_one_trip(M):
    verts, tris = O.sheet()
    want = O.expected_rings("sheet")
    trip = 2048 * 256
    assert len(verts) > trip and len(tris) > trip and len(want[1]) > trip
    v, t = dev(verts), dev(tris)
    rings = M.vertex_rings(t, len(verts))
    assert_rings(rings, want, "sheet")
    fixed = M.smooth_mesh(v, t, iterations=2, rings=rings)
    assert_bits(fixed, O.expected_smooth("sheet", 2, "fixed"), "sheet, fixed")
    assert_bits(M.smooth_mesh(v, t, iterations=2, boundary="free", rings=rings), O.expected_smooth("sheet", 2, "free"), "sheet, free")
    rim = rings[2]
    assert int(rim.sum()) == 2956 and torch.equal(fixed[rim].view(torch.int32), v[rim].view(torch.int32))


# ---------------------------------------------------------------- 4. long segments, a racing fill
def test_fan_three_runs(M):
    verts, tris = O.fan()
    want_rings, want = O.expected_rings("fan"), O.expected_smooth("fan", 2, "free")
    v, t = dev(verts), dev(tris)
    runs = []
    for k in range(3):
        assert_rings(M.vertex_rings(t, len(verts)), want_rings, ("fan", k))
        runs.append(M.smooth_mesh(v, t, iterations=2, boundary="free"))
        assert_bits(runs[-1], want, ("fan", k))
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])


# ---------------------------------------------------------------- 5. the valence cap
def test_hub_at_and_above_the_cap(M):
    cap = M.mesh.MAX_TRIANGLES_PER_VERTEX
    verts, tris = O.hub(cap)
    want = O.rings(tris, len(verts))
    assert want[0][1] == cap
    assert_rings(M.vertex_rings(dev(tris), len(verts)), want, "hub at the cap")
    assert_bits(M.smooth_mesh(dev(verts), dev(tris), iterations=2, boundary="free"), O.smooth(verts, tris, 2, boundary="free", rings_=want),
                "hub at the cap")
    over_v, over_t = O.hub(cap + 1)
    with pytest.raises(RuntimeError, match="1 vertices are in more than"):
        M.vertex_rings(dev(over_t), len(over_v))
    with pytest.raises(RuntimeError, match="MAX_TRIANGLES_PER_VERTEX"):
        M.smooth_mesh(dev(over_v), dev(over_t))
    sv, st = O.sphere()                                                  # nothing is left behind
    assert_rings(M.vertex_rings(dev(st), len(sv)), O.expected_rings("sphere"), "sphere after the refusal")
    assert_bits(M.smooth_mesh(dev(sv), dev(st)), O.expected_smooth("sphere", 10), "sphere after the refusal")


# ---------------------------------------------------------------- 6. one bad index
@pytest.mark.parametrize("kind", ["index_V", "index_negative", "index_2_40"])
def test_one_bad_index_raises(M, kind):
    """Exactly one bad index in the sphere's triangles: counted, never used as an address (csrc/mf_mesh_smooth.hip `corners`:
    the range test comes before any use of the index, in the counting and in the filling pass)."""
    verts, tris = O.sphere()
    tris = tris.copy()
    tris[3001, 1] = {"index_V": len(verts), "index_negative": -1, "index_2_40": 1 << 40}[kind]
    with pytest.raises(RuntimeError, match=r"1 triangles name a vertex outside \[0, 2482\)"):
        M.vertex_rings(dev(tris), len(verts))
    with pytest.raises(RuntimeError, match="outside"):
        M.smooth_mesh(dev(verts), dev(tris))
    v, t = O.hand_meshes()["octahedron"]
    assert_rings(M.vertex_rings(dev(t), len(v)), O.rings(t, len(v)), "after the refusal")


# ---------------------------------------------------------------- 7. empty cases
def test_empty_cases(M):
    none_v, none_t = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64)
    verts, tris = O.hand_meshes()["octahedron"]
    assert_rings(M.vertex_rings(dev(none_t), 0), O.rings(none_t, 0), "V = 0")
    assert_rings(M.vertex_rings(dev(none_t), 6), O.rings(none_t, 6), "T = 0")
    got = M.smooth_mesh(dev(none_v), dev(none_t))
    assert tuple(got.shape) == (0, 3) and got.dtype == torch.float32 and got.is_cuda
    v = dev(verts)
    got = M.smooth_mesh(v, dev(none_t))                                  # all rings empty: a copy
    assert got.data_ptr() != v.data_ptr()
    assert_bits(got, verts, "no triangles")
    got = M.smooth_mesh(v, dev(tris), iterations=0)
    assert got.data_ptr() != v.data_ptr()
    assert_bits(got, verts, "iterations = 0")
    skipped = np.array([[0, 0, 1], [2, 3, 2], [4, 4, 4]], np.int64)      # every triangle is skipped: T > 0, R = 0
    assert_rings(M.vertex_rings(dev(skipped), 6), O.rings(skipped, 6), "all skipped")
    assert_bits(M.smooth_mesh(v, dev(skipped), boundary="free"), verts, "all skipped")
    with pytest.raises(RuntimeError, match="3 triangles name a vertex outside"):
        M.vertex_rings(dev(skipped), 0)


# ---------------------------------------------------------------- 8. streams
def test_side_streams(M):
    verts, tris = O.sphere()
    want = O.expected_smooth("sphere", 10)
    moved = (verts[:, [2, 0, 1]] * np.float32(1.5)).astype(np.float32)
    want_moved = O.smooth(moved, tris, 10, rings_=O.expected_rings("sphere"))
    v, w, t = dev(verts), dev(moved), dev(tris)
    rings = M.vertex_rings(t, len(verts))
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        alone = M.smooth_mesh(v, t)
    s1.synchronize()
    assert_bits(alone, want, "side stream")
    outs = []
    for k in range(4):                                                   # two calls in flight on two streams, several times over
        with torch.cuda.stream(s1):
            a = M.smooth_mesh(v, t, rings=rings)
        with torch.cuda.stream(s2):
            b = M.smooth_mesh(w, t, rings=rings)
        outs.append((a, b))
    torch.cuda.synchronize()
    for k, (a, b) in enumerate(outs):
        assert_bits(a, want, ("stream 1", k))
        assert_bits(b, want_moved, ("stream 2", k))


# ---------------------------------------------------------------- 9, 10. wiring
def mesh_models():
    from test_gpu_mesh_components import mesh_models as models          # the suite's small test NeRF (raw sigma crosses 10)
    return models()


def test_extract_mesh_smooth(M):
    nerf, embs = mesh_models()
    Ng = 32
    kw = dict(N_grid=Ng, sigma_threshold=10)
    post = lambda p: p[:, [1, 0, 2]] / Ng * 3.0 - 1.5
    with torch.no_grad():
        verts, tris = M.extract_mesh(nerf, embs[0], **kw)
        none = M.extract_mesh(nerf, embs[0], smooth=None, **kw)
        assert torch.equal(verts, none[0]) and torch.equal(tris, none[1])
        sigma = M.query_sigma(M.mesh.lattice(Ng, verts.device), nerf, embs[0]).view(Ng, Ng, Ng)
        raw, rt = M.marching_cubes(sigma, 10, clamp_zero=True)
        got = M.extract_mesh(nerf, embs[0], smooth=3, **kw)
        sv = M.smooth_mesh(raw, rt, iterations=3)
        assert torch.equal(got[0], post(sv)) and torch.equal(got[1], rt[:, [0, 2, 1]]) and torch.equal(got[1], tris)
        assert_bits(sv, O.smooth(raw.cpu().numpy(), rt.cpu().numpy(), 3), "the isosurface")
        assert not torch.equal(got[0], verts)
        fv, ft = M.filter_components(raw, rt, keep_largest=1)            # after the filter and the clustering
        kv, kt = M.simplify_mesh(fv, ft, 2, lo=(0, 0, 0), hi=(Ng - 1,) * 3)
        both = M.extract_mesh(nerf, embs[0], smooth=3, keep_largest=1, simplify=2, **kw)
        assert torch.equal(both[0], post(M.smooth_mesh(kv, kt, iterations=3))) and torch.equal(both[1], kt[:, [0, 2, 1]])
        spec = dict(iterations=2, lam=0.4, mu=None, boundary="free")
        by_dict = M.extract_mesh(nerf, embs[0], smooth=spec, **kw)
        assert torch.equal(by_dict[0], post(M.smooth_mesh(raw, rt, **spec))) and torch.equal(by_dict[1], tris)
    print(f"extract_mesh N_grid {Ng} smooth 3: V {len(raw)}, T {len(rt)}, {int(M.vertex_rings(rt, len(raw))[2].sum())} boundary vertices")


def test_extract_colored_mesh_smooth(M):
    from test_gpu_mesh_components import IND_SCALAR
    nerf, embs = mesh_models()
    Ng = 32
    kw = dict(N_grid=Ng, sigma_threshold=10, ind=IND_SCALAR)
    with torch.no_grad():
        plain = M.extract_colored_mesh(nerf, embs, **kw)
        none = M.extract_colored_mesh(nerf, embs, smooth=None, **kw)
        for x, y in zip(plain, none):
            assert torch.equal(x, y)
        verts, tris, normals, colors = M.extract_colored_mesh(nerf, embs, smooth=3, **kw)
        mesh = M.extract_mesh(nerf, embs[0], smooth=3, **kw)
        assert torch.equal(verts, mesh[0]) and torch.equal(tris, mesh[1]) and not torch.equal(verts, plain[0])
        assert torch.equal(normals, plain[2]) and torch.equal(colors, plain[3]) and torch.equal(tris, plain[1])
        empty = M.extract_colored_mesh(nerf, embs, smooth=3, min_triangles=len(tris) + 1, **kw)
    assert len(verts) > 0 and [tuple(x.shape) for x in empty] == [(0, 3)] * 4
