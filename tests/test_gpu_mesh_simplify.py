"""Mesh simplification on the MI355X: simplify_mesh (mf_simplify_mesh_plan / mf_simplify_mesh_emit, mf_gather_rows) against
the numpy oracle of its contract (tests/mesh_simplify_oracle.py), bit for bit (torch.equal on every output: new vertices under
both placements, triangles, first, cluster, attribute rows -- the arithmetic is integers plus singly rounded float64, no
tolerance is needed): hand-made meshes, the marching-cubes mesh of a rippled sphere, a height field past the first trip of
every kernel, a fan whose triangles race for a handful of slots, the duplicate table at its smallest legal size, bad input,
the ``simplify`` keyword of extract_mesh / extract_colored_mesh, and empty meshes.  tests/test_mesh_simplify_cpu.py proves on
the CPU that the oracle's results on these meshes are not trivial."""
import numpy as np
import pytest
import torch

import mesh_simplify_oracle as S

pytestmark = pytest.mark.gpu
NAMES = ("verts_k", "tris_k", "attr_k", "first", "cluster")


@pytest.fixture(scope="module")
def M():
    import moco_flow_amd
    return moco_flow_amd


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(M, verts, tris, cell, lo=None, hi=None, placement="mean", **kw):
    """simplify_mesh on the device with the oracle's attribute: (verts_k, tris_k, attr_k, first, cluster)."""
    out = M.simplify_mesh(dev(verts), dev(tris), cell, lo=lo, hi=hi, placement=placement, attrs=(dev(S.attribute(len(verts))),),
                          return_map=True, **kw)
    torch.cuda.synchronize()
    assert len(out) == 5
    return out


def assert_equal(got, want, what=""):
    """The device's five tensors against the oracle's (verts_k, tris_k, first, cluster, attr_k), bit for bit."""
    want = (want[0], want[1], want[4], want[2], want[3])
    for name, g, w in zip(NAMES, got, want):
        w = torch.from_numpy(np.ascontiguousarray(w))
        assert g.is_cuda and g.dtype == w.dtype and tuple(g.shape) == tuple(w.shape), (what, name, g.dtype, tuple(g.shape), tuple(w.shape))
        g = g.cpu()
        if g.dtype == torch.float32:
            g, w = g.view(torch.int32), w.view(torch.int32)
        assert torch.equal(g, w), (what, name, int((g != w).sum()))


def same(a, b):
    return all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a, b)) and len(a) == len(b)


# ---------------------------------------------------------------- 1. hand-made meshes
@pytest.mark.parametrize("name", sorted(S.hand_meshes()))
@pytest.mark.parametrize("placement", ["mean", "first"])
def test_hand_made_meshes(M, name, placement):
    verts, tris, cell, lo, hi = S.hand_meshes()[name]
    want = S.simplify(verts, tris, cell, lo, hi, placement, attrs=(S.attribute(len(verts)),))
    assert_equal(run(M, verts, tris, cell, lo, hi, placement), want, (name, placement))
    plain = M.simplify_mesh(dev(verts), dev(tris), cell, lo=lo, hi=hi, placement=placement)      # no attributes, no map
    assert len(plain) == 2 and torch.equal(plain[0].cpu(), torch.from_numpy(want[0])) and torch.equal(plain[1].cpu(), torch.from_numpy(want[1]))


# ---------------------------------------------------------------- 2. a marching-cubes mesh
@pytest.mark.parametrize("cell", S.SPHERE_CELLS)
@pytest.mark.parametrize("given", [True, False])
def test_sphere(M, cell, given):
    verts, tris = S.sphere()
    lo, hi = S.SPHERE_BOUNDS if given else (None, None)
    for placement in ("mean", "first"):
        got = run(M, verts, tris, cell, lo, hi, placement)
        assert_equal(got, S.expected("sphere", cell, given, placement), (cell, given, placement))
    print(f"sphere cell {cell}, bounds {'given' if given else 'defaulted'}: V {len(verts)} -> {len(got[0])}, T {len(tris)} -> {len(got[1])}")


# ---------------------------------------------------------------- 3. past the first trip of every kernel
@pytest.mark.parametrize("cell", [1.2, 2.5])
def test_sheet_past_one_trip(M, cell):
    """547 600 vertices and 1 092 242 triangles: the kernels over vertices and over triangles take several trips of their
    2048 x 256 grids, the ordered ranks several tiles per workgroup.  cell 1.2: the survivors, the new vertices (mean_kernel)
    and the mask's words (word_count / word_prefix) are past one trip as well; cell 2.5 is a real reduction, where those last
    three stay inside one trip (tests/test_mesh_simplify_cpu.py asserts the sizes).  scan_kernel is one workgroup by design:
    it scans at most 2048 workgroup totals per column."""
    verts, tris = S.sheet()
    lo, hi = S.SHEET_BOUNDS
    got = run(M, verts, tris, cell, lo, hi, "mean")
    print(f"sheet cell {cell}: V {len(verts)} -> {len(got[0])}, T {len(tris)} -> {len(got[1])}")
    assert_equal(got, S.expected("sheet", cell, True), cell)
    first = M.simplify_mesh(dev(verts), dev(tris), cell, lo=lo, hi=hi, placement="first")
    assert torch.equal(first[0], dev(verts)[got[3]]) and torch.equal(first[1], got[1])


# ---------------------------------------------------------------- 4. contention
def test_fan_contention_three_runs(M):
    """50 000 triangles in 8 cells: at most 112 key classes, hundreds of triangles racing for each slot's minimum, thousands of
    vertices adding into each of 8 sums."""
    verts, tris = S.fan()
    lo, hi = S.FAN_BOUNDS
    want = S.expected("fan", 1.0, True)
    runs = [run(M, verts, tris, 1.0, lo, hi) for _ in range(3)]
    for r in runs:
        assert_equal(r, want, "fan")
        assert same(r, runs[0])
    assert len(runs[0][0]) == 8 and 0 < len(runs[0][1]) <= 112


# ---------------------------------------------------------------- 5. probing
@pytest.mark.parametrize("cell", S.SPHERE_CELLS)
def test_smallest_legal_table(M, cell):
    """_slots = the next power of two above T: the table is more than half full of distinct keys at small cells, probe
    chains are long and wrap around its end.  One slot fewer than legal is refused."""
    verts, tris = S.sphere()
    T = len(tris)
    slots = 1 << T.bit_length()
    assert slots // 2 <= T < slots
    lo, hi = S.SPHERE_BOUNDS
    small = run(M, verts, tris, cell, lo, hi, _slots=slots)
    assert_equal(small, S.expected("sphere", cell, True), (cell, slots))
    assert same(small, run(M, verts, tris, cell, lo, hi))
    for bad in (slots // 2, slots + 1):
        with pytest.raises(RuntimeError, match="slots"):
            M.simplify_mesh(dev(verts), dev(tris), cell, lo=lo, hi=hi, _slots=bad)


def test_full_table_of_distinct_keys(M):
    """The sheet at a cell below the vertex spacing keeps nearly every triangle a key of its own: with _slots at the legal
    minimum (2^21 for 1 092 242 triangles) the table is half full, and chains cross the end of the table."""
    verts, tris = S.sheet()
    lo, hi = S.SHEET_BOUNDS
    got = run(M, verts, tris, 1.2, lo, hi, _slots=1 << 21)
    assert_equal(got, S.expected("sheet", 1.2, True), "sheet, 2^21 slots")


# ---------------------------------------------------------------- 6. error paths
@pytest.mark.parametrize("kind", ["nan", "inf", "beyond_hi", "below_lo", "index_V", "index_negative"])
def test_one_bad_element_raises(M, kind):
    """Exactly one bad element, past the first trip (vertex and triangle 530 000 of the sheet): RuntimeError.  Outputs are not
    inspected; the next good call is."""
    verts, tris = (a.copy() for a in S.sheet())
    lo, hi = S.SHEET_BOUNDS
    cell, at = 2.5, 530_000
    assert at > 2048 * 256
    if kind == "nan":
        verts[at, 1] = np.nan
    elif kind == "inf":
        verts[at, 0] = np.inf
    elif kind == "beyond_hi":
        verts[at, 2] = hi[2] + cell
    elif kind == "below_lo":
        verts[at, 0] = -1e-3
    elif kind == "index_V":
        tris[at, 1] = len(verts)
    else:
        tris[at, 2] = -1
    with pytest.raises(RuntimeError, match="outside"):
        M.simplify_mesh(dev(verts), dev(tris), cell, lo=lo, hi=hi)
    if kind in ("nan", "inf"):                        # defaulted bounds are not finite then: refused as well
        with pytest.raises(RuntimeError, match="not finite"):
            M.simplify_mesh(dev(verts), dev(tris), cell)
    v, t = S.hand_meshes()["speck"][:2]
    assert_equal(run(M, v, t, 1.0, (0, 0, 0), (4, 4, 4)), S.simplify(v, t, 1.0, (0, 0, 0), (4, 4, 4), attrs=(S.attribute(len(v)),)))


# ---------------------------------------------------------------- 7. wiring
def mesh_models():
    from test_gpu_mesh_components import mesh_models as models          # the suite's small test NeRF (raw sigma crosses 10)
    return models()


@pytest.mark.parametrize("simplify", [2, 4.5])
def test_extract_mesh_simplify(M, simplify):
    nerf, embs = mesh_models()
    Ng = 32
    kw = dict(N_grid=Ng, sigma_threshold=10)
    with torch.no_grad():
        verts, tris = M.extract_mesh(nerf, embs[0], **kw)
        none = M.extract_mesh(nerf, embs[0], simplify=None, **kw)
        assert torch.equal(verts, none[0]) and torch.equal(tris, none[1])
        sigma = M.query_sigma(M.mesh.lattice(Ng, verts.device), nerf, embs[0]).view(Ng, Ng, Ng)
        raw, rt = M.marching_cubes(sigma, 10, clamp_zero=True)
        got = M.extract_mesh(nerf, embs[0], simplify=simplify, **kw)
        sv, st = M.simplify_mesh(raw, rt, simplify, lo=(0, 0, 0), hi=(Ng - 1,) * 3, placement="mean")
        assert 0 < len(st) < len(rt) and 0 < len(sv) < len(raw)
        assert torch.equal(got[0], sv[:, [1, 0, 2]] / Ng * 3.0 - 1.5) and torch.equal(got[1], st[:, [0, 2, 1]])
        want = S.simplify(raw.cpu().numpy(), rt.cpu().numpy(), simplify, (0, 0, 0), (Ng - 1,) * 3)
        assert torch.equal(sv.cpu(), torch.from_numpy(want[0])) and torch.equal(st.cpu(), torch.from_numpy(want[1]))
        # after the component filter: the filter's mesh is what gets simplified
        fv, ft = M.filter_components(raw, rt, keep_largest=1)
        kv, kt = M.simplify_mesh(fv, ft, simplify, lo=(0, 0, 0), hi=(Ng - 1,) * 3)
        both = M.extract_mesh(nerf, embs[0], simplify=simplify, keep_largest=1, **kw)
        assert torch.equal(both[0], kv[:, [1, 0, 2]] / Ng * 3.0 - 1.5) and torch.equal(both[1], kt[:, [0, 2, 1]])
    print(f"extract_mesh N_grid {Ng} simplify {simplify}: V {len(raw)} -> {len(sv)}, T {len(rt)} -> {len(st)}")


def test_extract_colored_mesh_simplify(M):
    from test_gpu_mesh_components import IND_SCALAR
    nerf, embs = mesh_models()
    Ng, s = 32, 3
    kw = dict(N_grid=Ng, sigma_threshold=10, ind=IND_SCALAR)
    with torch.no_grad():
        full = M.extract_colored_mesh(nerf, embs, **kw)
        none = M.extract_colored_mesh(nerf, embs, simplify=None, **kw)
        for x, y in zip(full, none):
            assert torch.equal(x, y)
        verts, tris, normals, colors = M.extract_colored_mesh(nerf, embs, simplify=s, **kw)
        sigma = M.query_sigma(M.mesh.lattice(Ng, verts.device), nerf, embs[0], ind=IND_SCALAR).view(Ng, Ng, Ng)
        raw, rt = M.marching_cubes(sigma, 10, clamp_zero=True)
        rn = M.vertex_normals(sigma, raw, clamp_zero=True)[:, [1, 0, 2]].contiguous()
        sv, st, sn, first, cluster = M.simplify_mesh(raw, rt, s, lo=(0, 0, 0), hi=(Ng - 1,) * 3, attrs=(rn,), return_map=True)
        assert torch.equal(full[2], rn)
    assert 0 < len(sv) < len(raw) and 0 < len(st) < len(rt)
    assert torch.equal(verts, sv[:, [1, 0, 2]] / Ng * 3.0 - 1.5) and torch.equal(tris, st[:, [0, 2, 1]])
    assert torch.equal(normals, sn) and torch.equal(normals, rn[first])                          # the rows of first, not re-normalised
    assert tuple(colors.shape) == (len(sv), 3) and colors.dtype == torch.float32 and bool(torch.isfinite(colors).all())
    print(f"extract_colored_mesh simplify {s}: V {len(raw)} -> {len(sv)}, T {len(rt)} -> {len(st)}, {len(colors)} colours queried")


# ---------------------------------------------------------------- 8. empty cases
def test_empty_cases(M):
    none_v, none_t = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64)
    verts = np.array([[0.5, 0.5, 0.5], [0.6, 0.7, 0.8], [0.9, 0.1, 0.2], [2.5, 0.5, 0.5]], np.float32)
    cases = {"no vertices": (none_v, none_t), "no triangles": (verts, none_t),
             "all degenerate": (verts, np.array([[0, 1, 2], [2, 1, 0], [0, 1, 3], [3, 3, 3]], np.int64))}
    for what, (v, t) in cases.items():
        for placement in ("mean", "first"):
            for lo, hi in (((0, 0, 0), (3, 3, 3)), (None, None)):
                got = run(M, v, t, 1.0, lo, hi, placement)
                assert_equal(got, S.simplify(v, t, 1.0, lo, hi, placement, attrs=(S.attribute(len(v)),)), (what, placement))
                assert [tuple(x.shape) for x in got] == [(0, 3), (0, 3), (0, 3), (0,), (len(v),)], what
                assert bool((got[4] == -1).all())
