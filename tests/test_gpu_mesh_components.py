"""Mesh clean-up on the MI355X: mesh_components (mf_mesh_label, mf_mesh_table_*) and filter_components (mf_mesh_filter_*,
mf_gather_rows) against the numpy oracle of their contract (tests/mesh_components_oracle.py), exactly (torch.equal): the
marching-cubes meshes of the fixtures, white-noise volumes (up to a thousand small components, many ties in triangle count),
index meshes built to be hard on a concurrent union-find (long paths in every index order, one hub, interleaved index
ranges, degenerate and repeated triangles, unused vertices, empty inputs), an index out of range, determinism, idempotence,
the two keywords of extract_mesh / extract_colored_mesh, and index meshes past one trip of the table's and the filter's
grid-stride loops (sizes from the launch constants of csrc/mf_mesh_components.hip), with patterns that drive the wave-level
count through every branch it has for a pair carried from an earlier trip."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import mc_oracle as O
import mesh_components_oracle as CC

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "m_mesh.npz"))
FIXTURES = ("ball", "torus", "noise", "noncubic", "boundary", "nerf")
NOISE_SHAPES = ((9, 11, 13), (40, 37, 64))
COLOUR_TOL = 1e-4                # tests/test_gpu_mesh_color.py: TOL, the bar between two queries of the same points
IND_SCALAR = float(np.float32(17 * 2 / 300 - 1.0))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M():
    import moco_flow_amd
    return moco_flow_amd


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def assert_components(M, tris, V, want=None, what=""):
    """mesh_components on the device equals the oracle's four arrays; returns the oracle's."""
    want = CC.components(tris, V) if want is None else want
    got = M.mesh_components(dev(tris), V)
    torch.cuda.synchronize()
    for name, g, w in zip(("labels", "ids", "tri_counts", "vert_counts"), got, want):
        assert g.dtype == torch.int64 and g.is_cuda and g.shape == w.shape, (what, name, g.shape, w.shape)
        assert torch.equal(g.cpu(), torch.from_numpy(w)), (what, name)
    return want


def assert_filter(M, verts, tris, attr, comps, what="", **rule):
    """filter_components on the device equals the oracle's vertices, triangles and attribute; returns the device's."""
    want = CC.filter_components(verts, tris, attrs=(attr,), comps=comps, **rule)
    got = M.filter_components(dev(verts), dev(tris), attrs=(dev(attr),), **rule)
    torch.cuda.synchronize()
    assert len(got) == 3
    for name, g, w in zip(("verts", "tris", "attr"), got, want):
        assert g.is_cuda and g.dtype == torch.from_numpy(w).dtype and tuple(g.shape) == w.shape, (what, rule, name, g.shape, w.shape)
        assert torch.equal(g.cpu(), torch.from_numpy(w)), (what, rule, name)
    return got


# ---------------------------------------------------------------- marching-cubes meshes
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_meshes_equal_the_oracle(M, name):
    vol, iso, clamp = GOLD[name + "_vol"], float(GOLD[name + "_iso"]), bool(GOLD[name + "_clamp"])
    verts, tris = M.marching_cubes(dev(vol), iso, clamp_zero=clamp)
    lab, ids, tc, vc = assert_components(M, tris.cpu().numpy(), len(verts), what=name)
    print(f"{name}: V {len(verts)} T {len(tris)}, {len(ids)} components, largest {sorted(tc.tolist())[::-1][:4]}")
    assert len(ids) == {"noncubic": 2, "nerf": 480}.get(name, 1)


@functools.lru_cache(maxsize=None)
def noise_mesh(shape):
    """(verts, tris, a float attribute, the oracle's components) of a white-noise volume at iso 0, computed once."""
    import moco_flow_amd as M
    vol = np.random.default_rng(sum(shape)).standard_normal(shape).astype(np.float32)
    verts, tris = M.marching_cubes(dev(vol), 0.0)
    verts, tris = verts.cpu().numpy(), tris.cpu().numpy()
    attr = np.random.default_rng(1).standard_normal((len(verts), 2)).astype(np.float32)
    return verts, tris, attr, CC.components(tris, len(verts))


@pytest.mark.parametrize("shape", NOISE_SHAPES)
def test_white_noise_table_and_filters(M, shape):
    verts, tris, attr, comps = noise_mesh(shape)
    assert_components(M, tris, len(verts), want=comps, what=shape)
    tc = comps[2]
    _, reps = np.unique(tc, return_counts=True)
    print(f"noise {shape}: V {len(verts)} T {len(tris)}, {len(tc)} components, largest {int(tc.max())}, "
          f"{int((reps > 1).sum())} triangle counts shared by several components")
    assert len(tc) >= (10, 500)[NOISE_SHAPES.index(shape)] and (reps > 1).any()     # the input is what the case is for
    for k in (1, 2, 5):
        assert_filter(M, verts, tris, attr, comps, what=shape, keep_largest=k)
    for m in (1, 2, 8):
        assert_filter(M, verts, tris, attr, comps, what=shape, min_triangles=m)
    assert_filter(M, verts, tris, attr, comps, what=shape, keep_largest=5, min_triangles=8)
    v, t, a = assert_filter(M, verts, tris, attr, comps, what=shape, min_triangles=int(tc.max()) + 1)
    assert tuple(v.shape) == (0, 3) and tuple(t.shape) == (0, 3) and tuple(a.shape) == (0, 2) and t.dtype == torch.int64


# ---------------------------------------------------------------- index meshes, no volume
STRIP = 200_000                  # more triangles than the labelling's grid has threads (512 workgroups of 256)
FAN = 100_000


def strip(n, first=0):
    i = np.arange(n, dtype=np.int64) + first
    return np.stack([i, i + 1, i + 2], 1)


@functools.lru_cache(maxsize=None)
def index_mesh(name):
    """(tris, V) of one adversarial mesh."""
    rng = np.random.default_rng(7)
    if name.startswith("strip_"):                       # a path graph: deep trees; rows shuffled
        tris, V = strip(STRIP)[rng.permutation(STRIP)], STRIP + 2
        if name == "strip_descending":
            tris = V - 1 - tris
        elif name == "strip_permuted":
            tris = rng.permutation(V)[tris]
        else:
            assert name == "strip_ascending"
        return tris, V
    if name == "fan":                                   # every union and every count on one address: the hub, in column 0
        hub, rim = 31_415, np.delete(np.arange(FAN + 2, dtype=np.int64), 31_415)
        return np.stack([np.full(FAN, hub, np.int64), rim[:-1], rim[1:]], 1)[rng.permutation(FAN)], FAN + 2
    if name == "interleaved":                           # two strips, one on the even indices, one on the odd
        n = 30_000
        return np.concatenate([2 * strip(n), 2 * strip(n) + 1])[rng.permutation(2 * n)], 2 * n + 4
    if name == "duplicated":
        return np.concatenate([strip(300), strip(300), strip(300)[::-1], strip(50, 400), strip(50, 400)]), 460
    if name == "degenerate":                            # (i, i, j) and (i, i, i): legal, they join what they name
        i = np.arange(0, 600, 3, dtype=np.int64)
        return np.concatenate([np.stack([i, i, i + 4], 1), np.stack([i + 1, i + 1, i + 1], 1), np.stack([i + 5, i + 2, i + 2], 1)]), 606
    if name == "unused_vertices":                       # vertices in no triangle: components without triangles
        return 3 * strip(500) + 7, 3 * 502 + 40
    if name == "single":
        return np.array([[4, 2, 9]], np.int64), 11
    if name == "no_triangles":
        return np.zeros((0, 3), np.int64), 1000
    assert name == "no_vertices"
    return np.zeros((0, 3), np.int64), 0


INDEX_MESHES = ("strip_ascending", "strip_descending", "strip_permuted", "fan", "interleaved", "duplicated", "degenerate",
                "unused_vertices", "single", "no_triangles", "no_vertices")


@functools.lru_cache(maxsize=None)
def index_components(name):
    return CC.components(*index_mesh(name))


@pytest.mark.parametrize("name", INDEX_MESHES)
def test_index_meshes_equal_the_oracle(M, name):
    tris, V = index_mesh(name)
    comps = index_components(name)
    assert_components(M, tris, V, want=comps, what=name)
    ids, tc = comps[1], comps[2]
    want_c = {"interleaved": 2, "duplicated": 2 + 460 - 302 - 52, "unused_vertices": 1 + (3 * 502 + 40) - 502, "single": 9, "no_triangles": 1000,
              "no_vertices": 0}.get(name)
    if name.startswith("strip_") or name == "fan":
        want_c = 1
    if want_c is not None:
        assert len(ids) == want_c, (name, len(ids))
    # the filter on the same mesh: vertices are their own old indices, so the kept rows say which were kept
    verts = np.arange(V, dtype=np.int64)[:, None].repeat(3, 1).astype(np.float32)
    attr = np.arange(V, dtype=np.int32)
    assert_filter(M, verts, tris, attr, comps, what=name, keep_largest=1)
    assert_filter(M, verts, tris, attr, comps, what=name, min_triangles=1)
    assert_filter(M, verts, tris, attr, comps, what=name, keep_largest=3, min_triangles=2)


# ---------------------------------------------------------------- past one trip of the grid-stride loops
# Every kernel of the table and of the filter is a grid-stride loop of at most MAX_BLOCKS workgroups of THREADS threads: it
# takes a second trip only past TRIP elements.  A 512^3 extraction has millions of triangles; no mesh above reaches TRIP.
_SRC = open(os.path.join(HERE, "..", "moco_flow_amd", "csrc", "mf_mesh_components.hip")).read()
_const = lambda name: int(re.search(r"\bconstexpr int %s = (\d+);" % name, _SRC).group(1))
THREADS, MAX_BLOCKS = _const("kThreads"), _const("kMaxBlocks")
TRIP = THREADS * MAX_BLOCKS
RAGGED = 70_001                                         # the elements of the last trip: some workgroups take it, the last wave partly
assert STRIP + 2 < TRIP and 40 * 37 * 64 * 5 < TRIP and 0 < RAGGED < TRIP and RAGGED % 64 and THREADS % 64 == 0
SHORT = TRIP // 4 + 19_000                              # strips of 4 triangles on 6 vertices


@functools.lru_cache(maxsize=None)
def big_mesh(name):
    """(tris, V) of one mesh with more than TRIP triangles, vertices or components."""
    rng = np.random.default_rng(11)
    if name == "strip":                                 # one component: T, V > TRIP; vertices permuted, rows shuffled
        T = TRIP + RAGGED
        return rng.permutation(T + 2)[strip(T)[rng.permutation(T)]], T + 2
    if name == "disjoint":                              # C = T > TRIP components of one triangle each, on scattered vertices
        T = TRIP + 6_001
        return rng.permutation(3 * T).reshape(T, 3), 3 * T
    if name == "isolated":                              # C = V > TRIP components without a triangle
        return np.zeros((0, 3), np.int64), TRIP + RAGGED
    assert name == "short_strips"                       # C = SHORT; kept whole: Vk, Tk > TRIP
    tris = (strip(4)[None] + 6 * np.arange(SHORT, dtype=np.int64)[:, None, None]).reshape(-1, 3)
    return tris[rng.permutation(len(tris))], 6 * SHORT


@functools.lru_cache(maxsize=None)
def big_components(name):
    return CC.components(*big_mesh(name))


def _index_verts(V):
    """Vertices that are their own old indices, and an int32 attribute: the kept rows say which were kept."""
    return np.arange(V, dtype=np.int64)[:, None].repeat(3, 1).astype(np.float32), np.arange(V, dtype=np.int32)


@pytest.mark.parametrize("name", ["strip", "disjoint", "isolated", "short_strips"])
def test_table_and_filter_past_one_trip(M, name):
    """table_tris / table_verts / table_gather and the root compaction, keep_roots / keep_verts / keep_tris, remap / reindex
    and the row gathers with more than TRIP triangles, vertices, components, kept vertices and kept triangles."""
    tris, V = big_mesh(name)
    comps = big_components(name)
    T, C = len(tris), len(comps[1])
    assert_components(M, tris, V, want=comps, what=name)
    verts, attr = _index_verts(V)
    if name == "strip":
        assert T > TRIP and V > TRIP and C == 1
        v, t, _ = assert_filter(M, verts, tris, attr, comps, what=name, keep_largest=1)
        assert len(v) == V and len(t) == T
    if name == "disjoint":
        assert C == T > TRIP and V > 3 * TRIP
        assert_filter(M, verts, tris, attr, comps, what=name, keep_largest=3)                   # every rank is a tie: by label
        v, t, _ = assert_filter(M, verts, tris, attr, comps, what=name, min_triangles=1)
        assert len(v) == V and len(t) == T
    if name == "isolated":
        assert C == V > TRIP and T == 0
        v, t, _ = assert_filter(M, verts, tris, attr, comps, what=name, keep_largest=2)
        assert len(v) == 2 and len(t) == 0
        v, t, _ = assert_filter(M, verts, tris, attr, comps, what=name, min_triangles=1)
        assert len(v) == 0 and len(t) == 0
    if name == "short_strips":
        assert C == SHORT and T == 4 * SHORT > TRIP and (comps[2] == 4).all() and (comps[3] == 6).all()
        v, t, _ = assert_filter(M, verts, tris, attr, comps, what=name, min_triangles=1)        # all of it: Vk, Tk > TRIP
        assert len(v) == V > TRIP and len(t) == T
        v, t, _ = assert_filter(M, verts, tris, attr, comps, what=name, keep_largest=5, min_triangles=5)
        assert len(v) == 0 and len(t) == 0


# WaveCount (csrc/mf_mesh_components.hip) carries a wave's (key, count) pair across the trips; on the first trip the pair
# starts empty, so what it does with a pair held over is reached only past TRIP elements.  A pattern spells the mesh
# (CC.pattern_mesh): rows and vertices are in pattern order, nothing is shuffled -- the order is the input.  Lane l of a wave
# reads the elements = l (mod 64): TRIP and every workgroup's base are multiples of 64.
def _pattern(name):
    n = RAGGED + (TRIP if name == "one_three_trips" else 0)
    lane = np.arange(n) % 64
    later = {"one": np.zeros(n), "one_three_trips": np.zeros(n),             # the held key again: carried, flushed once
             "switch": np.ones(n),                                          # a new majority flushes a non-empty pair
             "minority_low": lane >= 20,                                    # 20 A then 44 B: A is carried, then B takes the pair
             "minority_high": lane < 44,                                    # 44 B take the pair, then A, no longer held: its leader adds
             "half": lane >= 32,                                            # 32 A carried, 32 B: no majority, their leader adds
             "distinct": 1 + lane}[name]                                    # 64 keys of one lane each
    return np.concatenate([np.zeros(TRIP, np.int64), later.astype(np.int64)])


PATTERNS = {"one": (1, ("carry_add",)), "one_three_trips": (1, ("carry_add",)), "switch": (2, ("take_flush",)),
            "minority_low": (2, ("carry_add", "take_flush")), "minority_high": (2, ("take_flush", "leader_add_holding")),
            "half": (2, ("carry_add", "leader_add_holding")), "distinct": (65, ("leader_add_holding",))}


@pytest.mark.parametrize("name", list(PATTERNS))
def test_counts_carried_across_trips(M, name):
    """tri_counts and vert_counts where a wave meets, on a later trip, the key it holds, a new majority, the held key as a
    minority before or after the new majority, an even split and 64 distinct keys.  CC.wave_count_replay proves on the
    oracle's labels that the mesh drives both counting kernels through the branches it was built for."""
    n_comps, branches = PATTERNS[name]
    tris, V = CC.pattern_mesh(_pattern(name))
    comps = lab, ids, tc, vc = CC.components(tris, V)
    assert len(ids) == n_comps and min(len(tris), V) > TRIP * (2 if name == "one_three_trips" else 1)
    for what, keys, counts in (("triangles", lab[tris[:, 0]], tc), ("vertices", lab, vc)):
        adds, later = CC.wave_count_replay(keys, THREADS, MAX_BLOCKS)
        assert [adds.get(int(r), 0) for r in ids] == counts.tolist(), (name, what)
        for b in branches:
            assert later[b] > 0, (name, what, later)
        print(f"{name} {what}: {len(keys)} elements, on later trips {later}")
    assert_components(M, tris, V, want=comps, what=name)
    verts, attr = _index_verts(V)
    assert_filter(M, verts, tris, attr, comps, what=name, keep_largest=1)
    assert_filter(M, verts, tris, attr, comps, what=name, keep_largest=2, min_triangles=3)


def test_index_out_of_range_raises_and_leaves_nothing_behind(M):
    tris, V = index_mesh("duplicated")
    good = dev(tris)
    verts = torch.zeros(V, 3, device="cuda")
    for value in (V, -1):
        for row, col in ((0, 0), (len(tris) // 2, 1), (len(tris) - 1, 2)):
            bad = good.clone()
            bad[row, col] = value
            with pytest.raises(RuntimeError, match="outside"):
                M.mesh_components(bad, V)
            with pytest.raises(RuntimeError, match="outside"):
                M.filter_components(verts, bad, keep_largest=1)
    comps = index_components("duplicated")
    assert_components(M, tris, V, want=comps)
    assert_filter(M, np.zeros((V, 3), np.float32), tris, np.arange(V), comps, keep_largest=1)


def test_repeat_runs_bit_identical(M):
    strip_tris, strip_V = index_mesh("strip_permuted")
    verts, tris, attr, _ = noise_mesh(NOISE_SHAPES[1])
    for what, t, V, v, a in (("strip", dev(strip_tris), strip_V, torch.zeros(strip_V, 1, device="cuda"), torch.arange(strip_V, device="cuda")),
                             ("noise", dev(tris), len(verts), dev(verts), dev(attr))):
        first = None
        for _ in range(5):
            out = M.mesh_components(t, V) + M.filter_components(v, t, keep_largest=3, attrs=(a,)) \
                + M.filter_components(v, t, min_triangles=2, attrs=(a,))
            if first is None:
                first = out
            for x, y in zip(first, out):
                assert torch.equal(x, y), what


def test_filter_is_idempotent(M):
    verts, tris, attr, comps = noise_mesh(NOISE_SHAPES[1])
    tc = comps[2]
    v, t, a = dev(verts), dev(tris), dev(attr)
    for rule, kept in ((dict(keep_largest=5), 5), (dict(min_triangles=8), int((tc >= 8).sum())),
                       (dict(keep_largest=40, min_triangles=3), int((np.sort(tc)[::-1][:40] >= 3).sum()))):
        v1, t1, a1 = M.filter_components(v, t, attrs=(a,), **rule)
        v2, t2, a2 = M.filter_components(v1, t1, attrs=(a1,), **rule)
        assert 0 < len(t1) < len(t) and 0 < len(v1) < len(v)
        assert torch.equal(v1, v2) and torch.equal(t1, t2) and torch.equal(a1, a2)
        labels, ids, tcounts, vcounts = M.mesh_components(t1, len(v1))
        assert len(ids) == kept and int(tcounts.sum()) == len(t1) and int(vcounts.sum()) == len(v1)
        assert int(tcounts.min()) >= rule.get("min_triangles", 1)


# ---------------------------------------------------------------- extract_mesh / extract_colored_mesh
@functools.lru_cache(maxsize=None)
def mesh_models():
    """The NeRF of tests/test_gpu_mesh.py (raw sigma crosses 10)."""
    import moco_flow_amd as M
    from moco_flow_amd import synth
    sd = synth.nerf_state(0, extra_feat_type="ind", extra_feat_dim=5, regime="dense")
    sd["sigma.weight"] = sd["sigma.weight"] * np.float32(3.0)
    nerf = M.NeRF(8, 256, 63, [4], "ind", 5)
    nerf.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return nerf.cuda(), [M.Embedding(3, 10), M.Embedding(1, 2), None]


def test_extract_mesh_keywords(M):
    nerf, embs = mesh_models()
    Ng = 32
    with torch.no_grad():
        verts, tris = M.extract_mesh(nerf, embs[0], N_grid=Ng, sigma_threshold=10)
        # today's path, spelled out: sigma lattice, marching cubes, the reference's post-processing
        sigma = M.query_sigma(M.mesh.lattice(Ng, verts.device), nerf, embs[0]).view(Ng, Ng, Ng)
        raw, rt = M.marching_cubes(sigma, 10, clamp_zero=True)
        assert torch.equal(verts, raw[:, [1, 0, 2]] / Ng * 3.0 - 1.5) and torch.equal(tris, rt[:, [0, 2, 1]])
        explicit = M.extract_mesh(nerf, embs[0], N_grid=Ng, sigma_threshold=10, keep_largest=None, min_triangles=None)
        assert torch.equal(verts, explicit[0]) and torch.equal(tris, explicit[1])
        _, ids, tc, _ = M.mesh_components(tris, len(verts))
        assert len(ids) > 1
        for rule in (dict(keep_largest=1), dict(min_triangles=20), dict(keep_largest=3, min_triangles=2)):
            got = M.extract_mesh(nerf, embs[0], N_grid=Ng, sigma_threshold=10, **rule)
            want = M.filter_components(verts, tris, **rule)
            assert 0 < len(got[1]) < len(tris)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), rule
        v1, t1 = M.extract_mesh(nerf, embs[0], N_grid=Ng, sigma_threshold=10, keep_largest=1)
        assert len(t1) == int(tc.max()) and len(M.mesh_components(t1, len(v1))[1]) == 1
        print(f"extract_mesh N_grid {Ng}: V {len(verts)} T {len(tris)} in {len(ids)} components; keep_largest=1: V {len(v1)} T {len(t1)}")
        empty = M.extract_mesh(nerf, embs[0], N_grid=Ng, sigma_threshold=10, min_triangles=len(tris) + 1)
        assert tuple(empty[0].shape) == (0, 3) and tuple(empty[1].shape) == (0, 3)


def test_extract_colored_mesh_keywords(M):
    nerf, embs = mesh_models()
    kw = dict(N_grid=32, sigma_threshold=10, ind=IND_SCALAR)
    with torch.no_grad():
        verts, tris, normals, colors = M.extract_colored_mesh(nerf, embs, **kw)
        explicit = M.extract_colored_mesh(nerf, embs, keep_largest=None, min_triangles=None, **kw)
        for x, y in zip((verts, tris, normals, colors), explicit):
            assert torch.equal(x, y)
        v1, t1, n1, c1 = M.extract_colored_mesh(nerf, embs, keep_largest=1, **kw)
        wv, wt, wn, wc = M.filter_components(verts, tris, keep_largest=1, attrs=(normals, colors))
        empty = M.extract_colored_mesh(nerf, embs, min_triangles=len(tris) + 1, **kw)
    assert 0 < len(v1) < len(verts) and 0 < len(t1) < len(tris)
    assert torch.equal(v1, wv) and torch.equal(t1, wt) and torch.equal(n1, wn)
    assert c1.shape == wc.shape and c1.dtype == torch.float32
    err = float((c1.double() - wc.double()).abs().max() / wc.double().abs().max())
    print(f"extract_colored_mesh keep_largest=1: V {len(v1)} of {len(verts)}, T {len(t1)} of {len(tris)}; colours of the kept "
          f"vertices against the unfiltered call's: max-rel {err:.2e}, bitwise equal {torch.equal(c1, wc)}")
    assert err <= COLOUR_TOL
    assert [tuple(x.shape) for x in empty] == [(0, 3)] * 4
