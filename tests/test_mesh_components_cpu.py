"""CPU-side checks (-m "not gpu") of the mesh clean-up: the numpy oracle of its contract (tests/mesh_components_oracle.py)
against scipy.sparse.csgraph on the marching-cubes meshes of the fixtures (tests/golden/m_mesh.npz), with the component
counts those fixtures have; the library's exports, ABI version and ctypes prototypes; host-side validation of mf_mesh_* and
of mesh_components / filter_components, none of which touches a GPU."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

import mc_oracle as O
import mesh_components_oracle as CC

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = np.load(os.path.join(HERE, "golden", "m_mesh.npz"))
# fixture -> (components, their largest triangle counts in rank order)
PINNED = {"ball": (1, None), "torus": (1, None), "noise": (1, None), "boundary": (1, None), "noncubic": (2, [5615, 7]),
          "nerf": (480, [6244, 776, 600, 560])}
NEW_SYMBOLS = ("mf_mesh_label_scratch_bytes", "mf_mesh_label", "mf_mesh_table_scratch_bytes", "mf_mesh_table_count",
               "mf_mesh_table_emit", "mf_mesh_filter_scratch_bytes", "mf_mesh_filter_plan", "mf_mesh_filter_emit",
               "mf_gather_rows")


@functools.lru_cache(maxsize=None)
def fixture_mesh(name):
    return O.marching_cubes(GOLD[name + "_vol"], float(GOLD[name + "_iso"]), bool(GOLD[name + "_clamp"]))


@pytest.mark.parametrize("name", sorted(PINNED))
def test_oracle_equals_scipy_on_the_fixtures(name):
    sparse = pytest.importorskip("scipy.sparse")
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    verts, tris = fixture_mesh(name)
    V = len(verts)
    lab, ids, tri_counts, vert_counts = CC.components(tris, V)
    e = np.concatenate([tris[:, [0, 1]], tris[:, [1, 2]], tris[:, [2, 0]]])
    graph = sparse.coo_matrix((np.ones(len(e), np.int8), (e[:, 0], e[:, 1])), shape=(V, V))
    n, slab = csgraph.connected_components(graph, directed=False)
    # scipy numbers components in its own order: the smallest index of each is the contract's label
    first = np.full(n, V, np.int64)
    np.minimum.at(first, slab, np.arange(V))
    assert np.array_equal(lab, first[slab])
    assert np.array_equal(ids, np.sort(first)) and len(ids) == n
    assert np.array_equal(vert_counts, np.bincount(slab, minlength=n)[slab[ids]])
    assert np.array_equal(tri_counts, np.bincount(slab[tris[:, 0]], minlength=n)[slab[ids]])
    assert tri_counts.sum() == len(tris) and vert_counts.sum() == V
    want_n, want_top = PINNED[name]
    assert n == want_n
    ranked = tri_counts[CC.ranking(ids, tri_counts)]
    assert np.all(ranked[:-1] >= ranked[1:])
    if want_top is not None:
        assert ranked[:len(want_top)].tolist() == want_top
    if n > 1:
        assert ranked[0] > ranked[1]                                      # no tie at the top rank
    if name == "nerf":
        assert (V, len(tris)) == (10003, 17107)


def test_oracle_on_hand_made_meshes():
    # two components, a vertex in no triangle, a degenerate and a repeated triangle
    tris = np.array([[5, 4, 6], [1, 1, 3], [3, 3, 3], [4, 5, 6], [4, 5, 6]], np.int64)
    lab, ids, tc, vc = CC.components(tris, 8)
    assert lab.tolist() == [0, 1, 2, 1, 4, 4, 4, 7]
    assert ids.tolist() == [0, 1, 2, 4, 7] and tc.tolist() == [0, 2, 0, 3, 0] and vc.tolist() == [1, 2, 1, 3, 1]
    assert CC.ranking(ids, tc).tolist() == [3, 1, 0, 2, 4]                  # ties by label
    verts = np.arange(24, dtype=np.float32).reshape(8, 3)
    attr = np.arange(8)
    v, t, a = CC.filter_components(verts, tris, keep_largest=2, attrs=(attr,))
    assert a.tolist() == [1, 3, 4, 5, 6] and np.array_equal(v, verts[a])
    assert t.tolist() == [[3, 2, 4], [0, 0, 1], [1, 1, 1], [2, 3, 4], [2, 3, 4]]
    v, t = CC.filter_components(verts, tris, keep_largest=2, min_triangles=3)
    assert t.tolist() == [[1, 0, 2], [0, 1, 2], [0, 1, 2]] and np.array_equal(v, verts[4:7])
    v, t = CC.filter_components(verts, tris, min_triangles=4)
    assert v.shape == (0, 3) and t.shape == (0, 3) and t.dtype == np.int64
    lab, ids, tc, vc = CC.components(np.zeros((0, 3), np.int64), 0)
    assert lab.shape == ids.shape == tc.shape == vc.shape == (0,)


def _replay(tris, V, comps, threads, max_blocks):
    """CC.wave_count_replay over the triangles and the vertices: its sums equal the oracle's table; the branch counts of both."""
    lab, ids, tc, vc = comps
    out = []
    for keys, counts in ((lab[tris[:, 0]], tc), (lab, vc)):
        adds, later = CC.wave_count_replay(keys, threads, max_blocks)
        assert [adds.get(int(r), 0) for r in ids] == counts.tolist() and sum(adds.values()) == len(keys)
        out.append(later)
    return out


def test_small_meshes_never_carry_a_count_across_trips():
    """The gap that tests/test_gpu_mesh_components.py closes past TRIP elements, written down: under the kernels' launch
    constants every mesh of the older tests is counted in one trip, so WaveCount never meets a pair held over."""
    import test_gpu_mesh_components as G
    assert (G.THREADS, G.MAX_BLOCKS, G.TRIP) == (256, 2048, 524288)                    # read from the source; a change shows here
    meshes = [(name, fixture_mesh(name)[1], len(fixture_mesh(name)[0])) for name in sorted(PINNED)]
    meshes += [(name,) + G.index_mesh(name) for name in G.INDEX_MESHES]
    for name, tris, V in meshes:
        assert max(len(tris), V) < G.TRIP, name
        for later in _replay(tris, V, CC.components(tris, V), G.THREADS, G.MAX_BLOCKS):
            assert not any(later.values()), (name, later)


def test_replay_on_patterns_under_a_small_grid():
    """CC.pattern_mesh and CC.wave_count_replay under a grid of 3 workgroups of 128 threads: every branch of a later trip is
    taken by the pattern built for it, and the replayed sums are the oracle's counts."""
    threads, blocks = 128, 3
    trip, n = threads * blocks, 5 * 64 + 37
    lane = np.arange(n) % 64
    cases = {"one": (np.zeros(n), ("carry_add",)), "switch": (np.ones(n), ("take_flush",)),
             "minority_low": (lane >= 20, ("carry_add", "take_flush")), "minority_high": (lane < 44, ("take_flush", "leader_add_holding")),
             "half": (lane >= 32, ("carry_add", "leader_add_holding")), "distinct": (1 + lane, ("leader_add_holding",))}
    seen = set()
    for name, (later_part, branches) in cases.items():
        pattern = np.concatenate([np.zeros(trip, np.int64), np.asarray(later_part, np.int64)])
        tris, V = CC.pattern_mesh(pattern)
        comps = CC.components(tris, V)
        assert np.array_equal(comps[0], comps[1][pattern]) and len(tris) == V - 2 * len(comps[1])   # the labels spell the pattern
        assert np.array_equal(tris[:, 0], np.sort(tris[:, 0])) and len(np.unique(tris[:, 0])) == len(tris)
        for later in _replay(tris, V, comps, threads, blocks):
            for b in branches:
                assert later[b] > 0, (name, later)
            seen |= {b for b in later if later[b]}
    assert seen == set(CC.BRANCHES) - {"take_empty"}                    # a wave that takes a later trip filled its pair on the first
    adds, later = CC.wave_count_replay([7] * 40 + [5] * 24 + [5] * 10, 64, 1)         # one wave, two trips, by hand
    assert adds == {7: 40, 5: 34} and later == dict(carry_add=0, take_flush=0, take_empty=0, leader_add_holding=1)


def test_library_exports_header_symbols_and_prototypes():
    import moco_flow_amd._lib as L
    header = open(os.path.join(ROOT, "include", "mocoflow_hip.h")).read()
    declared = set(re.findall(r"^int(?:32|64)_t (mf_\w+)\(", header, re.M))
    lib = L.lib()
    assert lib.mf_version() == 16 and L.MF_ABI_VERSION == 16
    assert "#define MF_ABI_VERSION 16" in header
    listed = " ".join(header.split("additive entries since")[1].split("*/")[0].split())
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in L.SYMBOLS, name
        fn = getattr(lib, name)
        assert fn.restype is L.SYMBOLS[name][0] and list(fn.argtypes) == L.SYMBOLS[name][1]
        assert name.replace("_scratch_bytes", "").replace("_emit", "").replace("_plan", "").replace("_count", "") in listed, name
    new_in_header = {n for n in declared if n.startswith(("mf_mesh_", "mf_gather_"))}
    assert new_in_header == set(NEW_SYMBOLS)
    i64, p = C.c_int64, C.c_void_p
    assert L.SYMBOLS["mf_mesh_label"] == (C.c_int32, [p, i64, i64, p, p, p, p])
    assert L.SYMBOLS["mf_mesh_table_count"] == (C.c_int32, [p, i64, i64, p, p, p, p])
    assert L.SYMBOLS["mf_mesh_table_emit"] == (C.c_int32, [i64, i64, p, p, p, p, p])
    assert L.SYMBOLS["mf_mesh_filter_plan"] == (C.c_int32, [p, i64, i64, p, p, p, i64, p, p, p])
    assert L.SYMBOLS["mf_mesh_filter_emit"] == (C.c_int32, [p, i64, i64, i64, i64, p, p, p, p, p])
    assert L.SYMBOLS["mf_gather_rows"] == (C.c_int32, [p, i64, i64, p, i64, p, p])
    for name in ("mf_mesh_label_scratch_bytes", "mf_mesh_table_scratch_bytes", "mf_mesh_filter_scratch_bytes"):
        assert L.SYMBOLS[name] == (i64, [i64, i64])


def test_host_side_validation():
    """Sizes, the 2^31 limit and null arguments are settled on the host, before anything is launched: the fake pointers are
    never touched."""
    import moco_flow_amd._lib as L
    lib = L.lib()
    fake = C.c_void_p(256)
    big = 1 << 31
    assert lib.mf_mesh_label_scratch_bytes(0, 0) == 0
    assert lib.mf_mesh_label_scratch_bytes(5, 3) == 32 and lib.mf_mesh_label_scratch_bytes(big - 1, 0) == 4 * big
    compact = lambda n: (lib.mf_mask_compact_scratch_bytes(n) + 15) // 16 * 16
    assert lib.mf_mesh_table_scratch_bytes(1000, 7) == 4000 + 4000 + 1008 + 16 + compact(1000)
    assert lib.mf_mesh_filter_scratch_bytes(1000, 5000) == 1008 + 1008 + 5008 + 4000 + 16 + max(compact(1000), compact(5000))
    n = 4096 * 1024                                  # mf_mask_compact needs more for n bytes than for n + 1: the filter takes the larger
    assert compact(n) > compact(n + 1)
    assert lib.mf_mesh_filter_scratch_bytes(n, n + 1) == lib.mf_mesh_filter_scratch_bytes(n, n) + 16
    for fn in (lib.mf_mesh_label_scratch_bytes, lib.mf_mesh_table_scratch_bytes, lib.mf_mesh_filter_scratch_bytes):
        for V, T in ((big, 1), (1, big), (-1, 1), (1, -1)):
            assert fn(V, T) == -1 and b"2^31" in lib.mf_last_error()
    for V, T in ((big, 4), (4, big)):
        assert lib.mf_mesh_label(fake, T, V, fake, fake, fake, None) == -1 and b"2^31" in lib.mf_last_error()
        assert lib.mf_mesh_table_count(fake, T, V, fake, fake, fake, None) == -1 and b"2^31" in lib.mf_last_error()
        assert lib.mf_mesh_filter_plan(fake, T, V, fake, fake, fake, 1, fake, fake, None) == -1 and b"2^31" in lib.mf_last_error()
        assert lib.mf_mesh_filter_emit(fake, T, V, 1, 1, fake, fake, fake, fake, None) == -1 and b"2^31" in lib.mf_last_error()
    assert lib.mf_mesh_table_emit(big, 1, fake, fake, fake, fake, None) == -1
    assert lib.mf_mesh_label(fake, 4, 4, fake, None, fake, None) == -1 and b"bad" in lib.mf_last_error()
    assert lib.mf_mesh_table_count(fake, 4, 4, fake, None, fake, None) == -1 and b"counts" in lib.mf_last_error()
    assert lib.mf_mesh_table_emit(4, 5, fake, fake, fake, fake, None) == -1 and b"C=5" in lib.mf_last_error()
    assert lib.mf_mesh_table_emit(4, 2, fake, None, fake, fake, None) == -1 and b"null" in lib.mf_last_error()
    assert lib.mf_mesh_table_emit(4, 0, None, None, None, None, None) == 0
    assert lib.mf_mesh_filter_plan(fake, 4, 4, fake, fake, fake, 5, fake, fake, None) == -1 and b"C=5" in lib.mf_last_error()
    assert lib.mf_mesh_filter_plan(fake, 4, 4, fake, fake, fake, 1, None, fake, None) == -1 and b"counts" in lib.mf_last_error()
    assert lib.mf_mesh_filter_emit(fake, 4, 4, 5, 1, fake, fake, fake, fake, None) == -1 and b"Vk=5" in lib.mf_last_error()
    assert lib.mf_mesh_filter_emit(fake, 4, 4, 1, 5, fake, fake, fake, fake, None) == -1 and b"Tk=5" in lib.mf_last_error()
    assert lib.mf_mesh_filter_emit(fake, 4, 4, 1, 1, fake, None, fake, fake, None) == -1 and b"vert_inds" in lib.mf_last_error()
    assert lib.mf_mesh_filter_emit(None, 4, 4, 0, 0, None, None, None, None, None) == 0
    assert lib.mf_gather_rows(fake, 4, -1, fake, 4, fake, None) == -1
    assert lib.mf_gather_rows(fake, 4, 12, None, 4, fake, None) == -1 and b"null" in lib.mf_last_error()
    assert lib.mf_gather_rows(None, 4, 12, None, 0, None, None) == 0
    assert lib.mf_gather_rows(None, 4, 0, None, 9, None, None) == 0


def test_argument_validation_needs_no_gpu():
    import moco_flow_amd as M
    tris = torch.zeros(4, 3, dtype=torch.int64)
    verts = torch.zeros(5, 3)
    with pytest.raises(RuntimeError, match=r"\(T, 3\)"):
        M.mesh_components(torch.zeros(4, 2, dtype=torch.int64), 5)
    with pytest.raises(RuntimeError, match=r"\(T, 3\)"):
        M.mesh_components(torch.zeros(12, dtype=torch.int64), 5)
    with pytest.raises(RuntimeError, match="int64"):
        M.mesh_components(tris.int(), 5)
    with pytest.raises(RuntimeError, match="n_verts"):
        M.mesh_components(tris, -1)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        M.mesh_components(tris, 5)
    with pytest.raises(ValueError, match="keep_largest, min_triangles"):
        M.filter_components(verts, tris)
    for k in (0, -3):
        with pytest.raises(ValueError, match="at least 1"):
            M.filter_components(verts, tris, keep_largest=k)
        with pytest.raises(ValueError, match="at least 1"):
            M.filter_components(verts, tris, keep_largest=k, min_triangles=2)
    with pytest.raises(RuntimeError, match=r"\(T, 3\)"):
        M.filter_components(verts, tris.view(3, 4), keep_largest=1)
    with pytest.raises(RuntimeError, match="int64"):
        M.filter_components(verts, tris.float(), min_triangles=1)
    with pytest.raises(RuntimeError, match=r"attrs\[1\].*5 vertices"):
        M.filter_components(verts, tris, keep_largest=1, attrs=(torch.zeros(5), torch.zeros(4, 3)))
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        M.filter_components(verts, tris, keep_largest=1, attrs=(torch.zeros(5),))
    # the new keywords reach the same refusals through extract_mesh / extract_colored_mesh
    nerf = M.NeRF(8, 256, 63, [4], "dir", 27)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        M.extract_mesh(nerf, M.Embedding(3, 10), N_grid=8, keep_largest=1)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        M.extract_colored_mesh(nerf, [M.Embedding(3, 10), None, M.Embedding(3, 4)], N_grid=8, min_triangles=4)
