"""CPU-side checks (-m "not gpu") of vertex_rings and smooth_mesh: the numpy oracle of their contracts
(tests/mesh_smooth_oracle.py) against a brute-force restatement with Python sets and one float32 operation at a time on
hand-made meshes; facts about the fixtures tests/test_gpu_mesh_smooth.py relies on, so that a changed fixture is noticed; that
the method smooths (on the oracle); the library's exports, ABI version and ctypes prototypes; every refusal that is made before a
launch.  None of it touches a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import mesh_smooth_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW_SYMBOLS = ("mf_rings_mesh_scratch_bytes", "mf_rings_mesh_plan", "mf_rings_mesh_emit", "mf_smooth_mesh_scratch_bytes",
               "mf_smooth_mesh")


def brute_rings(tris, V):
    pairs = {}
    for tri in tris:
        a, b, c = (int(x) for x in tri)
        if a == b or b == c or a == c:
            continue
        for i, j in ((a, b), (b, a), (b, c), (c, b), (c, a), (a, c)):
            pairs[(i, j)] = pairs.get((i, j), 0) + 1
    rings = [sorted({j for (i, j) in pairs if i == v}) for v in range(V)]
    boundary = [any(pairs[(v, j)] == 1 for j in rings[v]) for v in range(V)]
    offsets = np.cumsum([0] + [len(r) for r in rings]).astype(np.int64)
    return offsets, np.array([j for r in rings for j in r], np.int64), np.array(boundary, bool)


def brute_smooth(verts, rings, iterations, lam, mu, boundary):
    offsets, ring, bnd = rings
    f32 = np.float32
    p = [[f32(x) for x in row] for row in verts]
    factors = [lam] * iterations if mu is None else [lam, mu] * iterations
    for f in factors:
        f = f32(f)
        q = [list(row) for row in p]
        for v in range(len(p)):
            nb = [int(j) for j in ring[offsets[v]:offsets[v + 1]]]
            if not nb or (boundary == "fixed" and bnd[v]):
                continue
            for a in range(3):
                s = p[nb[0]][a]
                for j in nb[1:]:
                    s = f32(s + p[j][a])
                m = f32(s / f32(len(nb)))
                d = f32(m - p[v][a])
                q[v][a] = f32(p[v][a] + f32(f * d))
        p = q
    return np.array(p, np.float32).reshape(-1, 3)


@pytest.mark.parametrize("name", sorted(O.hand_meshes()))
def test_oracle_equals_brute_force_on_hand_made_meshes(name):
    verts, tris = O.hand_meshes()[name]
    assert len(tris) <= 12
    got, want = O.rings(tris, len(verts)), brute_rings(tris, len(verts))
    for what, g, w in zip(("offsets", "ring", "boundary"), got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w), (name, what, g, w)
    for iterations, mu, boundary in ((1, O.MU, "fixed"), (3, O.MU, "free"), (3, None, "fixed"), (2, None, "free"), (0, O.MU, "fixed")):
        g = O.smooth(verts, tris, iterations, O.LAM, mu, boundary)
        w = brute_smooth(verts, want, iterations, O.LAM, mu, boundary)
        assert g.dtype == np.float32 and np.array_equal(g.view(np.uint32), w.view(np.uint32)), (name, iterations, mu, boundary)


def test_hand_made_meshes_show_what_they_were_built_for():
    H = O.hand_meshes()
    r = lambda name: O.rings(H[name][1], len(H[name][0]))
    for closed in ("tetrahedron", "octahedron", "twelve"):
        assert not r(closed)[2].any(), closed
    assert r("tetrahedron")[1].tolist() == [1, 2, 3, 0, 2, 3, 0, 1, 3, 0, 1, 2]
    assert r("one_triangle")[2].all() and r("one_triangle")[0].tolist() == [0, 2, 4, 6]
    offsets, ring, boundary = r("two_on_an_edge")
    assert ring.tolist() == [1, 2, 0, 2, 3, 0, 1, 3, 1, 2] and boundary.all()
    offsets, ring, boundary = r("three_on_an_edge")                      # edge 0-1 is in three triangles; the others in one
    assert O.max_multiplicity(H["three_on_an_edge"][1], 5) == 3 and boundary.all()
    only = np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4], [2, 1, 0], [3, 0, 1], [4, 1, 0]])      # every other edge twice
    assert O.rings(only, 5)[2].tolist() == [False] * 5                   # 0 and 1 are not boundary through their shared edge
    for name in ("same_twice", "both_windings"):                         # m changes, the ring does not
        offsets, ring, boundary = r(name)
        assert ring.tolist() == [1, 2, 0, 2, 3, 0, 1, 3, 1, 2], name
        assert boundary.tolist() == [False, True, True, True], name      # 0 touches only the doubled triangle's edges
    offsets, ring, boundary = r("repeated_index")                        # three of five triangles are skipped
    assert np.array_equal(ring, O.rings(np.array([[0, 1, 2], [2, 1, 3]]), 5)[1]) and offsets[-1] - offsets[-2] == 0
    offsets, ring, boundary = r("lonely_vertex")
    assert offsets[4] - offsets[3] == 0 and offsets[6] - offsets[5] == 0 and not boundary[3] and not boundary[5]
    verts = H["lonely_vertex"][0]
    moved = O.smooth(verts, H["lonely_vertex"][1], 3, boundary="free")
    assert np.array_equal(moved[[3, 5]], verts[[3, 5]]) and not np.array_equal(moved[0], verts[0])
    empty = O.rings(np.zeros((0, 3), np.int64), 0)
    assert empty[0].tolist() == [0] and empty[1].shape == (0,) and empty[2].shape == (0,)
    with pytest.raises(O.BadMesh):
        O.rings(np.array([[0, 1, 3]]), 3)


FACTS = {"sphere": dict(V=2482, T=4668, degenerate=0, R=14004, boundary=0, max_raw=26, above_64=0, max_m=2),
         "sheet": dict(V=547600, T=1092242, degenerate=0, R=3279682, boundary=2956, max_raw=12, above_64=0, max_m=2),
         "fan": dict(V=4096, T=50000, degenerate=38, R=297174, boundary=4096, max_raw=118, above_64=3059, max_m=3)}


@pytest.mark.parametrize("name", sorted(FACTS))
def test_facts_about_the_gpu_fixtures(name):
    verts, tris = getattr(O, name)()
    V = len(verts)
    offsets, ring, boundary = O.expected_rings(name)
    raw = O.raw_entries(tris, V)
    got = dict(V=V, T=len(tris), degenerate=int(((tris[:, 0] == tris[:, 1]) | (tris[:, 1] == tris[:, 2]) | (tris[:, 0] == tris[:, 2])).sum()),
               R=len(ring), boundary=int(boundary.sum()), max_raw=int(raw.max()), above_64=int((raw > 64).sum()),
               max_m=O.max_multiplicity(tris, V))
    assert got == FACTS[name]
    if name == "sheet":
        trip = 2048 * 256                                                # every kernel over vertices, triangles and ring entries
        assert V > trip and len(tris) > trip and len(ring) > trip        # goes past its first trip
        assert int(boundary.sum()) == 4 * O.S.SHEET_N - 4
    if name == "fan":
        import moco_flow_amd.mesh as mesh
        assert (raw > 32).sum() > 3059 and raw.max() < 2 * mesh.MAX_TRIANGLES_PER_VERTEX     # the long path, below the cap


def _umbrella(p, rings):
    offsets, ring, _ = rings
    n = (offsets[1:] - offsets[:-1])[:, None]
    return float(np.linalg.norm(np.add.reduceat(p[ring].astype(np.float64), offsets[:-1]) / n - p, axis=1).mean())


def _volume(p, tris):
    a, b, c = (p[tris[:, k]].astype(np.float64) for k in range(3))
    return abs(float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum()) / 6.0)


def test_smoothing_smooths_on_the_oracle():
    """Properties of the method on the sphere fixture: the umbrella vector shrinks to less than half, and Taubin's 10 iterations
    change the enclosed volume less than 20 plain Laplacian steps do."""
    verts, tris = O.sphere()
    rings = O.expected_rings("sphere")
    taubin, laplace = O.expected_smooth("sphere", 10), O.expected_smooth("sphere", 20, "fixed", None)
    u0, u1 = _umbrella(verts, rings), _umbrella(taubin, rings)
    v0, vt, vl = _volume(verts, tris), _volume(taubin, tris), _volume(laplace, tris)
    print(f"umbrella {u0:.3f} -> {u1:.3f}; volume {v0:.1f} -> {vt:.1f} (Taubin), {vl:.1f} (Laplace)")
    assert u1 < 0.5 * u0
    assert abs(vt - v0) < abs(vl - v0)


def test_boundary_modes_on_the_sheet():
    verts, _ = O.sheet()
    _, _, boundary = O.expected_rings("sheet")
    assert int(boundary.sum()) == 2956
    fixed, free = O.expected_smooth("sheet", 2, "fixed"), O.expected_smooth("sheet", 2, "free")
    assert np.array_equal(fixed[boundary].view(np.uint32), verts[boundary].view(np.uint32))
    assert (free[boundary] != verts[boundary]).any(1).all()              # every rim vertex moves
    assert (fixed[~boundary] != verts[~boundary]).any()


def test_library_exports_header_symbols_and_prototypes():
    import moco_flow_amd as M
    import moco_flow_amd._lib as L
    header = open(os.path.join(ROOT, "include", "mocoflow_hip.h")).read()
    declared = set(re.findall(r"^int(?:32|64)_t (mf_\w+)\(", header, re.M))
    lib = L.lib()
    assert lib.mf_version() == 16 and L.MF_ABI_VERSION == 16
    assert "#define MF_ABI_VERSION 16" in header
    additive = header[header.index("additive entries since, version unchanged"):header.index("#define MF_ABI_VERSION")]
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in additive, name
        fn = getattr(lib, name)
        assert fn.restype is L.SYMBOLS[name][0] and list(fn.argtypes) == L.SYMBOLS[name][1]
    assert {n for n in declared if n.startswith(("mf_rings_", "mf_smooth_"))} == set(NEW_SYMBOLS)
    for entry in ("mf_rings_mesh_plan (serves", "mf_rings_mesh_emit (serves", "mf_smooth_mesh (serves"):
        doc = header[header.index(entry):]
        doc = doc[:doc.index("*/")]
        for cite in ("trainer_moco_flow.py:490-538", "trainer_nerf.py:200-259"):
            assert cite in doc, (entry, cite)
    i64, i32, p, f = C.c_int64, C.c_int32, C.c_void_p, C.c_float
    assert L.SYMBOLS["mf_rings_mesh_scratch_bytes"] == (i64, [i64, i64])
    assert L.SYMBOLS["mf_rings_mesh_plan"] == (i32, [p, i64, i64, p, p, p, p, p])
    assert L.SYMBOLS["mf_rings_mesh_emit"] == (i32, [i64, i64, i64, p, p, p, p])
    assert L.SYMBOLS["mf_smooth_mesh_scratch_bytes"] == (i64, [i64, i64])
    assert L.SYMBOLS["mf_smooth_mesh"] == (i32, [p, i64, p, p, i64, p, i32, f, f, i32, p, p, p])
    for name in ("vertex_rings", "smooth_mesh"):
        assert getattr(M, name) is getattr(M.mesh, name) and name in M.__all__
    assert M.mesh.MAX_TRIANGLES_PER_VERTEX >= 2048
    assert f"#define MF_MESH_MAX_TRIANGLES_PER_VERTEX {M.mesh.MAX_TRIANGLES_PER_VERTEX}\n" in header
    assert "mf_mesh_smooth.hip" in open(os.path.join(ROOT, "moco_flow_amd", "csrc", "Makefile")).read()


def test_host_side_validation():
    """Sizes, the 2^31 limits and null arguments are settled on the host, before anything is launched: the fake pointers are
    never touched."""
    import moco_flow_amd._lib as L
    lib = L.lib()
    fake = C.c_void_p(256)
    big = 1 << 31
    size = lib.mf_rings_mesh_scratch_bytes
    assert size(big, 1) == -1 and b"2^31" in lib.mf_last_error()
    for T in ((big + 5) // 6, big // 6 + 1, big, 1 << 40):               # 6 T >= 2^31
        assert 6 * T >= big and size(10, T) == -1 and b"2^31" in lib.mf_last_error(), T
    assert size(-1, 1) == -1 and size(1, -1) == -1
    assert 6 * ((big - 1) // 6) < big and size(big - 1, (big - 1) // 6) > 0                       # just below both bounds
    last = 0
    for V, T in ((0, 0), (1, 0), (1, 1), (10, 1), (10, 20), (1000, 20), (1000, 2000), (10 ** 6, 2 * 10 ** 6), (10 ** 8, 2 * 10 ** 8)):
        assert size(V, T) > last, (V, T)                                 # positive and monotone
        last = size(V, T)
    # hdr 16 | deg 4 V | raw_off 4 (V + 1) | ucount 4 V | 2048 share totals | list 4 min(V, 6 T / 33 + 1) | raw 24 T, 16-byte pieces
    assert size(1000, 5000) == 16 + 4000 + 4016 + 4000 + 8 * 2048 + 3648 + 120000
    plan = lambda **k: lib.mf_rings_mesh_plan(k.get("tris", fake), k.get("T", 8), k.get("V", 10), k.get("counts", fake),
                                              k.get("offsets", fake), k.get("boundary", fake), k.get("scratch", fake), None)
    assert plan(V=big) == -1 and b"2^31" in lib.mf_last_error()
    assert plan(T=big // 6 + 1) == -1 and b"2^31" in lib.mf_last_error()
    for null in ("tris", "counts", "offsets", "boundary", "scratch"):
        assert plan(**{null: None}) == -1 and b"null" in lib.mf_last_error(), null
    emit = lambda **k: lib.mf_rings_mesh_emit(k.get("V", 10), k.get("T", 8), k.get("R", 12), k.get("scratch", fake),
                                              k.get("offsets", fake), k.get("ring", fake), None)
    assert emit(V=big) == -1 and b"2^31" in lib.mf_last_error()
    assert emit(R=49) == -1 and b"R=49" in lib.mf_last_error()
    assert emit(R=-1) == -1
    for null in ("scratch", "offsets", "ring"):
        assert emit(**{null: None}) == -1 and b"null" in lib.mf_last_error(), null
    assert emit(R=0, scratch=None, offsets=None, ring=None) == 0        # nothing is launched
    ssize = lib.mf_smooth_mesh_scratch_bytes
    assert ssize(big, 1) == -1 and ssize(1, big) == -1 and ssize(-1, 0) == -1 and b"2^31" in lib.mf_last_error()
    assert ssize(1000, 6000) == 2 * 16000 + 4016 + 24000                 # two buffers of 16-byte rows, int32 offsets and ring
    smooth = lambda **k: lib.mf_smooth_mesh(k.get("verts", fake), k.get("V", 10), k.get("offsets", fake), k.get("ring", fake),
                                            k.get("R", 12), fake, k.get("iterations", 2), k.get("lam", 0.5), k.get("mu", -0.53),
                                            k.get("taubin", 1), k.get("out", fake), k.get("scratch", fake), None)
    assert smooth(V=big) == -1 and b"2^31" in lib.mf_last_error()
    assert smooth(R=big) == -1 and b"2^31" in lib.mf_last_error()
    assert smooth(iterations=-1) == -1 and b"iterations=-1" in lib.mf_last_error()
    assert smooth(lam=float("nan")) == -1 and b"finite" in lib.mf_last_error()
    assert smooth(mu=float("inf")) == -1 and b"finite" in lib.mf_last_error()
    for null in ("verts", "out", "offsets", "ring", "scratch"):
        assert smooth(**{null: None}) == -1 and b"null" in lib.mf_last_error(), null
    assert smooth(V=0, verts=None, out=None) == 0                        # nothing is launched


def test_argument_validation_needs_no_gpu():
    import moco_flow_amd as M
    verts, tris = torch.zeros(5, 3), torch.zeros(4, 3, dtype=torch.int64)
    for bad in (-1, 1.5, "3", None, True):
        with pytest.raises(ValueError, match="iterations"):
            M.smooth_mesh(verts, tris, iterations=bad)
    for name in ("lam", "mu"):
        for bad in (float("nan"), float("inf"), -float("inf"), "x"):
            with pytest.raises(ValueError, match=name):
                M.smooth_mesh(verts, tris, **{name: bad})
    with pytest.raises(ValueError, match="lam"):
        M.smooth_mesh(verts, tris, lam=None)
    with pytest.raises(ValueError, match="boundary"):
        M.smooth_mesh(verts, tris, boundary="pinned")
    rings = (torch.zeros(5, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), torch.zeros(5, dtype=torch.bool))
    with pytest.raises(ValueError, match=r"V \+ 1"):
        M.smooth_mesh(verts, tris, rings=rings)
    with pytest.raises(ValueError, match="rings"):
        M.smooth_mesh(verts, tris, rings=rings[:2])
    with pytest.raises(ValueError, match="iterations"):                  # argument errors come before the tensors are looked at
        M.smooth_mesh(torch.zeros(5, 2), tris, iterations=-2)
    with pytest.raises(RuntimeError, match=r"\(T, 3\)"):
        M.smooth_mesh(verts, torch.zeros(4, 2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="int64"):
        M.vertex_rings(tris.int(), 5)
    with pytest.raises(RuntimeError, match="float32"):
        M.smooth_mesh(verts.double(), tris)
    with pytest.raises(RuntimeError, match="n_verts=-1"):
        M.vertex_rings(tris, -1)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        M.vertex_rings(tris, 5)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        M.smooth_mesh(verts, tris)
    for bad in (0, -3, 2.5, True, "2", dict(steps=3), dict(iterations=-1), dict(boundary="x"), dict(lam=float("nan"))):
        with pytest.raises(ValueError, match="extract_mesh"):
            M.mesh._smooth_kwargs(bad, "extract_mesh")
    assert M.mesh._smooth_kwargs(3, "x") == {"iterations": 3}
    assert M.mesh._smooth_kwargs(dict(iterations=2, mu=None), "x") == {"iterations": 2, "mu": None}
