"""CPU-side checks (-m "not gpu") of the mesh simplification: the numpy oracle of its contract (tests/mesh_simplify_oracle.py)
against a brute-force Python loop on hand-made meshes; the library's exports, ABI version and ctypes prototypes; every
refusal that is made before a launch; and that the oracle's results on the meshes of tests/test_gpu_mesh_simplify.py are not
trivial, so that a pass on the device cannot be vacuous.  None of it touches a GPU."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import mesh_simplify_oracle as S

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW_SYMBOLS = ("mf_simplify_mesh_scratch_bytes", "mf_simplify_mesh_plan", "mf_simplify_mesh_emit")


def brute(verts, tris, cell, lo, hi, placement):
    """The contract once more, one vertex and one triangle at a time, with Python floats (float64) and ints."""
    n = [math.floor((hi[a] - lo[a]) / cell) + 1 for a in range(3)]
    cells, fracs = [], []
    for v in verts:
        t = [(float(v[a]) - lo[a]) / cell for a in range(3)]
        c = [math.floor(x) for x in t]
        assert all(lo[a] <= float(v[a]) <= hi[a] for a in range(3))
        cells.append((c[0] * n[1] + c[1]) * n[2] + c[2])
        fracs.append([round((t[a] - c[a]) * 2.0 ** 20) for a in range(3)])     # round(): half to even, as rint
    seen, keep = {}, []
    for k, tri in enumerate(tris):
        a, b, c = (cells[int(i)] for i in tri)
        if a == b or b == c or a == c:
            continue
        key = min((a, b, c), (b, c, a), (c, a, b))
        if key not in seen:
            seen[key] = k
            keep.append(k)
    used = sorted({cells[int(i)] for k in keep for i in tris[k]})
    new = {cid: r for r, cid in enumerate(used)}
    cluster = [new.get(cid, -1) for cid in cells]
    first = [cluster.index(r) for r in range(len(used))]
    tris_k = [[new[cells[int(i)]] for i in tris[k]] for k in keep]
    verts_k = []
    for r, cid in enumerate(used):
        if placement == "first":
            verts_k.append([float(x) for x in verts[first[r]]])
            continue
        members = [v for v in range(len(verts)) if cluster[v] == r]
        c = [cid // (n[1] * n[2]), cid // n[2] % n[1], cid % n[2]]
        verts_k.append([lo[a] + cell * (c[a] + (float(sum(fracs[v][a] for v in members)) / float(len(members))) / 2.0 ** 20)
                        for a in range(3)])
    return (np.array(verts_k, np.float64).reshape(-1, 3).astype(np.float32), np.array(tris_k, np.int64).reshape(-1, 3),
            np.array(first, np.int64), np.array(cluster, np.int64))


@pytest.mark.parametrize("name", sorted(S.hand_meshes()))
@pytest.mark.parametrize("placement", ["mean", "first"])
def test_oracle_equals_brute_force_on_hand_made_meshes(name, placement):
    verts, tris, cell, lo, hi = S.hand_meshes()[name]
    assert len(tris) <= 12
    got = S.simplify(verts, tris, cell, lo, hi, placement)
    want = brute(verts, tris, cell, lo, hi, placement)
    for what, g, w in zip(("verts_k", "tris_k", "first", "cluster"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g.view(np.uint8), w.view(np.uint8)), (name, what, g, w)


def test_hand_made_meshes_show_what_they_were_built_for():
    H = S.hand_meshes()
    r = lambda name: S.simplify(*H[name])
    verts_k, tris_k, first, cluster = r("rotated_duplicate")             # triangles 2, 3, 4 are rotations of 0: 0 survives
    assert S.duplicate_classes(*H["rotated_duplicate"]).tolist() == [4, 1]
    assert tris_k.tolist() == [[0, 2, 1], [2, 3, 1]] and first.tolist() == [0, 2, 1, 6] and cluster.tolist() == [0, 2, 1, 0, 2, 1, 3]
    verts_k, tris_k, first, cluster = r("opposite_winding")              # 0 and its rotation 1 are one class, the flipped 2 stays
    assert tris_k.tolist() == [[0, 2, 1], [0, 1, 2]] and S.duplicate_classes(*H["opposite_winding"]).tolist() == [2, 1]
    verts_k, tris_k, first, cluster = r("degenerate")
    assert len(tris_k) == 2 and cluster.tolist() == [0, 2, 1, 0, 3]
    verts_k, tris_k, first, cluster = r("unused_vertex")                 # 3: alone in its cell, dropped; 5: joins the cell of 0
    assert cluster.tolist() == [0, 2, 1, -1, 3, 0] and first.tolist() == [0, 2, 1, 4]
    verts_k, tris_k, first, cluster = r("speck")                         # four triangles in one cell: all degenerate
    assert cluster.tolist() == [0, 2, 1, 3, -1, -1, -1, -1] and len(tris_k) == 2 and len(verts_k) == 4
    # the mean of the two members of cell (0, 0, 0) of "unused_vertex": vertices 0 and 5
    assert np.array_equal(r("unused_vertex")[0][0], np.array([0.625, 0.375, 0.375], np.float32))
    empty = S.simplify(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64), 1.0)
    assert [a.shape for a in empty] == [(0, 3), (0, 3), (0,), (0,)]
    with pytest.raises(S.BadMesh):
        S.simplify(np.array([[0, 0, np.nan]], np.float32), np.zeros((0, 3), np.int64), 1.0, (0, 0, 0), (1, 1, 1))
    with pytest.raises(S.BadMesh):
        S.simplify(np.array([[0, 0, 2.0]], np.float32), np.zeros((0, 3), np.int64), 1.0, (0, 0, 0), (1, 1, 1))
    with pytest.raises(S.BadMesh):
        S.simplify(np.zeros((2, 3), np.float32), np.array([[0, 1, 2]]), 1.0, (0, 0, 0), (1, 1, 1))


GPU_FIXTURES = [("sphere", c, g) for c in S.SPHERE_CELLS for g in (True, False)] + [("sheet", 1.2, True), ("sheet", 2.5, True),
                                                                                    ("fan", 1.0, True)]


@pytest.mark.parametrize("name,cell,given", GPU_FIXTURES)
def test_gpu_fixtures_are_not_trivial(name, cell, given):
    """Each mesh of the GPU tests loses triangles, keeps some, and has a duplicate class of at least two triangles."""
    verts, tris, bounds = {"sphere": (*S.sphere(), S.SPHERE_BOUNDS), "sheet": (*S.sheet(), S.SHEET_BOUNDS),
                           "fan": (*S.fan(), S.FAN_BOUNDS)}[name]
    lo, hi = bounds if given else (None, None)
    verts_k, tris_k, first, cluster, attr_k = S.expected(name, cell, given)
    classes = S.duplicate_classes(verts, tris, cell, lo, hi)
    print(f"{name} cell {cell} bounds {'given' if given else 'defaulted'}: V {len(verts)} -> {len(verts_k)}, T {len(tris)} -> {len(tris_k)}, "
          f"{int((classes > 1).sum())} duplicate classes, the largest of {int(classes[0])}, {int((cluster < 0).sum())} vertices dropped")
    assert 0 < len(tris_k) < len(tris) and 0 < len(verts_k) < len(verts)
    assert classes[0] >= 2 and len(classes) == len(tris_k)
    assert np.array_equal(attr_k, S.attribute(len(verts))[first])
    if name == "fan":
        assert len(verts_k) == 8 and len(tris_k) <= 8 * 7 * 6 // 3 and classes[0] > 100       # a handful of keys, hundreds of racers each
    if name == "sheet":
        trip = 2048 * 256
        assert len(verts) > trip and len(tris) > trip
        lo, hi, n = S.grid(verts, cell, lo, hi)
        if cell == 1.2:            # every kernel past its first trip: survivors, new vertices and the mask's words as well
            assert len(tris_k) > trip and len(verts_k) > trip and (int(n.prod()) + 31) // 32 > trip
        else:                      # a real reduction; the kernels over the mask's words and over the new vertices stay in one trip
            assert len(tris_k) > trip and len(verts_k) < trip and (int(n.prod()) + 31) // 32 < trip


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
        assert name in listed, name
    assert {n for n in declared if n.startswith("mf_simplify_")} == set(NEW_SYMBOLS)
    i64, p, d, pd = C.c_int64, C.c_void_p, C.c_double, C.POINTER(C.c_double)
    assert L.SYMBOLS["mf_simplify_mesh_scratch_bytes"] == (i64, [i64] * 6)
    assert L.SYMBOLS["mf_simplify_mesh_plan"] == (C.c_int32, [p, i64, p, i64, pd, pd, d, i64, i64, i64, i64, p, p, p])
    assert L.SYMBOLS["mf_simplify_mesh_emit"] == (C.c_int32, [p, i64, p, i64, pd, pd, d, i64, i64, i64, i64, i64, p, p, p, p, p, p, p])
    import moco_flow_amd as M
    assert M.simplify_mesh is M.mesh.simplify_mesh and "simplify_mesh" in M.__all__


def test_host_side_validation():
    """Sizes, the 2^31 limits, the table size and the grid are settled on the host, before anything is launched: the fake
    pointers are never touched."""
    import moco_flow_amd._lib as L
    lib = L.lib()
    fake = C.c_void_p(256)
    big = 1 << 31
    d3 = C.c_double * 3
    lo, hi = d3(0, 0, 0), d3(3, 3, 3)
    size = lib.mf_simplify_mesh_scratch_bytes
    # cellid 4 V | tflag T | mask and word prefix 4 W each | two columns of 2048 workgroup totals | table 4 slots, 16-byte pieces
    assert size(1000, 5000, 4, 4, 4, 8192) == 4000 + 5008 + 16 + 16 + 2 * 8 * 2048 + 4 * 8192
    assert size(0, 0, 1, 1, 1, 1) == 16 + 16 + 2 * 8 * 2048 + 16
    for n in ((big, 1, 1), (1 << 16, 1 << 15, 1), (1 << 11, 1 << 10, 1 << 10), (1 << 40, 1 << 40, 1 << 40), (0, 4, 4), (4, -1, 4)):
        assert size(10, 10, *n, 16) == -1 and b"cells" in lib.mf_last_error(), n
    assert size(10, 10, (1 << 11) - 1, 1 << 10, 1 << 10, 16) > 0                                  # just below 2^31 cells
    for V, T in ((big, 1), (1, big), (-1, 1), (1, -1)):
        assert size(V, T, 4, 4, 4, 1 << 31) == -1 and b"2^31" in lib.mf_last_error()
    for slots in (0, -8, 12, 1000, 8, 4, (1 << 31) + 1, 1 << 32):                                  # not a power of two; <= T; too large
        assert size(10, 8, 4, 4, 4, slots) == -1 and b"slots" in lib.mf_last_error(), slots
    assert size(10, 8, 4, 4, 4, 16) > 0 and size(10, 0, 4, 4, 4, 1) > 0
    plan = lambda **k: lib.mf_simplify_mesh_plan(fake, k.get("V", 10), fake, k.get("T", 8), k.get("lo", lo), k.get("hi", hi),
                                                 k.get("cell", 1.0), *k.get("n", (4, 4, 4)), k.get("slots", 16),
                                                 k.get("counts", fake), fake, None)
    emit = lambda **k: lib.mf_simplify_mesh_emit(fake, k.get("V", 10), fake, k.get("T", 8), k.get("lo", lo), k.get("hi", hi),
                                                 k.get("cell", 1.0), *k.get("n", (4, 4, 4)), k.get("Vk", 3), k.get("Tk", 1), fake,
                                                 fake, fake, fake, fake, k.get("cluster", fake), None)
    for call in (plan, emit):
        assert call(V=big) == -1 and b"2^31" in lib.mf_last_error()
        assert call(T=big, slots=big) == -1 and b"2^31" in lib.mf_last_error()
        assert call(n=(big, 1, 1)) == -1 and b"cells" in lib.mf_last_error()
        for cell in (0.0, -1.0, float("nan"), float("inf")):
            assert call(cell=cell) == -1 and b"cell=" in lib.mf_last_error(), cell
        assert call(hi=d3(3, -1, 3)) == -1 and b"hi >= lo" in lib.mf_last_error()
        assert call(lo=d3(0, float("nan"), 0)) == -1 and b"finite" in lib.mf_last_error()
        assert call(hi=d3(3, float("inf"), 3)) == -1 and b"finite" in lib.mf_last_error()
        assert call(n=(4, 5, 4)) == -1 and b"axis 1 has 5 cells" in lib.mf_last_error()           # not floor((hi - lo) / cell) + 1
        assert call(lo=None) == -1 and b"null" in lib.mf_last_error()
    for slots in (12, 8, 4):
        assert plan(slots=slots) == -1 and b"slots" in lib.mf_last_error()
    assert plan(counts=None) == -1 and b"counts" in lib.mf_last_error()
    assert emit(Vk=11) == -1 and b"Vk=11" in lib.mf_last_error()
    assert emit(Tk=9) == -1 and b"Tk=9" in lib.mf_last_error()
    assert emit(Vk=0, Tk=1) == -1 and emit(Vk=1, Tk=0) == -1
    assert emit(n=(1, 1, 1), hi=d3(0.5, 0.5, 0.5), Vk=2, Tk=1) == -1 and b"1 cells" in lib.mf_last_error()
    assert emit(cluster=None) == -1 and b"cluster" in lib.mf_last_error()
    assert lib.mf_simplify_mesh_emit(None, 0, None, 0, lo, hi, 1.0, 4, 4, 4, 0, 0, None, None, None, None, None, None, None) == 0


def test_argument_validation_needs_no_gpu():
    import moco_flow_amd as M
    verts, tris = torch.zeros(5, 3), torch.zeros(4, 3, dtype=torch.int64)
    with pytest.raises(RuntimeError, match=r"\(T, 3\)"):
        M.simplify_mesh(verts, torch.zeros(4, 2, dtype=torch.int64), 1.0)
    with pytest.raises(RuntimeError, match="int64"):
        M.simplify_mesh(verts, tris.int(), 1.0)
    with pytest.raises(RuntimeError, match=r"\(V, 3\)"):
        M.simplify_mesh(torch.zeros(5, 2), tris, 1.0)
    with pytest.raises(RuntimeError, match=r"\(V, 3\)"):
        M.simplify_mesh(torch.zeros(15), tris, 1.0)
    with pytest.raises(RuntimeError, match="float32"):
        M.simplify_mesh(verts.double(), tris, 1.0)
    with pytest.raises(RuntimeError, match=r"attrs\[1\].*5 vertices"):
        M.simplify_mesh(verts, tris, 1.0, attrs=(torch.zeros(5), torch.zeros(4, 3)))
    with pytest.raises(ValueError, match="placement"):
        M.simplify_mesh(verts, tris, 1.0, placement="median")
    for cell in (0, -2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="cell="):
            M.simplify_mesh(verts, tris, cell)
    with pytest.raises(ValueError, match="below lo"):
        M.simplify_mesh(verts, tris, 1.0, lo=(0, 0, 0), hi=(1, -1, 1))
    with pytest.raises(ValueError, match="both lo and hi"):
        M.simplify_mesh(verts, tris, 1.0, lo=(0, 0, 0))
    with pytest.raises(ValueError, match="3-vectors"):
        M.simplify_mesh(verts, tris, 1.0, lo=(0, 0), hi=(1, 1))
    with pytest.raises(RuntimeError, match="not finite"):
        M.simplify_mesh(verts, tris, 1.0, lo=(0, 0, 0), hi=(1, float("inf"), 1))
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        M.simplify_mesh(verts, tris, 1.0, lo=(0, 0, 0), hi=(1, 1, 1))
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        M.simplify_mesh(verts.cpu(), tris, 1.0, attrs=(torch.zeros(5),))
    # the new keyword reaches the same refusal through extract_mesh / extract_colored_mesh
    nerf = M.NeRF(8, 256, 63, [4], "dir", 27)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        M.extract_mesh(nerf, M.Embedding(3, 10), N_grid=8, simplify=4)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        M.extract_colored_mesh(nerf, [M.Embedding(3, 10), None, M.Embedding(3, 4)], N_grid=8, simplify=2)
