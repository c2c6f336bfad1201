"""CPU-side checks (-m "not gpu") of the device marching cubes: the committed case table (mf_mc_tables.hpp), the numpy
oracle of the kernel's contract (tests/mc_oracle.py) against scikit-image's Lorensen meshes (tests/golden/m_mesh.npz),
the meshes' topology and orientation, host-side validation of mf_mc_*, CPU tensors raising, export_obj."""
import ctypes
import os

import numpy as np
import pytest
import torch

import mc_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "m_mesh.npz"))
NAMES = ("ball", "torus", "noise", "noncubic", "boundary", "nerf")


def fixture(name):
    return GOLD[name + "_vol"], float(GOLD[name + "_iso"]), bool(GOLD[name + "_clamp"])


def edge_corners(e):
    a, o = O.edge_offset(e)
    lo = 4 * o[0] + 2 * o[1] + o[2]
    return lo, lo + (4, 2, 1)[a]


def test_case_table_properties():
    ntri, edges = O.NTRI, O.EDGES
    assert ntri.shape == (256,) and edges.shape == (256, 15)
    assert ntri[0] == 0 and ntri[255] == 0 and ntri.max() == 5 and ntri.sum() == 820
    for c in range(256):
        used = edges[c, :3 * ntri[c]]
        assert np.all(edges[c, 3 * ntri[c]:] == -1)
        assert np.all((used >= 0) & (used < 12))
        for e in used:                                    # a triangle corner sits on an edge that crosses the surface
            c0, c1 = edge_corners(int(e))
            assert (c >> c0 & 1) != (c >> c1 & 1), (c, e)
        crossing = {e for e in range(12) if (c >> edge_corners(e)[0] & 1) != (c >> edge_corners(e)[1] & 1)}
        assert set(used.tolist()) == crossing, c         # and every crossing edge carries a vertex
        tris = used.reshape(-1, 3)
        assert np.all((tris[:, 0] != tris[:, 1]) & (tris[:, 1] != tris[:, 2]) & (tris[:, 0] != tris[:, 2]))
    for c in range(8):                                    # one corner alone: one triangle
        assert ntri[1 << c] == 1 and ntri[255 ^ (1 << c)] == 1


@pytest.mark.parametrize("name", NAMES)
def test_oracle_equals_skimage_fixture(name):
    vol, iso, clamp = fixture(name)
    verts, tris = O.marching_cubes(vol, iso, clamp)
    assert verts.dtype == np.float32 and tris.dtype == np.int64
    assert len(tris) > 0
    ok, msg = O.same_mesh_as_sets(verts, tris, GOLD[name + "_verts"], GOLD[name + "_faces"])
    assert ok, f"{name}: {msg}"


def directed_edges(tris):
    return np.concatenate([tris[:, [0, 1]], tris[:, [1, 2]], tris[:, [2, 0]]])


@pytest.mark.parametrize("name", ["ball", "torus"])
def test_closed_surfaces_are_watertight_and_oriented(name):
    vol, iso, clamp = fixture(name)
    verts, tris = O.marching_cubes(vol, iso, clamp)
    d = directed_edges(tris)
    und = np.sort(d, 1)
    _, cnt = np.unique(und, axis=0, return_counts=True)
    assert np.all(cnt == 2)                               # every edge in exactly two triangles
    _, dcnt = np.unique(d, axis=0, return_counts=True)
    assert np.all(dcnt == 1)                              # ... traversed once each way: consistently oriented
    E = len(cnt)
    assert len(np.unique(tris)) == len(verts)
    assert len(verts) - E + len(tris) == (2 if name == "ball" else 0)
    # raw winding: the signed volume enclosed (index coordinates (axis 0, 1, 2), right-hand rule) is positive -- normals
    # point from the below-iso side to the other, out of the ball
    p = verts[tris].astype(np.float64)
    signed = np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6
    assert signed > 0


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_volumes_are_consistently_oriented(seed):
    """Open and multi-component surfaces: no directed edge twice, interior edges shared by exactly two triangles."""
    rng = np.random.default_rng(seed)
    vol = rng.standard_normal((9, 11, 13)).astype(np.float32)
    verts, tris = O.marching_cubes(vol, 0.0)
    d = directed_edges(tris)
    _, dcnt = np.unique(d, axis=0, return_counts=True)
    assert np.all(dcnt == 1)
    und, cnt = np.unique(np.sort(d, 1), axis=0, return_counts=True)
    assert np.all(cnt <= 2)
    # an edge used by one triangle lies on the volume's boundary
    shape = np.array(vol.shape) - 1
    for a, b in und[cnt == 1]:
        pa, pb = verts[a], verts[b]
        assert any((pa[x] in (0, shape[x])) and pa[x] == pb[x] for x in range(3)), (pa, pb)


def test_all_cases_volume_covers_the_table():
    vol = O.all_cases_volume()
    case = O._cases(vol < 0)[0, 0]
    assert set(case[0::2].tolist()) == set(range(256))
    verts, tris = O.marching_cubes(vol, 0.0)
    assert len(tris) >= 820


def test_slab_and_counts_agree_with_the_whole_volume():
    vol = np.random.default_rng(5).standard_normal((12, 7, 9)).astype(np.float32)
    verts, tris = O.marching_cubes(vol, 0.2)
    assert O.counts(vol, 0.2, chunk=5) == (len(verts), len(tris))
    sv, st, V0, T0 = O.slab(vol, 0.2, 4, 8)
    assert np.array_equal(sv, verts[V0:V0 + len(sv)]) and np.array_equal(st, tris[T0:T0 + len(st)])


def test_host_side_validation():
    import moco_flow_amd._lib as L
    lib = L.lib()
    assert lib.mf_mc_scratch_bytes(512, 512, 512) == 4 * 512 ** 3 + 24 * (512 ** 3 // 1024)
    assert lib.mf_mc_scratch_bytes(2, 2, 2) == 4 * 8 + 24
    for shape in [(1, 4, 4), (4, 4, 1), (0, 2, 2), (2048, 2048, 1024), (1 << 31, 2, 2)]:
        assert lib.mf_mc_scratch_bytes(*shape) == -1, shape
        assert lib.mf_last_error()
    # over-large or null arguments are refused on the host, before anything is launched (the pointers are never touched)
    fake = ctypes.c_void_p(256)
    assert lib.mf_mc_count(fake, 2048, 2048, 1024, 0.0, 0, fake, fake, None) == -1
    assert b"2^31" in lib.mf_last_error()
    assert lib.mf_mc_count(None, 4, 4, 4, 0.0, 0, fake, fake, None) == -1
    assert lib.mf_mc_emit(fake, 4, 1, 4, 0.0, 0, fake, fake, fake, None) == -1
    assert lib.mf_mc_emit(fake, 4, 4, 4, 0.0, 0, None, fake, fake, None) == -1


def test_cpu_tensors_raise():
    import moco_flow_amd as M
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        M.marching_cubes(torch.zeros(4, 4, 4), 0.5)
    nerf = M.NeRF(8, 256, 63, [4], "dir", 27)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        M.extract_mesh(nerf, M.Embedding(3, 10), N_grid=8)


def test_export_obj(tmp_path):
    import moco_flow_amd as M
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1.25, 0], [0, 0, -1]], np.float32)
    tris = np.array([[0, 2, 1], [0, 1, 3]], np.int64)
    path = tmp_path / "m.obj"
    M.export_obj(str(path), torch.from_numpy(verts), torch.from_numpy(tris))
    lines = path.read_text().splitlines()
    v = np.array([[float(x) for x in ln.split()[1:]] for ln in lines if ln.startswith("v ")])
    f = np.array([[int(x) for x in ln.split()[1:]] for ln in lines if ln.startswith("f ")])
    assert np.array_equal(v, verts) and np.array_equal(f, tris + 1)
    assert [ln[0] for ln in lines] == ["v"] * 4 + ["f"] * 2
