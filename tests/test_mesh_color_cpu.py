"""CPU-side checks (-m "not gpu") of the coloured-mesh path: the new C entries (mf_points_radiance, mf_mc_normals) exist with
their ctypes prototypes and validate their arguments on the host, the Python surface is exported, export_ply round-trips,
and the numpy oracle of mf_mc_normals (tests/mesh_color_oracle.py) is held to a closed form."""
import ctypes
import os

import numpy as np
import pytest
import torch

import mc_oracle as O
import mesh_color_oracle as N

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "m_mesh.npz"))

MF_OK, MF_E_INVALID, MF_E_UNSUPPORTED = 0, -1, -3


def nerf_desc(L, kind, dim, W=256):
    d = L.mf_nerf_desc()
    d.D, d.W, d.in_channels_xyz, d.skip_mask = 8, W, 63, 1 << 4
    d.extra_feat_type, d.extra_feat_dim = kind, dim
    return d


def embedding(L, channels, n_freqs):
    e = L.mf_embedding()
    e.in_channels, e.n_freqs = channels, n_freqs
    for k in range(min(n_freqs, L.MF_MAX_FREQS)):
        e.freq[k], e.weight[k] = float(2 ** k), 1.0
    return e


def test_abi_version_and_symbols():
    import moco_flow_amd._lib as L
    lib = L.lib()
    assert lib.mf_version() == L.MF_ABI_VERSION == 16
    header = open(os.path.join(os.path.dirname(HERE), "include", "mocoflow_hip.h")).read()
    for name, n_args in (("mf_points_radiance", 16), ("mf_mc_normals", 9)):
        assert hasattr(lib, name), f"{name} is not exported"
        res, args = L.SYMBOLS[name]
        assert res is ctypes.c_int32 and len(args) == n_args
        decl = header.split(f"int32_t {name}(", 1)[1].split(");", 1)[0]
        assert decl.count(",") + 1 == n_args, f"{name}: the header declares another argument count"
    _, args = L.SYMBOLS["mf_points_radiance"]
    assert args[11] is ctypes.c_float and args[12] is ctypes.c_int64               # ind_scalar, B
    _, args = L.SYMBOLS["mf_mc_normals"]
    assert args[1:5] == [ctypes.c_int64] * 3 + [ctypes.c_int32] and args[6] is ctypes.c_int64
    assert "mf_points_radiance" in header.split("#define MF_ABI_VERSION")[0]      # listed in the history comment
    assert "mf_mc_normals" in header.split("#define MF_ABI_VERSION")[0]


def test_points_radiance_validates_on_the_host():
    """Null pointers, an extra embedding wider than the NeRF's block and an unsupported NeRF are refused before anything is
    launched (the fake pointers are never touched); B == 0 is MF_OK without a launch."""
    import moco_flow_amd._lib as L
    lib = L.lib()
    fake = ctypes.c_void_p(256)
    ref = ctypes.byref
    exyz, edir, eind = embedding(L, 3, 10), embedding(L, 3, 4), embedding(L, 1, 2)
    d_dir, d_ind, d_none = nerf_desc(L, L.MF_EXTRA_DIR, 27), nerf_desc(L, L.MF_EXTRA_IND, 5), nerf_desc(L, L.MF_EXTRA_NONE, 0)

    def call(d, packed=fake, ex=exyz, ee=None, xyz=fake, dirs=None, B=8, out=fake, nof=None, nof_packed=None, nx=None, ni=None):
        return lib.mf_points_radiance(ref(d) if d is not None else None, packed, ref(ex) if ex is not None else None,
                                      ref(ee) if ee is not None else None, ref(nof) if nof is not None else None, nof_packed,
                                      ref(nx) if nx is not None else None, ref(ni) if ni is not None else None, xyz, dirs, None,
                                      0.0, B, out, None, None)

    # B == 0: nothing is read, nothing launched
    assert call(d_dir, ee=edir, xyz=None, out=None, B=0) == MF_OK
    assert call(d_ind, ee=eind, xyz=None, out=None, B=0) == MF_OK
    assert call(d_none, xyz=None, out=None, B=0) == MF_OK
    # null arguments
    assert call(None, ee=edir, dirs=fake) == MF_E_INVALID and b"null" in lib.mf_last_error()
    assert call(d_dir, packed=None, ee=edir, dirs=fake) == MF_E_INVALID
    assert call(d_dir, ex=None, ee=edir, dirs=fake) == MF_E_INVALID
    assert call(d_dir, ee=edir, dirs=fake, xyz=None) == MF_E_INVALID
    assert call(d_dir, ee=edir, dirs=fake, out=None) == MF_E_INVALID
    assert call(d_dir, ee=edir, dirs=None) == MF_E_INVALID and b"view_dirs" in lib.mf_last_error()
    assert call(d_dir, ee=None, dirs=fake) == MF_E_INVALID
    assert call(d_ind, ee=None) == MF_E_INVALID
    assert call(d_none, B=-1) == MF_E_INVALID
    # an extra embedding wider than the block (mf_render_pass's bounds)
    assert call(nerf_desc(L, L.MF_EXTRA_DIR, 26), ee=edir, dirs=fake) == MF_E_INVALID and b"fit" in lib.mf_last_error()
    assert call(d_dir, ee=embedding(L, 3, 5), dirs=fake) == MF_E_INVALID
    assert call(d_dir, ee=eind, dirs=fake) == MF_E_INVALID                     # one channel where three are embedded
    assert call(nerf_desc(L, L.MF_EXTRA_IND, 4), ee=eind) == MF_E_INVALID
    assert call(d_ind, ee=embedding(L, 1, 3)) == MF_E_INVALID
    assert call(d_ind, ee=edir) == MF_E_INVALID
    # a NeRF the kernels are not built for
    assert call(nerf_desc(L, L.MF_EXTRA_DIR, 27, W=192), ee=edir, dirs=fake) == MF_E_UNSUPPORTED
    assert call(nerf_desc(L, L.MF_EXTRA_DIR, 27, W=128), ee=edir, dirs=fake) == MF_E_UNSUPPORTED
    assert b"unsupported" in lib.mf_last_error()
    assert call(d_none, ex=embedding(L, 3, 11)) == MF_E_UNSUPPORTED
    # a NoF without its packed weights / embeddings
    nof = L.mf_nof_desc()
    nof.D, nof.W, nof.in_channels_xyz, nof.extra_feat_dim, nof.skip_mask, nof.use_quat = 4, 128, 33, 33, 1 << 2, 1
    assert call(d_none, nof=nof) == MF_E_INVALID and b"NoF" in lib.mf_last_error()
    assert call(d_none, nof=nof, nof_packed=fake, nx=embedding(L, 3, 5), ni=embedding(L, 1, 16), xyz=None, out=None, B=0) == MF_OK


def test_mc_normals_validates_on_the_host():
    import moco_flow_amd._lib as L
    lib = L.lib()
    fake = ctypes.c_void_p(256)
    assert lib.mf_mc_normals(fake, 4, 4, 4, 0, None, 0, None, None) == MF_OK                   # V == 0: no launch
    assert lib.mf_mc_normals(None, 4, 4, 4, 1, None, 0, None, None) == MF_OK
    for shape in [(1, 4, 4), (4, 4, 1), (0, 2, 2), (2048, 2048, 1024)]:
        assert lib.mf_mc_normals(fake, *shape, 0, fake, 5, fake, None) == MF_E_INVALID, shape
    assert b"2^31" in lib.mf_last_error()
    assert lib.mf_mc_normals(None, 4, 4, 4, 0, fake, 5, fake, None) == MF_E_INVALID and b"null" in lib.mf_last_error()
    assert lib.mf_mc_normals(fake, 4, 4, 4, 0, None, 5, fake, None) == MF_E_INVALID
    assert lib.mf_mc_normals(fake, 4, 4, 4, 0, fake, 5, None, None) == MF_E_INVALID
    assert lib.mf_mc_normals(fake, 4, 4, 4, 0, fake, -1, fake, None) == MF_E_INVALID


def test_python_surface():
    import moco_flow_amd as M
    for name in ("query_radiance", "extract_colored_mesh", "vertex_normals", "export_ply"):
        assert name in M.__all__ and callable(getattr(M, name)), name
    nerf = M.NeRF(8, 256, 63, [4], "dir", 27)
    embs = [M.Embedding(3, 10), None, M.Embedding(3, 4)]
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        M.query_radiance(torch.zeros(4, 3), nerf, embs, view_dirs=torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        M.vertex_normals(torch.zeros(4, 4, 4), torch.zeros(2, 3))
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        M.extract_colored_mesh(nerf, embs, N_grid=8)
    latent = M.NeRF(8, 256, 63, [4], "latent_code", 16)
    with pytest.raises(NotImplementedError):
        M.query_radiance(torch.zeros(4, 3), latent, embs)


def ply_case(tmp_path, M, verts, tris, colors, normals, tensors):
    path = str(tmp_path / "m.ply")
    wrap = (lambda a: None if a is None else torch.from_numpy(a)) if tensors else (lambda a: a)
    M.export_ply(path, wrap(verts), wrap(tris), colors=wrap(colors), normals=wrap(normals))
    lines, v, f = N.read_ply(path)
    names = ["x", "y", "z"] + (["nx", "ny", "nz"] if normals is not None else []) + (["red", "green", "blue"] if colors is not None else [])
    assert list(v.dtype.names) == names
    want = [f"property float {n}" for n in names if n not in ("red", "green", "blue")] + \
           [f"property uchar {n}" for n in names if n in ("red", "green", "blue")]
    assert [ln for ln in lines if ln.startswith("property") and "list" not in ln] == want
    assert f"element vertex {len(verts)}" in lines and f"element face {len(tris)}" in lines
    assert "property list uchar int vertex_indices" in lines
    assert np.array_equal(np.stack([v["x"], v["y"], v["z"]], 1).reshape(-1, 3), verts)
    assert f.dtype == np.dtype("<i4") and np.array_equal(f.reshape(-1, 3), tris)
    if normals is not None:
        assert np.array_equal(np.stack([v["nx"], v["ny"], v["nz"]], 1).reshape(-1, 3), normals)
    return v


def test_export_ply_round_trip(tmp_path):
    import moco_flow_amd as M
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1.25, 0], [0, 0, -1], [1e-3, 2.5, 7]], np.float32)
    tris = np.array([[0, 2, 1], [0, 1, 3], [4, 3, 2]], np.int64)
    normals = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0], [0, 0, 0], [0.6, -0.8, 0]], np.float32)
    # 0.5 / 255 is a rounding tie (round half to even -> 0), 1.5 / 255 -> 2; out-of-range values clamp
    colors = np.array([[0, 1, 0.5], [0.25, 0.75, 1.0 / 255], [-0.2, 1.3, 0.999], [0.5 / 255, 1.5 / 255, 254.6 / 255], [0.1, 0.2, 0.3]],
                      np.float32)
    want_u1 = np.clip(np.rint(255.0 * colors.astype(np.float64)), 0, 255).astype(np.uint8)
    assert want_u1[2].tolist() == [0, 255, 255] and want_u1[0].tolist() == [0, 255, 128]
    for tensors in (True, False):
        for c, n in ((colors, normals), (colors, None), (None, normals), (None, None)):
            v = ply_case(tmp_path, M, verts, tris, c, n, tensors)
            if c is not None:
                assert v["red"].dtype == np.uint8
                assert np.array_equal(np.stack([v["red"], v["green"], v["blue"]], 1), want_u1)
    # an empty mesh: header only
    empty_v, empty_t = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64)
    ply_case(tmp_path, M, empty_v, empty_t, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), True)
    ply_case(tmp_path, M, empty_v, empty_t, None, None, True)
    with pytest.raises(RuntimeError):
        M.export_ply(str(tmp_path / "bad.ply"), verts, tris, colors=colors[:3])


def test_normals_oracle_against_the_closed_form():
    """v = R - |x - c|: the normal -grad v / |grad v| is the radial direction (x - c) / |x - c|.  Discretisation error of the
    oracle's gradient, with r_min = R - 2.5 the smallest radius of a lattice point it reads (a vertex lies within ~0.1 of the
    sphere, its cell corner within 1 of it, the differences reach 1 further): every third derivative of |x| is at most 3 /
    r^2 in magnitude (those along one axis 1.16 / r^2), so a central difference at spacing 1 is off by at most 1.16 / (6
    r_min^2) and the linear interpolation of the gradient along an edge by at most 3 / (8 r_min^2) per component, 0.57 /
    r_min^2 together, sqrt(3) times that as a vector, and normalising two vectors of length ~1 at most doubles their distance:
    2 / r_min^2.  Measured: 2.7e-3 against the bound 5.6e-2 at R = 8.5 (float64 and float32 alike)."""
    n, R = 24, 8.5
    c = np.array([11.3, 12.1, 11.7])
    ax = np.arange(n, dtype=np.float64)
    x = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1)
    vol = (R - np.linalg.norm(x - c, axis=-1)).astype(np.float32)
    verts, tris = O.marching_cubes(vol, 0.0)
    assert len(verts) > 500
    radial = verts.astype(np.float64) - c
    radial /= np.linalg.norm(radial, axis=1, keepdims=True)
    bound = 2.0 / (R - 2.5) ** 2
    for dtype in (np.float64, np.float32):
        got = N.normals(vol, verts, dtype=dtype)
        assert got.dtype == dtype
        err = float(np.abs(got.astype(np.float64) - radial).max())
        print(f"normals oracle ({dtype.__name__}) vs the radial direction on {len(verts)} vertices: max error {err:.2e} (bound {bound:.2e})")
        assert err <= bound
        assert np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1).max() < 1e-6


def test_normals_oracle_contract_details():
    """Ties and borders of the contract, on values small enough to check by hand."""
    vol = np.zeros((3, 3, 3), np.float32)
    vol[2] = 4.0                                                  # v = 0, 0, 4 along axis 0
    # lattice point (1, 1, 1): central difference (4 - 0) / 2 = 2 along axis 0 -> normal -e_0
    # border point (0, 1, 1): one-sided 0 - 0 = 0 -> zero vector;  (2, 1, 1): one-sided 4 - 0 = 4 -> -e_0
    verts = np.array([[1, 1, 1], [0, 1, 1], [2, 1, 1], [1.5, 1, 1], [0.25, 1, 1]], np.float32)
    g = N.gradient_at(vol, verts)
    assert np.array_equal(g[:, 0], np.array([2, 0, 4, 3, 0.5], np.float32)) and not g[:, 1:].any()
    nn = N.normals(vol, verts)
    assert np.array_equal(nn, np.array([[-1, 0, 0], [0, 0, 0], [-1, 0, 0], [-1, 0, 0], [-1, 0, 0]], np.float32))
    # ties go to the lowest axis: (0.5, 0.5, 0) interpolates along axis 0, between (0,0,0) and (1,0,0)
    tie = np.arange(27, dtype=np.float32).reshape(3, 3, 3) ** 2
    a = N.gradient_at(tie, np.array([[0.5, 0.5, 0]], np.float32))
    want = 0.5 * N.gradient_at(tie, np.array([[0, 0, 0]], np.float32)) + 0.5 * N.gradient_at(tie, np.array([[1, 0, 0]], np.float32))
    assert np.array_equal(a, want)
    # clamp_zero: negative values read as 0;  NaN in the volume -> the zero vector
    neg = np.full((3, 3, 3), -2.0, np.float32)
    neg[2] = -7.0
    assert N.normals(neg, verts[:1]).tolist() == [[1, 0, 0]] and N.normals(neg, verts[:1], clamp_zero=True).tolist() == [[0, 0, 0]]
    bad = vol.copy()
    bad[2, 1, 1] = np.nan
    assert N.normals(bad, verts[:1]).tolist() == [[0, 0, 0]]


FIXTURES = (("ball", False), ("noncubic", False), ("boundary", False), ("noise", False), ("noise", True))


def test_normals_fixture_list_and_tolerance():
    """The float32-vs-float64 gap of the oracle on the GPU test's fixtures (what its fixed tolerance is 4x of) and the share
    of vertices the comparison leaves out (float64 |g| <= 1e-3 of the volume's value range): at most 1 % of any fixture."""
    import test_gpu_mesh_color as G
    worst = 0.0
    for name, clamp in FIXTURES:
        vol, verts, keep, gap = G.normals_case(name, clamp)
        out = 1.0 - keep.mean()
        print(f"{name} clamp={clamp}: V {len(verts)}, float32-float64 gap {gap:.3e}, left out {100 * out:.2f} %")
        assert out <= 0.01
        worst = max(worst, gap)
    print(f"largest gap {worst:.3e}; 4x = {4 * worst:.3e}; the GPU test's tolerance {G.NORMALS_TOL:.3e}")
    assert 4 * worst <= G.NORMALS_TOL <= 4 * worst * 1.01         # the committed figure is the measured one, rounded up
