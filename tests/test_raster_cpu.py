"""CPU-side checks (-m "not gpu") of the rasterizer: the library's exports, ABI version and ctypes prototypes; the refusals the
entries make on the host before any launch; the properties of the numpy oracle the GPU tests compare with (tests/raster_oracle.py:
a mesh with shared edges partitions the plane, winding does not matter); the host camera helpers against the reference's outputs
(tests/golden/u_camera_paths.npz, written by tests/golden/gen_camera_paths.py).  None of it touches a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import raster_oracle as RO

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW_SYMBOLS = ("mf_project_vertices", "mf_raster_scratch_bytes", "mf_rasterize", "mf_raster_resolve", "mf_raster_interpolate",
               "mf_raster_shade")


def test_library_exports_header_symbols_and_prototypes():
    import moco_flow_amd as M
    import moco_flow_amd._lib as L
    from moco_flow_amd import raster
    header = open(os.path.join(ROOT, "include", "mocoflow_hip.h")).read()
    declared = set(re.findall(r"^int(?:32|64)_t (mf_\w+)\(", header, re.M))
    lib = L.lib()
    assert lib.mf_version() == 16 and L.MF_ABI_VERSION == 16
    assert "#define MF_ABI_VERSION 16" in header
    listed = " ".join(header.split("additive entries since")[1].split("*/")[0].split())
    for name in NEW_SYMBOLS:
        assert name in declared and name in L.SYMBOLS, name
        fn = getattr(lib, name)
        assert fn.restype is L.SYMBOLS[name][0] and list(fn.argtypes) == L.SYMBOLS[name][1]
        assert name.replace("mf_raster_scratch_bytes", "mf_rasterize") in listed, name
        # each entry's comment cites the reference lines it serves
        comment = header.split(name + "(")[0].rsplit("/*", 1)[1]
        assert "data_utils.py:23-86, 273-336" in comment and "camera.py:29-81" in comment, name
    assert {n for n in declared if n.startswith(("mf_raster", "mf_project_"))} == set(NEW_SYMBOLS)
    i64, i32, p, f = C.c_int64, C.c_int32, C.c_void_p, C.c_float
    assert L.SYMBOLS["mf_project_vertices"] == (i32, [p, i64, C.POINTER(f), f, f, f, f, p, p, p, p])
    assert L.SYMBOLS["mf_raster_scratch_bytes"] == (i64, [i64, i64])
    assert L.SYMBOLS["mf_rasterize"] == (i32, [p, p, i64, p, i64, i64, i64, f, p, p])
    assert L.SYMBOLS["mf_raster_resolve"] == (i32, [p, p, p, i64, p, i64, i64, i64, f, p, p, p, p, p])
    assert L.SYMBOLS["mf_raster_interpolate"] == (i32, [p, i64, i32, p, i64, p, p, i64, p, p])
    # the struct travels field for field as the header lays it out (a 64-bit build: 208 bytes)
    fields = re.search(r"typedef struct mf_raster_shade_args \{(.*?)\} mf_raster_shade_args;", header, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = [re.sub(r"\[\d+\]", "", d.split()[-1].lstrip("*")) for part in fields.split(";") for d in part.split(",") if d.strip()]
    assert names == [n for n, _ in L.mf_raster_shade_args._fields_]
    assert C.sizeof(L.mf_raster_shade_args) == 208
    for name in ("raster", "project_vertices", "rasterize", "interpolate", "render_mesh", "smpl_views"):
        assert name in M.__all__ and hasattr(M, name)
    assert M.render_mesh is raster.render_mesh
    assert "mf_raster.hip" in open(os.path.join(ROOT, "moco_flow_amd", "csrc", "Makefile")).read()


def test_host_side_refusals_before_any_launch():
    """Null buffers, sizes, the 2^31 limits, pixel_offset and C are settled on the host: the fake pointers are never touched."""
    import moco_flow_amd._lib as L
    lib = L.lib()
    fake = C.c_void_p(256)
    big = 1 << 31
    eye = (C.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    err = lambda: lib.mf_last_error()
    assert lib.mf_raster_scratch_bytes(45, 61) == 45 * 61 * 8 + 8
    for H, W in ((0, 4), (4, 0), (-1, 4), (4, -3), (1 << 16, 1 << 15), (big, 1), (3, big)):
        assert lib.mf_raster_scratch_bytes(H, W) == -1
        assert lib.mf_rasterize(fake, fake, 4, fake, 4, H, W, 0.0, fake, None) == -1
        assert (b"positive" in err()) if min(H, W) <= 0 else (b"2^31" in err())
        assert lib.mf_raster_resolve(fake, fake, fake, 4, fake, 4, H, W, 0.0, fake, fake, fake, None, None) == -1
    assert lib.mf_raster_scratch_bytes(1 << 15, (1 << 16) - 1) == ((1 << 31) - (1 << 15)) * 8 + 8
    for V, T in ((4, big), (big, 4), (-1, 4), (4, -1)):
        assert lib.mf_rasterize(fake, fake, V, fake, T, 8, 8, 0.0, fake, None) == -1 and b"2^31" in err()
        assert lib.mf_raster_resolve(fake, fake, fake, V, fake, T, 8, 8, 0.0, fake, fake, fake, None, None) == -1 and b"2^31" in err()
        assert lib.mf_raster_interpolate(fake, V, 3, fake, T, fake, fake, 64, fake, None) == -1 and b"2^31" in err()
    for off in (0.25, -0.5, 1.0, float("nan")):
        assert lib.mf_rasterize(fake, fake, 4, fake, 4, 8, 8, off, fake, None) == -1 and b"pixel_offset" in err()
        assert lib.mf_raster_resolve(fake, fake, fake, 4, fake, 4, 8, 8, off, fake, fake, fake, None, None) == -1 and b"pixel_offset" in err()
    assert lib.mf_rasterize(fake, fake, 4, fake, 4, 8, 8, 0.0, None, None) == -1 and b"scratch" in err()
    assert lib.mf_rasterize(fake, fake, 4, None, 4, 8, 8, 0.5, fake, None) == -1 and b"tris" in err()
    assert lib.mf_rasterize(None, fake, 4, fake, 4, 8, 8, 0.0, fake, None) == -1 and b"screen" in err()
    assert lib.mf_rasterize(fake, None, 4, fake, 4, 8, 8, 0.0, fake, None) == -1 and b"inv_z" in err()
    assert lib.mf_raster_resolve(fake, fake, fake, 4, fake, 4, 8, 8, 0.0, None, None, None, None, None) == -1 and b"output" in err()
    assert lib.mf_raster_resolve(None, fake, fake, 4, fake, 4, 8, 8, 0.0, fake, fake, fake, None, None) == -1 and b"scratch" in err()
    for Cn in (0, 17, -2):
        assert lib.mf_raster_interpolate(fake, 4, Cn, fake, 4, fake, fake, 64, fake, None) == -1 and b"C=" in err()
    assert lib.mf_raster_interpolate(fake, 4, 3, fake, 4, None, fake, 64, fake, None) == -1 and b"null" in err()
    assert lib.mf_raster_interpolate(None, 4, 3, fake, 4, fake, fake, 64, fake, None) == -1 and b"null" in err()
    assert lib.mf_raster_interpolate(fake, 4, 3, fake, 4, fake, fake, big, fake, None) == -1 and b"n_pix" in err()
    assert lib.mf_raster_interpolate(None, 4, 3, None, 4, None, None, 0, None, None) == 0
    assert lib.mf_project_vertices(fake, big, eye, 60.0, 4.0, 4.0, 1e-3, fake, fake, None, None) == -1 and b"2^31" in err()
    assert lib.mf_project_vertices(fake, 4, None, 60.0, 4.0, 4.0, 1e-3, fake, fake, None, None) == -1 and b"c2w" in err()
    assert lib.mf_project_vertices(fake, 4, eye, 0.0, 4.0, 4.0, 1e-3, fake, fake, None, None) == -1 and b"focal" in err()
    assert lib.mf_project_vertices(fake, 4, eye, 60.0, 4.0, 4.0, 0.0, fake, fake, None, None) == -1 and b"znear" in err()
    assert lib.mf_project_vertices(None, 4, eye, 60.0, 4.0, 4.0, 1e-3, fake, fake, None, None) == -1 and b"null" in err()
    assert lib.mf_project_vertices(fake, 4, eye, 60.0, 4.0, 4.0, 1e-3, None, fake, None, None) == -1 and b"null" in err()
    assert lib.mf_project_vertices(None, 0, eye, 60.0, 4.0, 4.0, 1e-3, None, None, None, None) == 0
    a = L.mf_raster_shade_args()
    assert lib.mf_raster_shade(None, None) == -1
    a.scratch = a.screen = a.inv_z = a.tris = a.rgba = 256
    a.V = a.T = 4
    a.H = a.W = 8
    a.focal = 60.0
    for bad, word in (("H", b"positive"), ("W", b"positive")):
        setattr(a, bad, 0)
        assert lib.mf_raster_shade(C.byref(a), None) == -1 and word in err()
        setattr(a, bad, 8)
    a.pixel_offset = 0.75
    assert lib.mf_raster_shade(C.byref(a), None) == -1 and b"pixel_offset" in err()
    a.pixel_offset = 0.5
    a.shading = 2
    assert lib.mf_raster_shade(C.byref(a), None) == -1 and b"shading" in err()
    a.shading = L.MF_RASTER_SHADE_HEADLIGHT
    assert lib.mf_raster_shade(C.byref(a), None) == -1 and b"verts" in err()
    a.shading = L.MF_RASTER_SHADE_NONE
    a.background_kind = 3
    assert lib.mf_raster_shade(C.byref(a), None) == -1 and b"background_kind" in err()
    a.background_kind = L.MF_RASTER_BG_IMAGE
    assert lib.mf_raster_shade(C.byref(a), None) == -1 and b"background_image" in err()
    a.background_kind = L.MF_RASTER_BG_NONE
    a.rgba = 258
    assert lib.mf_raster_shade(C.byref(a), None) == -1 and b"aligned" in err()
    a.rgba = None
    assert lib.mf_raster_shade(C.byref(a), None) == -1 and b"output" in err()
    a.rgba, a.focal = 256, 0.0
    assert lib.mf_raster_shade(C.byref(a), None) == -1 and b"focal" in err()


def test_argument_validation_needs_no_gpu():
    import moco_flow_amd as M
    R = M.raster
    verts, tris = torch.zeros(5, 3), torch.zeros(4, 3, dtype=torch.int64)
    eye = np.eye(4)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        R.project_vertices(verts, eye, 60.0, (4, 4))
    with pytest.raises(RuntimeError, match=r"\(N, 3\)"):
        R.project_vertices(torch.zeros(5, 2), eye, 60.0, (4, 4))
    with pytest.raises(RuntimeError, match="floating-point"):
        R.project_vertices(torch.zeros(5, 3, dtype=torch.int64), eye, 60.0, (4, 4))
    with pytest.raises(RuntimeError, match="int32 tensor of project_vertices"):
        R.rasterize(torch.zeros(5, 2), torch.zeros(5), tris, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        R.rasterize(torch.zeros(5, 2, dtype=torch.int32), torch.zeros(5), tris, 8, 8)
    for off in (0.25, 1, -0.5, "0.5"):
        with pytest.raises(RuntimeError, match="pixel_offset"):
            R.rasterize(torch.zeros(5, 2, dtype=torch.int32), torch.zeros(5), tris, 8, 8, pixel_offset=off)
        with pytest.raises(RuntimeError, match="pixel_offset"):
            R.render_mesh(verts, tris, None, 8, 8, 60.0, (4, 4), eye, pixel_offset=off)
    for H, W in ((0, 8), (8, -1), (1 << 16, 1 << 15)):
        with pytest.raises(RuntimeError, match="H W < 2\\^31"):
            R.rasterize(torch.zeros(5, 2, dtype=torch.int32), torch.zeros(5), tris, H, W)
        with pytest.raises(RuntimeError, match="H W < 2\\^31"):
            R.render_mesh(verts, tris, None, H, W, 60.0, (4, 4), eye)
    with pytest.raises(RuntimeError, match="shading"):
        R.render_mesh(verts, tris, None, 8, 8, 60.0, (4, 4), eye, shading="phong")
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        R.render_mesh(verts, tris, None, 8, 8, 60.0, (4, 4), eye)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        R.interpolate(torch.zeros(5, 3), tris, torch.zeros(8, 8, dtype=torch.int32), torch.zeros(8, 8, 3))
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        next(R.smpl_views(verts, tris, 2, 8, 8, 60.0, (4, 4)))
    assert R.quantise([0.0, 1.0, 0.5, 0.25, -1.0, 2.0]).tolist() == [0, 255, 128, 64, 0, 255]


# ---- the oracle's own properties ----
def _random_planar_mesh(seed, H, W):
    """A grid over more than the viewport whose inner vertices are jittered onto random 1/256 positions -- and a few of them
    exactly onto samples, so that edges and vertices pass through samples."""
    rng = np.random.default_rng(seed)
    pts, tris = RO.grid_mesh(6, 5, x0=-3.0, y0=-2.5, dx=(W + 6) / 6, dy=(H + 5) / 5)
    inner = (pts[:, 0] > -3.0) & (pts[:, 0] < W + 3 - 1e-9) & (pts[:, 1] > -2.5) & (pts[:, 1] < H + 2.5 - 1e-9)
    pts[inner] += rng.uniform(-0.9, 0.9, (int(inner.sum()), 2))
    screen = RO.snap(pts)
    on_sample = rng.random(len(pts)) < 0.5
    screen[inner & on_sample] = screen[inner & on_sample] // 256 * 256
    return screen, tris


@pytest.mark.parametrize("off", [0, 128])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_oracle_shared_edge_mesh_partitions_the_plane(seed, off):
    H, W = 13, 17
    screen, tris = _random_planar_mesh(seed, H, W)
    _, sgn = RO.tri_status(screen, tris, len(screen))
    assert (sgn != 0).all() and len(set(sgn.tolist())) == 1              # the jitter folded nothing over
    e, cov = RO.coverage(screen, tris, H, W, off)
    assert (cov.sum(axis=0) == 1).all()                                  # every sample: exactly one triangle
    assert ((e == 0).any(axis=-1) & cov).sum() > 0 or off == 128         # ... also where an edge passes through a sample


def test_oracle_exact_grid_and_fan_cover_each_sample_once():
    # vertices exactly on samples: every edge of the grid passes through samples
    pts, tris = RO.grid_mesh(4, 3, x0=1.0, y0=2.0, dx=3.0, dy=2.0)
    e, cov = RO.coverage(RO.snap(pts), tris, 11, 16)
    inside = np.zeros((11, 16), bool)
    inside[2:8, 1:13] = True                                             # [x0, x0 + 12) x [y0, y0 + 6): top-left owns its edges
    assert np.array_equal(cov.sum(axis=0), inside.astype(int))
    assert ((e == 0).any(axis=-1) & cov).sum() >= 30
    # a fan around a vertex on a sample
    ang = np.linspace(0, 2 * np.pi, 8)[:-1] + 0.1
    ring = np.stack([4 + 3.3 * np.cos(ang), 4 + 3.1 * np.sin(ang)], axis=1)
    pts = np.concatenate([[[4.0, 4.0]], ring])
    fan = np.array([[0, 1 + k, 1 + (k + 1) % 7] for k in range(7)], dtype=np.int64)
    _, cov = RO.coverage(RO.snap(pts), fan, 9, 9)
    assert cov[:, 4, 4].sum() == 1 and cov.sum(axis=0).max() == 1 and cov.sum() > 20


def test_oracle_winding_and_order_do_not_matter():
    screen, tris = _random_planar_mesh(5, 13, 17)
    rng = np.random.default_rng(0)
    inv_z = rng.uniform(0.2, 2.0, len(screen))
    flipped = tris[:, ::-1].copy()
    mixed = np.where((np.arange(len(tris)) % 2 == 0)[:, None], tris, flipped)
    e0, c0 = RO.coverage(screen, tris, 13, 17)
    for other in (flipped, mixed):
        _, c1 = RO.coverage(screen, other, 13, 17)
        assert np.array_equal(c0, c1)
    f0, d0, b0, _ = RO.rasterize(screen, inv_z, tris, 13, 17)
    f1, d1, b1, _ = RO.rasterize(screen, inv_z, flipped, 13, 17)
    assert np.array_equal(f0, f1)
    assert np.allclose(d0, d1, rtol=1e-14, atol=0)                       # (the sum of three products runs in the other order)
    assert np.allclose(b0, b1[..., ::-1], rtol=1e-14, atol=1e-16)        # the weights follow their vertices
    assert np.allclose(b0.sum(axis=-1), 1) and (b0 >= 0).all()
    # zero-area triangles and slivers between samples cover nothing
    screen = np.array([[256, 256], [1024, 1024], [640, 640], [300, 300], [400, 310], [500, 300]], dtype=np.int64)
    _, cov = RO.coverage(screen, np.array([[0, 1, 2], [0, 0, 1], [3, 4, 5]]), 8, 8)
    assert not cov.any()


def test_oracle_depth_is_the_plane_seen_along_the_ray():
    """The perspective-correct depth of the oracle is the camera-axis z of the point where the pixel's ray meets the
    triangle's plane -- for the UNsnapped projection; here the vertices project exactly onto 1/256 positions."""
    f, cx, cy = 64.0, 8.0, 6.0
    sx = np.array([[2.0, 1.0], [14.5, 3.25], [6.75, 11.5]])
    z = np.array([2.0, 4.0, 1.0])
    verts = np.stack([(sx[:, 0] - cx) / f * z, -(sx[:, 1] - cy) / f * z, -z], axis=1)
    x, y, inv_z, ok = RO.project(verts, np.eye(4), f, cx, cy)
    assert ok.all() and np.array_equal(RO.snap(np.stack([x, y], 1)), (sx * 256).astype(np.int64))
    face, depth, bary, _ = RO.rasterize(RO.snap(np.stack([x, y], 1)), inv_z, [[0, 1, 2]], 12, 16)
    hit = face >= 0
    assert hit.sum() > 30
    jj, ii = np.nonzero(hit)
    d = np.stack([(ii - cx) / f, -(jj - cy) / f, -np.ones(len(ii))], axis=1)
    n = np.cross(verts[1] - verts[0], verts[2] - verts[0])
    t = (n @ verts[0]) / (d @ n)                                         # the ray o + t d with d.z = -1: z = t
    assert np.allclose(depth[hit], t, rtol=1e-12)
    assert np.allclose(np.einsum("nk,kc->nc", bary[hit], verts), d * t[:, None], atol=1e-12)


# ---- the camera helpers against the reference's outputs ----
GOLD = np.load(os.path.join(HERE, "golden", "u_camera_paths.npz"))
EPS64, EPS32 = np.finfo(np.float64).eps, np.finfo(np.float32).eps


def test_sample_on_sphere_matches_the_reference():
    from moco_flow_amd import camera
    for k, (n, dist, half) in enumerate(GOLD["sphere_args"]):
        want = GOLD[f"sphere_{k}"]
        got = camera.sample_on_sphere(int(n), dist, bool(half))
        assert got.shape == want.shape == (int(n), 3) and got.dtype == np.float64
        # the same float64 formula; numpy's vector and scalar cos / sin may differ in the last place
        assert np.abs(got - want).max() <= 8 * EPS64 * dist
        assert np.allclose(np.linalg.norm(got, axis=1), dist, rtol=1e-12)
        if half:
            assert (got[:, 1] >= 0).all()


def test_look_at_pose_matches_the_reference():
    from moco_flow_amd import camera
    target = GOLD["pose_target"]
    for pos, want in zip(GOLD["pose_positions"], GOLD["pose_out"]):
        got = camera.look_at_pose(pos, target)
        assert got.shape == (4, 4) and np.abs(got - want).max() <= 8 * EPS64 * max(1.0, np.abs(pos).max())
        Rm = got[:3, :3]
        if abs(Rm[2, 2]) < 0.999:                                        # (the pole branch keeps x = (1, 0, 0): not orthogonal off the pole)
            assert np.allclose(Rm.T @ Rm, np.eye(3), atol=1e-12) and np.linalg.det(Rm) > 0
        to_target = (target - pos) / np.linalg.norm(target - pos)
        assert np.allclose(-Rm[:, 2], to_target, atol=1e-12)             # the camera looks down -z through the target
    assert np.array_equal(camera.look_at_pose(target + [0, 0, 2.0], target)[:3, 0], [1, 0, 0])     # the pole branch


def test_spheric_poses_match_the_reference():
    from moco_flow_amd import camera
    for k, row in enumerate(GOLD["turn_args"]):
        n, radius, center, up, has_up = int(row[0]), row[1], row[2:5].tolist(), row[5:8], bool(row[8])
        want = GOLD[f"turn_{k}"]
        got = camera.spheric_poses(n, radius, center, up if has_up else None)
        assert got.shape == want.shape == (3 * n, 4, 4) and got.dtype == np.float32
        # float32 matrices multiplied in the same order: a few units in the last place of the largest entry
        assert np.abs(got.astype(np.float64) - want).max() <= 8 * EPS32 * (radius + np.abs(center).max() + 1)
        dist = np.linalg.norm(got[:, :3, 3].astype(np.float64) - np.asarray(center), axis=1)
        if not has_up:                                                   # (the up-vector frame is orthonormal only for u.x = 0)
            assert np.allclose(dist, radius, rtol=1e-5)
