"""GPU tests of the rasterizer (moco_flow_amd.raster; csrc/mf_raster.hip) against the numpy oracle of its contract
(tests/raster_oracle.py).  Viewports are tiny and awkward on purpose: 45 x 61, 8 x 8 and one 37 x 130.

Bars.  Coverage and face ids are bit-exact (integers).  Floating-point outputs follow the project's yardstick: the kernel's error
against the float64 oracle may be at most 4 x the error of a numpy-fp32 restatement of the same formula against float64, on the
same inputs (4: division and the transform may associate differently).  Figures measured on an MI355X (kernel / numpy-fp32):
    projection   position 7.538e-06 / 7.538e-06 pixel, inv_z 1.429e-07 / 1.429e-07 relative
    visibility   depth 1.637e-07 / 1.637e-07 relative, bary 7.837e-08 / 7.837e-08; 2246 covered pixels, none excluded (no pixel
                 has its two nearest depths within 1e-5 relative), no face mismatch
    rays         |o + ray_t d - sum bary_k v_k| at most 0.728 of the snapping bound (largest gap 1.47e-04 world units)
    headlight    0 of 6285 bytes differ from float64 (1 LSB is allowed)"""
import functools

import numpy as np
import pytest
import torch

import raster_oracle as RO

pytestmark = pytest.mark.gpu
EPS32 = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def R():
    from moco_flow_amd import raster
    return raster


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def device_raster(R, screen, inv_z, tris, H, W, off=0.0, dropped=False):
    out = R.rasterize(dev(screen, torch.int32), dev(inv_z, torch.float32), dev(np.asarray(tris, np.int64).reshape(-1, 3)), H, W,
                      pixel_offset=off, return_dropped=dropped)
    return tuple(o.cpu().numpy() if isinstance(o, torch.Tensor) else o for o in out)


def yardstick(name, got, want64, ref32, relative):
    """print both errors, then hold the kernel to 4 x the numpy-fp32 restatement's"""
    want64 = np.asarray(want64, np.float64)
    scale = np.abs(want64) if relative else 1.0
    e_dev = float(np.max(np.abs(np.asarray(got, np.float64) - want64) / scale))
    e_ref = float(np.max(np.abs(np.asarray(ref32, np.float64) - want64) / scale))
    print(f"{name}: kernel {e_dev:.3e}  numpy-fp32 {e_ref:.3e}  ({'relative' if relative else 'absolute'}, against float64)")
    assert e_dev <= 4 * e_ref, (name, e_dev, e_ref)
    return e_dev, e_ref


# ---- projection ----
@functools.lru_cache(maxsize=None)
def projection_case():
    from moco_flow_amd import camera
    rng = np.random.default_rng(7)
    c2w = camera.look_at_pose([1.2, -2.0, 1.5], [0.1, 0.2, -0.1])
    verts = rng.uniform(-1, 1, (1000, 3)).astype(np.float32)
    verts[::50] = (c2w[:3, 3] + c2w[:3, 2] * rng.uniform(0.5, 2, (20, 1))).astype(np.float32)      # behind the camera
    verts[7] = c2w[:3, 3].astype(np.float32)                                                        # at the camera: z = 0
    return verts, c2w, 60.0, 30.5, 22.5


def test_projection_against_float64(R):
    verts, c2w, f, cx, cy = projection_case()
    screen, inv_z, xy = (t.cpu().numpy() for t in R.project_vertices(dev(verts), c2w, f, (cx, cy), return_xy=True))
    x64, y64, w64, ok64 = RO.project(verts, c2w, f, cx, cy)
    x32, y32, w32, ok32 = RO.project(verts, c2w, f, cx, cy, dtype=np.float32)
    ok = inv_z > 0
    assert np.array_equal(ok, ok64) and np.array_equal(ok, ok32) and (~ok).sum() == 21
    assert (screen[~ok] == R.BEHIND).all() and (inv_z[~ok] == 0).all() and np.isnan(xy[~ok]).all()
    yardstick("projection x, y [pixel]", xy[ok], np.stack([x64, y64], 1)[ok], np.stack([x32, y32], 1)[ok], relative=False)
    yardstick("projection inv_z", inv_z[ok], w64[ok], w32[ok], relative=True)


def test_snapped_coordinates_are_rint_of_the_devices_own_positions(R):
    verts, c2w, f, cx, cy = projection_case()
    screen, inv_z, xy = R.project_vertices(dev(verts), c2w, f, (cx, cy), return_xy=True)
    ok = inv_z > 0
    want = torch.round(xy[ok] * 256).to(torch.int32)                     # torch.round: ties to even, as rintf; 256 x is exact
    assert torch.equal(screen[ok], want)
    assert (screen[ok].abs() < 2 ** 23).all()
    # znear is a keyword: a larger one flags more vertices
    far = R.project_vertices(dev(verts), c2w, f, (cx, cy), znear=2.0)[1]
    assert int((far > 0).sum()) < int(ok.sum()) and bool((far[far > 0] < 0.5).all())


# ---- coverage and face ids, bit-exact ----
def check_faces(R, screen, inv_z, tris, H, W, off=0.0):
    face, depth, bary = device_raster(R, screen, inv_z, tris, H, W, off)
    want, d64, b64, _ = RO.rasterize(screen, inv_z, tris, H, W, int(off * 256))
    assert torch.equal(torch.from_numpy(face), torch.from_numpy(want))
    hit = want >= 0
    assert np.isposinf(depth[~hit]).all() and (bary[~hit] == 0).all()
    if hit.any():
        assert np.allclose(depth[hit], d64[hit], rtol=1e-5) and np.allclose(bary[hit], b64[hit], atol=1e-5)
    return want


def layered_triangles(T, H, W, seed):
    """T triangles with their own vertices, triangle t in its own depth layer (layers 1 % apart: fp32 and float64 order alike);
    small and large, inside, straddling every viewport edge and outside; corners on random 1/256 positions, every fourth
    triangle with a corner exactly on a sample."""
    rng = np.random.default_rng(seed)
    centre = rng.uniform([-6, -6], [W + 6, H + 6], (T, 1, 2))
    size = rng.choice([0.4, 1.5, 4.0, 12.0], (T, 1, 1))
    pts = centre + rng.uniform(-1, 1, (T, 3, 2)) * size
    screen = RO.snap(pts.reshape(-1, 2))
    screen[::12] = screen[::12] // 256 * 256
    layer = rng.permutation(T)
    inv_z = np.repeat(1.0 / (1.0 + 0.01 * layer), 3)
    return screen, inv_z, np.arange(3 * T, dtype=np.int64).reshape(T, 3)


@pytest.mark.parametrize("off", [0.0, 0.5])
@pytest.mark.parametrize("T", [1, 63, 64, 65, 641])
def test_triangle_lists(R, T, off):
    screen, inv_z, tris = layered_triangles(T, 45, 61, T)
    want = check_faces(R, screen, inv_z, tris, 45, 61, off)
    if T >= 63:
        assert len(np.unique(want)) > min(T, 100) // 3


@pytest.mark.parametrize("off", [0.0, 0.5])
@pytest.mark.parametrize("flip", [False, True])
def test_grid_mesh_with_vertices_on_samples(R, flip, off):
    pts, tris = RO.grid_mesh(7, 6, x0=-4.0, y0=-3.0, dx=10.0, dy=9.0, flip=flip)           # edges pass through samples at offset 0
    screen = RO.snap(pts)
    want = check_faces(R, screen, np.full(len(pts), 0.5), tris, 45, 61, off)
    assert (want >= 0).all() and len(np.unique(want)) > 40                                  # every sample exactly once
    mixed = np.where((np.arange(len(tris)) % 3 == 0)[:, None], tris[:, ::-1], tris)
    assert np.array_equal(check_faces(R, screen, np.full(len(pts), 0.5), mixed, 45, 61, off), want)


def test_fan_around_a_vertex_on_a_sample(R):
    ang = np.linspace(0, 2 * np.pi, 8)[:-1] + 0.1
    pts = np.concatenate([[[4.0, 4.0]], np.stack([4 + 3.3 * np.cos(ang), 4 + 3.1 * np.sin(ang)], axis=1)])
    fan = np.array([[0, 1 + k, 1 + (k + 1) % 7] for k in range(7)], dtype=np.int64)
    want = check_faces(R, RO.snap(pts), np.linspace(0.3, 0.9, 8), fan, 8, 8)
    assert want[4, 4] >= 0 and (want >= 0).sum() > 20


def test_empty_meshes(R):
    none = np.zeros((0, 3), np.int64)
    for screen, inv_z, tris in ((np.zeros((0, 2)), np.zeros(0), none), (np.zeros((3, 2)), np.ones(3), none),
                                (np.zeros((0, 2)), np.zeros(0), np.array([[0, 1, 2], [3, 4, 5]]))):
        face, depth, bary, dropped = device_raster(R, screen, inv_z, tris, 8, 8, dropped=True)
        assert (face == -1).all() and np.isposinf(depth).all() and (bary == 0).all()
        assert dropped == (len(tris) if len(screen) == 0 else 0)                          # V = 0: every index is out of range
    out = R.render_mesh(torch.zeros((0, 3), device="cuda"), dev(none), None, 8, 8, 60.0, (4, 4), np.eye(4), background=(1, 0, 0))
    assert not out["mask"].any() and (out["face"] == -1).all()
    assert out["rgba"].reshape(-1, 4).unique(dim=0).tolist() == [[255, 0, 0, 0]]


def test_duplicates_slivers_and_zero_area(R):
    tri = RO.snap(np.array([[1.3, 0.7], [7.6, 2.2], [3.1, 7.4]]))
    # 70 copies of one triangle (across a wave's 64): an exact depth tie goes to the lowest index
    face, depth, bary = device_raster(R, np.tile(tri, (70, 1)), np.tile([0.5, 0.25, 1.0], 70), np.arange(210).reshape(70, 3), 8, 8)
    want, *_ = RO.rasterize(tri, [0.5, 0.25, 1.0], [[0, 1, 2]], 8, 8)
    assert np.array_equal(face, want) and set(np.unique(face)) == {-1, 0} and (face == 0).sum() > 10
    # the same with the copies in front of it in the list but behind it in depth
    inv_z = np.concatenate([np.tile([0.4, 0.2, 0.8], 69), [0.5, 0.25, 1.0]])
    face2, depth2, _ = device_raster(R, np.tile(tri, (70, 1)), inv_z, np.arange(210).reshape(70, 3), 8, 8)
    assert np.array_equal(face2 >= 0, face >= 0) and (face2[face2 >= 0] == 69).all() and np.array_equal(depth2, depth)
    # slivers between samples and zero-area triangles (collinear, repeated vertex, a point) cover nothing
    screen = np.array([[300, 300], [1500, 310], [900, 400], [256, 256], [1024, 1024], [640, 640], [512, 512]], dtype=np.int64)
    tris = np.array([[0, 1, 2], [3, 4, 5], [3, 3, 4], [6, 6, 6], [4, 3, 5]])
    face, _, _, dropped = device_raster(R, screen, np.ones(7), tris, 8, 8, dropped=True)
    assert (face == -1).all() and dropped == 0
    assert not RO.coverage(screen, tris, 8, 8)[1].any()


@pytest.mark.parametrize("off", [0.0, 0.5])
def test_triangles_straddling_and_outside_the_viewport(R, off):
    H, W = 45, 61
    pts = np.array([[-5.2, 10.1], [4.3, 3.2], [3.9, 30.7],            # left edge
                    [55.5, 5.5], [70.1, 20.2], [50.3, 40.4],            # right edge
                    [10.2, -7.7], [40.4, -3.3], [25.5, 6.6],            # top edge
                    [12.1, 40.2], [30.3, 60.6], [45.4, 38.8],           # bottom edge
                    [-9.0, -9.0], [5.5, -2.0], [-3.0, 6.5],             # the corner (0, 0)
                    [-30.0, 5.0], [-2.0, 9.0], [-12.0, 30.0],           # outside: left of it
                    [62.0, 1.0], [90.0, 3.0], [70.0, 44.0],             # right of it
                    [5.0, 45.5], [50.0, 46.0], [20.0, 80.0],            # below it
                    [1.0, -40.0], [60.0, -1.5], [30.0, -0.25],          # above it
                    [-200.0, -300.0], [400.0, -250.0], [10.0, 500.0]])  # around all of it
    tris = np.arange(30).reshape(10, 3)
    inv_z = np.repeat(1.0 / (1.0 + 0.05 * np.arange(10)), 3)
    want = check_faces(R, RO.snap(pts), inv_z, tris, H, W, off)
    assert set(np.unique(want)) == {0, 1, 2, 3, 4, 9}
    # beyond the guard band of 2^15 pixels: dropped whole and counted, like an index out of range
    far = RO.snap(np.array([[1.0, 1.0], [40000.0, 2.0], [3.0, 30.0], [9.0, 9.0], [30.0, 12.0], [12.0, 30.0]]))
    face, _, _, dropped = device_raster(R, far, np.ones(6), [[0, 1, 2], [3, 4, 5], [3, 4, 6], [-1, 4, 5]], H, W, off, dropped=True)
    assert dropped == 3 and set(np.unique(face)) == {-1, 1}


def test_triangles_behind_the_camera_are_dropped_and_counted(R):
    v1, t1 = RO.icosphere(1, 1.0, (0, 0, -0.2))                          # the camera sits inside it, near the front
    v2, t2 = RO.icosphere(1, 0.1, (0.05, 0, -0.6))                       # a small one inside it, in front of its far side
    verts, tris = np.concatenate([v1, v2]).astype(np.float32), np.concatenate([t1, t2 + len(v1)])
    H, W, f, c = 45, 61, 60.0, (30.5, 22.5)
    screen, inv_z = R.project_vertices(dev(verts), np.eye(4), f, c)
    face, depth, bary, dropped = R.rasterize(screen, inv_z, dev(tris), H, W, return_dropped=True)
    sc, w = screen.cpu().numpy(), inv_z.cpu().numpy()
    drop, _ = RO.tri_status(sc, tris, len(verts))
    assert dropped == int(drop.sum()) and 0 < dropped < len(t1) and not drop[len(t1):].any()
    want, *_ = RO.rasterize(sc, w, tris, H, W)
    assert torch.equal(face.cpu(), torch.from_numpy(want))
    assert not np.isin(want, np.nonzero(drop)[0]).any() and (want >= len(t1)).sum() > 50


@pytest.mark.parametrize("off", [0.0, 0.5])
def test_one_triangle_over_the_whole_37_x_130_viewport(R, off):
    screen = RO.snap(np.array([[-10.0, -5.0], [400.0, -6.0], [-12.0, 120.0]]))
    want = check_faces(R, screen, [0.5, 0.1, 0.9], [[0, 1, 2]], 37, 130, off)     # 5 x 17 blocks of 8 x 8: the walk's later trips
    assert (want == 0).all()


# ---- visibility ----
@functools.lru_cache(maxsize=None)
def scene():
    """Two interpenetrating icospheres (320 triangles each) in front of one large triangle; f = 60, 45 x 61."""
    v1, t1 = RO.icosphere(2, 0.5, (0, 0, -2.5))
    v2, t2 = RO.icosphere(2, 0.4, (0.35, 0.1, -2.3))
    big = np.array([[-3, -2, -4], [3, -2, -4], [0, 3, -4.0]])
    verts = np.concatenate([v1, v2, big]).astype(np.float32)
    n = len(v1) + len(v2)
    tris = np.concatenate([t1, t2 + len(v1), [[n, n + 1, n + 2]]])
    assert len(t1) == len(t2) == 320
    return verts, tris, 45, 61, 60.0, (30.5, 22.5), np.eye(4)


@functools.lru_cache(maxsize=None)
def scene_device():
    """The device's projection and rasterization of the scene, and both oracles on the device's own screen and inv_z."""
    from moco_flow_amd import raster as R
    verts, tris, H, W, f, c, c2w = scene()
    screen, inv_z = R.project_vertices(dev(verts), c2w, f, c)
    face, depth, bary = R.rasterize(screen, inv_z, dev(tris), H, W)
    sc, w = screen.cpu().numpy(), inv_z.cpu().numpy()
    o64 = RO.rasterize(sc, w.astype(np.float64), tris, H, W)
    o32 = RO.rasterize(sc, w, tris, H, W, dtype=np.float32)
    return (screen, inv_z), (face, depth, bary), o64, o32


def test_visibility_of_interpenetrating_spheres(R):
    _, (face, depth, bary), (f64, d64, b64, second), (f32, d32, b32, _) = scene_device()
    face, depth, bary = face.cpu().numpy(), depth.cpu().numpy(), bary.cpu().numpy()
    hit = f64 >= 0
    assert np.array_equal(face >= 0, hit)
    with np.errstate(invalid="ignore"):
        close = hit & ((second - d64) < 1e-5 * d64)
    print(f"visibility: {hit.sum()} covered pixels, {close.sum()} excluded (two nearest depths within 1e-5 relative), "
          f"{(face != f64)[hit & ~close].sum()} face mismatches outside them")
    assert hit.sum() > 2000 and close.sum() <= 0.005 * hit.sum()
    assert np.array_equal(face[~close], f64[~close])
    assert len(np.unique(face[hit])) > 150 and (face == 640).sum() > 500
    same = hit & (face == f64) & (f32 == f64)
    yardstick("visibility depth", depth[same], d64[same], d32[same], relative=True)
    yardstick("visibility bary", bary[same], b64[same], b32[same], relative=False)
    assert np.isposinf(depth[~hit]).all() and (bary[~hit] == 0).all()


def test_runs_are_bit_identical_and_order_independent(R):
    verts, tris, H, W, f, c, c2w = scene()
    (screen, inv_z), (face, depth, bary), *_ = scene_device()
    again = R.rasterize(screen, inv_z, dev(tris), H, W)
    for a, b in zip((face, depth, bary), again):
        assert torch.equal(a, b)
    perm = np.random.default_rng(3).permutation(len(tris))
    pf, pd, pb = R.rasterize(screen, inv_z, dev(tris[perm]), H, W)       # triangle k of the new list is perm[k] of the old
    assert torch.equal(pd, depth) and torch.equal(pb, bary)
    lut = torch.cat([dev(perm, torch.int32), torch.tensor([-1], dtype=torch.int32, device="cuda")])
    assert torch.equal(lut[pf.long()], face)


# ---- consistency with the renderer's rays ----
def test_surface_points_lie_on_the_rays_of_make_rays(R):
    from moco_flow_amd import camera
    verts, tris, H, W, f, c, _ = scene()
    c2w = camera.look_at_pose([0.4, -0.3, 0.2], [0.1, 0.0, -2.5])
    out = R.render_mesh(dev(verts), dev(tris), None, H, W, f, c, c2w)
    screen, inv_z = R.project_vertices(dev(verts), c2w, f, c)
    face, depth, bary = (t.cpu().numpy() for t in R.rasterize(screen, inv_z, dev(tris), H, W))
    assert np.array_equal(out["face"].cpu().numpy(), face) and np.array_equal(out["depth"].cpu().numpy(), depth)
    rays = camera.make_rays(H, W, f, c, c2w, 0.1, 10.0, 0.0).cpu().numpy().astype(np.float64)
    ray_t = out["ray_t"].cpu().numpy().astype(np.float64).reshape(-1)
    hit = face.reshape(-1) >= 0
    assert hit.sum() > 1500 and np.isposinf(ray_t[~hit]).all()
    on_ray = rays[hit, 0:3] + ray_t[hit, None] * rays[hit, 3:6]
    tri = verts.astype(np.float64)[tris[face.reshape(-1)[hit]]]                      # (n, 3, 3)
    on_tri = np.einsum("nk,nkc->nc", bary.reshape(-1, 3)[hit].astype(np.float64), tri)
    # The bound, from the contract: both points have the same camera-axis depth z (1 / sum beta_k w_k is the z of sum bary_k v_k);
    # sideways they differ by the snapping of the vertices, at most sqrt(2) / 512 pixel = (sqrt(2) / 512) z / f in the world, plus
    # the rounding of fp32 positions of this size (16 eps |p| covers the dozen operations on either side)
    z = depth.reshape(-1)[hit].astype(np.float64)
    bound = np.sqrt(2) / 512 * z / f + 16 * EPS32 * np.linalg.norm(on_tri - c2w[:3, 3], axis=1)
    gap = np.linalg.norm(on_ray - on_tri, axis=1)
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    off_plane = np.abs(np.einsum("nc,nc->n", on_ray - tri[:, 0], n / np.linalg.norm(n, axis=1, keepdims=True)))
    print(f"rays: |o + ray_t d - sum bary_k v_k| up to {np.max(gap / bound):.3f} of the bound, distance to the plane up to "
          f"{np.max(off_plane / bound):.3f} of it; largest gap {gap.max():.3e}")
    assert (gap <= bound).all() and (off_plane <= bound).all()


# ---- interpolate / render_mesh ----
def scene_colors():
    verts = scene()[0]
    return ((verts - verts.min(0)) / (verts.max(0) - verts.min(0))).astype(np.float32)


def test_interpolate_is_the_oracle_composed_from_face_and_bary(R):
    verts, tris, H, W, *_ = scene()
    _, (face, depth, bary), *_ = scene_device()
    rng = np.random.default_rng(11)
    for Cn in (1, 3, 16):
        attrs = rng.normal(size=(len(verts), Cn)).astype(np.float32)
        got = R.interpolate(dev(attrs), dev(tris), face, bary).cpu().numpy()
        want = RO.interpolate(attrs, tris, face.cpu().numpy(), bary.cpu().numpy())
        assert got.shape == (H, W, Cn) and np.array_equal(got, want)
    with pytest.raises(RuntimeError, match="1 to 16"):
        R.interpolate(torch.zeros((len(verts), 17), device="cuda"), dev(tris), face, bary)


@pytest.mark.parametrize("background", ["none", "colour", "image"])
def test_render_mesh_bytes_are_exact_given_the_devices_bary(R, background):
    verts, tris, H, W, f, c, c2w = scene()
    _, (face, depth, bary), *_ = scene_device()
    face, bary = face.cpu().numpy(), bary.cpu().numpy()
    colors = scene_colors()
    image = np.random.default_rng(5).integers(0, 256, (H, W, 3)).astype(np.uint8)
    bg = {"none": None, "colour": (1.0, 0.5, 0.25), "image": dev(image)}[background]
    # outputs inside larger sentinel-filled buffers: nothing outside them is written
    n, pad = H * W, 64
    raw = {"rgba": torch.full((4 * n + 2 * pad,), 0x5A, dtype=torch.uint8, device="cuda"),
           "mask": torch.full((n + 2 * pad,), 0x5A, dtype=torch.uint8, device="cuda"),
           "depth": torch.full((n + 2 * pad,), -7.0, device="cuda"), "ray_t": torch.full((n + 2 * pad,), -7.0, device="cuda"),
           "face": torch.full((n + 2 * pad,), -77, dtype=torch.int32, device="cuda")}
    views = {"rgba": raw["rgba"][pad:pad + 4 * n].view(H, W, 4), "mask": raw["mask"][pad:pad + n].view(torch.bool),
             "depth": raw["depth"][pad:pad + n].view(H, W), "ray_t": raw["ray_t"][pad:pad + n].view(H, W),
             "face": raw["face"][pad:pad + n].view(H, W)}
    out = R.render_mesh(dev(verts), dev(tris), dev(colors), H, W, f, c, c2w, background=bg, out=views)
    assert out["rgba"] is views["rgba"]
    for name, sentinel in (("rgba", 0x5A), ("mask", 0x5A), ("depth", -7.0), ("ray_t", -7.0), ("face", -77)):
        assert (raw[name][:pad] == sentinel).all() and (raw[name][-pad:] == sentinel).all(), name
    fresh = R.render_mesh(dev(verts), dev(tris), dev(colors), H, W, f, c, c2w, background=bg)
    for name in views:
        assert torch.equal(fresh[name], views[name]), name
    hit = face >= 0
    rgba, mask = fresh["rgba"].cpu().numpy(), fresh["mask"].cpu().numpy()
    assert fresh["mask"].dtype == torch.bool and np.array_equal(mask, hit.reshape(-1))
    assert np.array_equal(rgba[..., 3], np.where(hit, 255, 0)) and np.array_equal(fresh["face"].cpu().numpy(), face)
    want = RO.quantise(RO.interpolate(colors, tris, face, bary))
    assert np.array_equal(rgba[..., :3][hit], want[hit])
    back = {"none": np.zeros((H, W, 3), np.uint8), "colour": np.broadcast_to(np.array([255, 128, 64], np.uint8), (H, W, 3)),
            "image": image}[background]
    assert np.array_equal(rgba[..., :3][~hit], back[~hit]) and (~hit).sum() > 300
    # colors=None is white
    white = R.render_mesh(dev(verts), dev(tris), None, H, W, f, c, c2w)["rgba"].cpu().numpy()
    assert (white[hit] == 255).all() and (white[~hit] == 0).all()


def test_headlight_shading_against_float64(R):
    verts, tris, H, W, f, c, _ = scene()
    from moco_flow_amd import camera
    c2w = camera.look_at_pose([0.4, -0.3, 0.2], [0.1, 0.0, -2.5])
    colors = scene_colors()
    out = R.render_mesh(dev(verts), dev(tris), dev(colors), H, W, f, c, c2w, shading="headlight", ambient=0.25)
    screen, inv_z = R.project_vertices(dev(verts), c2w, f, c)
    face, _, bary = (t.cpu().numpy() for t in R.rasterize(screen, inv_z, dev(tris), H, W))
    hit = face >= 0
    b = bary[hit].astype(np.float64)
    tri = verts.astype(np.float64)[tris[face[hit]]]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    to_cam = c2w[:3, 3] - np.einsum("nk,nkc->nc", b, tri)
    cos = np.abs(np.einsum("nc,nc->n", n, to_cam)) / (np.linalg.norm(n, axis=1) * np.linalg.norm(to_cam, axis=1))
    shade = np.float64(np.float32(0.25)) + (1 - np.float64(np.float32(0.25))) * cos
    col = np.einsum("nk,nkc->nc", b, colors.astype(np.float64)[tris[face[hit]]]) * shade[:, None]
    want = np.clip(np.floor(col * 255 + 0.5), 0, 255)
    got = out["rgba"].cpu().numpy()[..., :3][hit].astype(np.float64)
    diff = np.abs(got - want)
    print(f"headlight: {int((diff > 0).sum())} of {diff.size} bytes differ from float64 ({(diff > 0).mean():.3%}), largest difference {int(diff.max())}")
    assert diff.max() <= 1 and (diff > 0).mean() < 0.01
    assert shade.min() < 0.7 and shade.max() > 0.95                     # the term does something


def test_frames_feed_frame_rays(R):
    import moco_flow_amd as M
    from moco_flow_amd import camera
    verts, tris, H, W, f, c, _ = scene()
    c2w = camera.look_at_pose([0.4, -0.3, 0.2], [0.1, 0.0, -2.5])
    out = R.render_mesh(dev(verts), dev(tris), dev(scene_colors()), H, W, f, c, c2w, background=(1.0, 1.0, 1.0))
    fr = M.FrameRays(H, W, f, c, c2w, 0.1, 10.0, 0.0, rays_msk=out["mask"])
    assert fr.n_valid == int(out["mask"].sum()) > 1500
    white = torch.ones(3, device="cuda")
    perm = torch.randperm(fr.n_valid, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    rays, rgbs, bkgd, sel = fr.sample(512, image=out["rgba"], background=white, perm=perm)
    assert bool(out["mask"][sel].all()) and rgbs.shape == (512, 3)
    colour = out["rgba"].view(-1, 4)[sel][:, :3]
    assert torch.allclose(rgbs, colour.float() / 255, rtol=0, atol=1e-7)             # alpha 255: the rasterized colour itself,
    plain = fr.sample(512, image=out["rgba"][..., :3].contiguous(), perm=perm)[1]    # bit for bit what the RGB frame gives
    assert torch.equal(rgbs, plain)
    assert torch.equal(rays, camera.make_rays(H, W, f, c, c2w, 0.1, 10.0, 0.0)[sel])


def test_smpl_views(R):
    from moco_flow_amd import camera
    verts, tris = RO.icosphere(2, 0.6, (0.2, -0.1, 3.0))
    H, W, f, c = 45, 61, 60.0, (30.5, 22.5)
    views = list(R.smpl_views(dev(verts, torch.float32), dev(tris), 4, H, W, f, c, target=[0.2, -0.1, 3.0]))
    assert len(views) == 4
    positions = camera.sample_on_sphere(4, np.linalg.norm([0.2, -0.1, 3.0]))
    colors = ((verts - verts.min(0)) / (verts.max(0) - verts.min(0)))
    for (c2w, out), pos in zip(views, positions):
        assert np.allclose(c2w, camera.look_at_pose(pos + [0.2, -0.1, 3.0], [0.2, -0.1, 3.0]))
        rgba, mask = out["rgba"].cpu().numpy(), out["mask"].cpu().numpy().reshape(H, W)
        assert 150 < mask.sum() < 600 and mask[H // 2, W // 2]                    # a disc in the middle
        assert (rgba[~mask] == [255, 255, 255, 0]).all()
        ref = R.render_mesh(dev(verts, torch.float32), dev(tris), dev(colors, torch.float32), H, W, f, c, c2w, background=(1, 1, 1))
        assert np.abs(ref["rgba"].cpu().numpy().astype(int) - rgba).max() <= 1 and torch.equal(ref["mask"], out["mask"])


# ---- inputs ----
def test_strided_and_narrower_inputs_are_copied_or_refused(R):
    verts, tris, H, W, f, c, c2w = scene()
    (screen, inv_z), (face, depth, bary), *_ = scene_device()
    wide = torch.zeros((len(verts), 5), device="cuda")
    wide[:, 1:4] = dev(verts)
    s2, w2 = R.project_vertices(wide[:, 1:4], c2w, f, c)                              # a strided view
    assert torch.equal(s2, screen) and torch.equal(w2, inv_z)
    s3, w3 = R.project_vertices(dev(verts).double(), c2w, f, c)                        # float64 holding fp32 values
    assert torch.equal(s3, screen) and torch.equal(w3, inv_z)
    t2 = torch.zeros((len(tris), 4), dtype=torch.int64, device="cuda")
    t2[:, :3] = dev(tris)
    for other in (t2[:, :3], dev(tris).int()):
        for a, b in zip(R.rasterize(screen, inv_z, other, H, W), (face, depth, bary)):
            assert torch.equal(a, b)
    pair = torch.stack([screen, screen], dim=1)[:, 0]                                  # non-contiguous int32 rows
    assert not pair.is_contiguous() and torch.equal(R.rasterize(pair, inv_z, dev(tris), H, W)[0], face)
    with pytest.raises(RuntimeError, match="int64"):
        R.rasterize(screen, inv_z, dev(tris).float(), H, W)
    with pytest.raises(RuntimeError, match="int32 tensor of project_vertices"):
        R.rasterize(screen.long(), inv_z, dev(tris), H, W)
    with pytest.raises(RuntimeError, match="fp32 tensor of project_vertices"):
        R.rasterize(screen, inv_z.double(), dev(tris), H, W)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        R.rasterize(screen, inv_z, torch.from_numpy(tris), H, W)
    with pytest.raises(RuntimeError, match="contiguous"):
        R.render_mesh(dev(verts), dev(tris), None, H, W, f, c, c2w, out={"depth": torch.zeros((H, 2 * W), device="cuda")[:, ::2]})


def test_a_side_stream_gives_the_same_bits(R):
    verts, tris, H, W, f, c, c2w = scene()
    colors = dev(scene_colors())
    v, t = dev(verts), dev(tris)
    base = R.render_mesh(v, t, colors, H, W, f, c, c2w, shading="headlight")
    _, (face, depth, bary), *_ = scene_device()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        out = R.render_mesh(v, t, colors, H, W, f, c, c2w, shading="headlight")
        screen, inv_z = R.project_vertices(v, c2w, f, c)
        ras = R.rasterize(screen, inv_z, t, H, W)
        attr = R.interpolate(colors, t, ras[0], ras[2])
    side.synchronize()
    for name in base:
        assert torch.equal(base[name], out[name]), name
    for a, b in zip(ras, (face, depth, bary)):
        assert torch.equal(a, b)
    assert torch.equal(attr, R.interpolate(colors, t, face, bary))
