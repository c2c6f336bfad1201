"""A triangle rasterizer on the device (reference: scripts/data_utils.py:23-86 ``Renderer``, :273-336 ``create_init_nerf_data``
-- the 120 stage-1 views of the posed SMPL mesh -- and the SMPL overlay of ``create_moco_flow_data(vis=True)``, :255-263; the
camera is utils/camera.py:29-81, the one ``camera.make_rays`` shoots rays through):

    project_vertices   world vertices -> screen positions snapped to 1/256 pixel, and 1 / z             (mf_project_vertices)
    rasterize          -> face (H, W), depth (H, W), perspective-correct bary (H, W, 3)          (mf_rasterize, mf_raster_resolve)
    interpolate        vertex attributes through (face, bary)                                         (mf_raster_interpolate)
    render_mesh        -> rgba bytes, mask, depth, ray_t, face: projection, mf_rasterize and ONE fused resolve (mf_raster_shade)
    smpl_views         the stage-1 views: position-coloured mesh, cameras on a sphere, white background

The reference draws with pyrender, which needs an OpenGL / EGL context.  PYRENDER NOT RESTATED: its metallic-roughness BRDF and
the three point lights of data_utils.py:36-46 are third-party arithmetic this project does not restate and is UNPINNED AGAINST
(as kornia and cv2 are): ``render_mesh`` gives the interpolated vertex colours -- what stage 1 trains on up to pyrender's
lighting -- optionally times a headlight term.

Camera convention (the contract): with p_cam = R^T (p_world - t) and z = -p_cam.z, column x = cx + f p_cam.x / z and row
y = cy - f p_cam.y / z, one focal length for both axes.  The sample of pixel (row j, column i) sits at (x, y) = (i, j) +
pixel_offset: 0.0 (the default) is where ``make_rays`` shoots that pixel's ray -- a rasterized pixel and the NeRF's ray for it see
the same point -- and 0.5 is OpenGL's sample position; other values raise.

Coverage is decided in integers with a top-left fill rule, visibility is the minimum of a 64-bit (depth, index) key: frames are
bit-identical from run to run and under a permutation of the triangle list (csrc/mf_raster.hip).  A triangle with a
vertex at z <= znear or beyond +-2^15 pixels is dropped whole: there is no clipping.  A viewport-filling triangle costs H W / 64
steps of one wave: many such triangles are slow.

CPU tensors raise.  No gradients.  Everything runs on the current stream of the inputs' device."""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from . import camera as _camera

__all__ = ["project_vertices", "rasterize", "interpolate", "render_mesh", "smpl_views"]

BEHIND = -2 ** 31          # both screen coordinates of a vertex at z <= znear


def _f32(x):
    return float(np.float32(x))


def _c2w(c2w, what):
    m = np.asarray(c2w.detach().cpu() if isinstance(c2w, torch.Tensor) else c2w, dtype=np.float64)
    if m.ndim != 2 or m.shape[0] not in (3, 4) or m.shape[1] != 4:
        raise RuntimeError(f"moco_flow_amd.raster.{what}: c2w must be a (3|4, 4) matrix, got shape {m.shape}")
    m = m[:3, :4].astype(np.float32)                                    # camera.py:141 .float()
    return (C.c_float * 12)(*m.reshape(-1).tolist())


def _offset(pixel_offset, what):
    if pixel_offset not in (0.0, 0.5):
        raise RuntimeError(f"moco_flow_amd.raster.{what}: pixel_offset={pixel_offset!r} must be 0.0 (make_rays' sample position) or "
                           "0.5 (OpenGL's)")
    return float(pixel_offset)


def _view(H, W, what):
    H, W = int(H), int(W)
    if H <= 0 or W <= 0 or H * W >= 2 ** 31:
        raise RuntimeError(f"moco_flow_amd.raster.{what}: H={H} W={W}; needs H, W >= 1 and H W < 2^31")
    return H, W


def _rows(t, cols, dtype, name, what, device=None):
    """A (N, cols) tensor of `dtype` on the device, contiguous: a strided view or another float / integer width is copied once;
    a wrong shape or kind of dtype raises."""
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"moco_flow_amd.raster.{what}: {name} must be a tensor, got {type(t).__name__}")
    if t.dim() != 2 or (cols is not None and t.shape[1] != cols):
        raise RuntimeError(f"moco_flow_amd.raster.{what}: {name} must be (N, {cols if cols is not None else 'C'}), got shape {tuple(t.shape)}")
    if dtype == torch.float32 and not t.is_floating_point():
        raise RuntimeError(f"moco_flow_amd.raster.{what}: {name} must be a floating-point tensor, got {t.dtype}")
    if dtype in (torch.int64, torch.int32) and t.dtype not in (torch.int64, torch.int32):
        raise RuntimeError(f"moco_flow_amd.raster.{what}: {name} must be an int64 (or int32, copied) tensor, got {t.dtype}")
    L.require_gpu(t, "raster." + what)
    if device is not None and t.device != device:
        raise RuntimeError(f"moco_flow_amd.raster.{what}: {name} is on {t.device}, the other inputs on {device}")
    return t.detach().to(dtype).contiguous()


def _tris(tris, what, device):
    t = _rows(tris, 3, torch.int64, "tris", what, device)
    if t.shape[0] >= 2 ** 31:
        raise RuntimeError(f"moco_flow_amd.raster.{what}: {t.shape[0]} triangles; needs T < 2^31")
    return t


def project_vertices(verts, c2w, focal, center, znear=1e-3, return_xy=False):
    """verts (V, 3) float on the device -> screen (V, 2) int32 = (x, y) in 1/256-pixel fixed point, rintf(256 x), and inv_z (V,)
    fp32 = 1 / z; a vertex with z <= znear has inv_z = 0 and both screen coordinates ``BEHIND``.  fp32, every operation rounded
    once.  focal, center = (cx, cy), c2w: as ``camera.make_rays`` takes them.  return_xy: also the unsnapped (V, 2) fp32 positions
    (NaN where behind)."""
    v = _rows(verts, 3, torch.float32, "verts", "project_vertices")
    dev, V = v.device, v.shape[0]
    mat = _c2w(c2w, "project_vertices")
    screen = torch.empty((V, 2), dtype=torch.int32, device=dev)
    inv_z = torch.empty(V, dtype=torch.float32, device=dev)
    xy = torch.empty((V, 2), dtype=torch.float32, device=dev) if return_xy else None
    L.launch(dev, "mf_project_vertices", L.ptr0(v), V, mat, _f32(focal), _f32(center[0]), _f32(center[1]), _f32(znear),
             L.ptr0(screen), L.ptr0(inv_z), L.ptr0(xy))
    return (screen, inv_z, xy) if return_xy else (screen, inv_z)


def _fill_keys(screen, inv_z, tris, H, W, pixel_offset, what):
    """Checks, scratch and mf_rasterize; -> (screen, inv_z, tris, scratch), the tensors as the launches read them."""
    if not isinstance(screen, torch.Tensor) or screen.dtype != torch.int32:
        raise RuntimeError(f"moco_flow_amd.raster.{what}: screen must be the int32 tensor of project_vertices")
    screen = _rows(screen, 2, torch.int32, "screen", what)
    dev, V = screen.device, screen.shape[0]
    if not isinstance(inv_z, torch.Tensor) or inv_z.dim() != 1 or inv_z.shape[0] != V or inv_z.dtype != torch.float32:
        raise RuntimeError(f"moco_flow_amd.raster.{what}: inv_z must be the ({V},) fp32 tensor of project_vertices")
    L.require_gpu(inv_z, "raster." + what)
    if inv_z.device != dev:
        raise RuntimeError(f"moco_flow_amd.raster.{what}: inv_z is on {inv_z.device}, screen on {dev}")
    inv_z = inv_z.detach().contiguous()
    tris = _tris(tris, what, dev)
    scratch = L.scratch(dev, "mf_raster_scratch_bytes", H, W)
    L.launch(dev, "mf_rasterize", L.ptr0(screen), L.ptr0(inv_z), V, L.ptr0(tris), tris.shape[0], H, W, pixel_offset,
             scratch.data_ptr())
    return screen, inv_z, tris, scratch


def rasterize(screen, inv_z, tris, H, W, pixel_offset=0.0, return_dropped=False):
    """screen, inv_z: project_vertices'; tris (T, 3) int64 (int32 is copied) -> face (H, W) int32 (-1 = none), depth (H, W) fp32
    (camera-axis z, +inf where none), bary (H, W, 3) fp32 (perspective-correct, zeros where none).  No culling; zero-area
    triangles cover nothing; triangles sharing an edge never both cover, or both miss, a sample on it.  return_dropped: also
    the number of triangles dropped whole (a vertex at z <= znear or beyond +-2^15 pixels, an index outside [0, V)) -- a device
    counter, read back (one synchronisation) only here."""
    H, W = _view(H, W, "rasterize")
    off = _offset(pixel_offset, "rasterize")
    screen, inv_z, tris, scratch = _fill_keys(screen, inv_z, tris, H, W, off, "rasterize")
    dev = screen.device
    face = torch.empty((H, W), dtype=torch.int32, device=dev)
    depth = torch.empty((H, W), dtype=torch.float32, device=dev)
    bary = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    dropped = torch.empty(1, dtype=torch.int64, device=dev) if return_dropped else None
    L.launch(dev, "mf_raster_resolve", scratch.data_ptr(), L.ptr0(screen), L.ptr0(inv_z), screen.shape[0], L.ptr0(tris),
             tris.shape[0], H, W, off, face.data_ptr(), depth.data_ptr(), bary.data_ptr(), L.ptr(dropped))
    return (face, depth, bary, int(dropped.item())) if return_dropped else (face, depth, bary)


def interpolate(attrs, tris, face, bary):
    """attrs (V, C) float, 1 <= C <= 16; face (H, W) int32 and bary (H, W, 3) fp32 of rasterize -> (H, W, C) fp32 =
    (bary_0 a_0 + bary_1 a_1) + bary_2 a_2; zeros where face < 0."""
    a = _rows(attrs, None, torch.float32, "attrs", "interpolate")
    dev, Cn = a.device, a.shape[1]
    if Cn < 1 or Cn > 16:
        raise RuntimeError(f"moco_flow_amd.raster.interpolate: attrs has {Cn} columns; 1 to 16 are built")
    tris = _tris(tris, "interpolate", dev)
    if not isinstance(face, torch.Tensor) or face.dtype != torch.int32 or face.dim() != 2:
        raise RuntimeError("moco_flow_amd.raster.interpolate: face must be the (H, W) int32 tensor of rasterize")
    H, W = face.shape
    if not isinstance(bary, torch.Tensor) or bary.dtype != torch.float32 or tuple(bary.shape) != (H, W, 3):
        raise RuntimeError(f"moco_flow_amd.raster.interpolate: bary must be the ({H}, {W}, 3) fp32 tensor of rasterize")
    for name, t in (("face", face), ("bary", bary)):
        L.require_gpu(t, "raster.interpolate")
        if t.device != dev:
            raise RuntimeError(f"moco_flow_amd.raster.interpolate: {name} is on {t.device}, attrs on {dev}")
    face, bary = face.contiguous(), bary.contiguous()
    out = torch.empty((H, W, Cn), dtype=torch.float32, device=dev)
    L.launch(dev, "mf_raster_interpolate", L.ptr0(a), a.shape[0], Cn, L.ptr0(tris), tris.shape[0], L.ptr0(face), L.ptr0(bary),
             H * W, L.ptr0(out))
    return out


def quantise(v):
    """The 8-bit rounding of vis.frame_sheet (torchvision's save_image): (uint8) clamp(v 255 + 0.5, 0, 255) in fp32, truncated."""
    t = np.asarray(v, dtype=np.float32) * np.float32(255) + np.float32(0.5)
    return np.clip(np.nan_to_num(t, nan=0.0), 0, 255).astype(np.uint8)


_SHADING = {"none": L.MF_RASTER_SHADE_NONE, "headlight": L.MF_RASTER_SHADE_HEADLIGHT}
_OUT = (("rgba", torch.uint8, lambda H, W: (H, W, 4)), ("mask", torch.bool, lambda H, W: (H * W,)),
        ("depth", torch.float32, lambda H, W: (H, W)), ("ray_t", torch.float32, lambda H, W: (H, W)),
        ("face", torch.int32, lambda H, W: (H, W)))


def render_mesh(verts, tris, colors, H, W, focal, center, c2w, background=None, shading="none", ambient=0.3, pixel_offset=0.0,
                znear=1e-3, out=None):
    """Draw a mesh: verts (V, 3), tris (T, 3) int64, colors (V, 3) float in [0, 1] or None (white) ->
        rgba  (H, W, 4) uint8: alpha 255 where covered, 0 elsewhere; rgb where covered = the interpolated colour, quantised as
              vis.frame_sheet quantises ((uint8) clamp(c 255 + 0.5, 0, 255) in fp32, truncated: torchvision's save_image); elsewhere
              the background: None -> 0, one (3,) colour in [0, 1] (host numbers; quantised the same way), or an (H, W, 3) uint8
              device image.  Goes straight into ``FrameRays.sample(image=...)``
        mask  (H W,) bool, the silhouette, for ``FrameRays(rays_msk=...)``
        depth (H, W) fp32 camera-axis z, +inf where nothing is
        ray_t (H, W) fp32 = z |((i - cx) / f, -(j - cy) / f, -1)|: with pixel_offset 0 the surface point on ``make_rays``' ray
              (o, d) of that pixel is o + ray_t d
        face  (H, W) int32, -1 where nothing is
    as a dict.  shading "headlight" multiplies the colour by ambient + (1 - ambient) |n . v|, n the unit normal of the triangle's
    world vertices and v the unit direction from the surface point to the camera.  PYRENDER NOT RESTATED (module docstring):
    neither its BRDF nor its lights.  Three launches: projection, mf_rasterize, one fused resolve; no host synchronisation.
    out: a dict of preallocated contiguous tensors to write into instead (any subset of the five)."""
    H, W = _view(H, W, "render_mesh")
    off = _offset(pixel_offset, "render_mesh")
    if shading not in _SHADING:
        raise RuntimeError(f"moco_flow_amd.raster.render_mesh: shading={shading!r} must be 'none' or 'headlight'")
    v = _rows(verts, 3, torch.float32, "verts", "render_mesh")
    dev, V = v.device, v.shape[0]
    col = None
    if colors is not None:
        col = _rows(colors, 3, torch.float32, "colors", "render_mesh", dev)
        if col.shape[0] != V:
            raise RuntimeError(f"moco_flow_amd.raster.render_mesh: colors has {col.shape[0]} rows, the mesh {V} vertices")
    a = L.mf_raster_shade_args()
    a.background_kind = L.MF_RASTER_BG_NONE
    bg_image = None
    if isinstance(background, torch.Tensor) and background.dtype == torch.uint8:
        if tuple(background.shape) != (H, W, 3):
            raise RuntimeError(f"moco_flow_amd.raster.render_mesh: a background image must be ({H}, {W}, 3) uint8, got {tuple(background.shape)}")
        L.require_gpu(background, "raster.render_mesh")
        if background.device != dev:
            raise RuntimeError(f"moco_flow_amd.raster.render_mesh: background is on {background.device}, verts on {dev}")
        bg_image = background.contiguous()
        a.background_kind, a.background_image = L.MF_RASTER_BG_IMAGE, bg_image.data_ptr()
    elif background is not None:
        rgb = np.asarray(background.detach().cpu() if isinstance(background, torch.Tensor) else background, dtype=np.float32)
        if rgb.shape != (3,):
            raise RuntimeError(f"moco_flow_amd.raster.render_mesh: background must be None, one (3,) colour in [0, 1] or an ({H}, {W}, 3) "
                               f"uint8 image, got shape {rgb.shape}")
        a.background_kind = L.MF_RASTER_BG_COLOUR
        a.background_colour = (C.c_uint8 * 4)(*quantise(rgb).tolist(), 0)
    mat = _c2w(c2w, "render_mesh")
    screen, inv_z = project_vertices(v, c2w, focal, center, znear=znear)
    screen, inv_z, tris, scratch = _fill_keys(screen, inv_z, tris, H, W, off, "render_mesh")
    res = {}
    for name, dtype, shape in _OUT:
        if out is not None and name in out:
            t = out[name]
            if t.dtype != dtype or tuple(t.shape) != shape(H, W) or not t.is_contiguous() or t.device != dev:
                raise RuntimeError(f"moco_flow_amd.raster.render_mesh: out[{name!r}] must be a contiguous {shape(H, W)} {dtype} tensor on {dev}")
            res[name] = t
        elif out is None:
            res[name] = torch.empty(shape(H, W), dtype=dtype, device=dev)
    if not res:
        raise RuntimeError("moco_flow_amd.raster.render_mesh: out names none of rgba, mask, depth, ray_t, face")
    a.scratch, a.screen, a.inv_z, a.verts, a.colors, a.V = scratch.data_ptr(), L.ptr0(screen), L.ptr0(inv_z), L.ptr0(v), L.ptr0(col), V
    a.tris, a.T, a.H, a.W = L.ptr0(tris), tris.shape[0], H, W
    a.focal, a.cx, a.cy, a.pixel_offset = _f32(focal), _f32(center[0]), _f32(center[1]), off
    a.c2w = mat
    a.shading, a.ambient = _SHADING[shading], _f32(ambient)
    for name in res:
        setattr(a, name, res[name].data_ptr())
    L.launch(dev, "mf_raster_shade", C.byref(a))
    return res


def smpl_views(verts, faces, num_images, H, W, focal, center, **kw):
    """The stage-1 views of create_init_nerf_data (data_utils.py:273-336) without pyrender: verts (V, 3) -- the posed SMPL
    vertices plus the translation, as ``smpl.SMPL`` returns them -- are coloured with their bounding-box-normalised position
    (:293-295, on the device); the cameras are ``camera.sample_on_sphere(num_images, |target|)`` moved by, and looking at,
    ``target`` (:315-317).  target= is the reference's ``cur_transl``; the default is the mean vertex, for a caller without the
    VIBE translation (one device read per mesh, never per view).  Yields (c2w (4, 4) float64 numpy, render_mesh(...) dict) per
    view, white background.  faces: ``SMPL.faces`` on the device.  Further keywords go to render_mesh."""
    v = _rows(verts, 3, torch.float32, "verts", "smpl_views")
    target = kw.pop("target", None)
    if target is None:
        target = v.double().mean(dim=0).cpu().numpy()                   # one read, per mesh and never per view
    target = np.asarray(target, dtype=np.float64).reshape(3)
    lo, hi = v.min(dim=0).values, v.max(dim=0).values
    colors = (v - lo) / (hi - lo)
    kw.setdefault("background", (1.0, 1.0, 1.0))
    for position in _camera.sample_on_sphere(int(num_images), float(np.sqrt(np.sum(target ** 2)))):
        c2w = _camera.look_at_pose(position + target, target)
        yield c2w, render_mesh(v, faces, colors, H, W, focal, center, c2w, **kw)
