"""Device-side ray generation: Camera.make_rays of
/root/reference/utils/camera.py:134-148 (gen_ray_directions :29-50, gen_rays :52-81) as one HIP
launch writing the (H*W, 9) ray tensor straight into GPU memory -- no host tensor, no H2D copy per
chunk (trainer_moco_flow.py:201-202)."""
import ctypes as C

import numpy as np
import torch

from . import _lib as L


def sample_on_sphere(num, dist=1.0, half=False):
    """Camera positions for the stage-1 views (scripts/data_utils.py:166-181): a golden-ratio spiral on the sphere of radius
    ``dist``.  With N = 2 num if half else num and g = (sqrt(5) - 1) / 2, point n = 1 .. N has y = (2 n - 1) / N - 1 and the
    angle 2 pi n g around the y axis: (cos(a) r, y, sin(a) r) dist with r = sqrt(1 - y^2); ``half`` keeps the points with
    y >= 0.  Host numpy, float64, (num, 3)."""
    n_all = int(num) * 2 if half else int(num)
    n = np.arange(1, n_all + 1, dtype=np.float64)
    y = (2.0 * n - 1) / n_all - 1.0
    ang = 2 * np.pi * n * ((np.sqrt(5) - 1.0) / 2.0)
    r = np.sqrt(1 - y * y)
    pts = np.stack([np.cos(ang) * r * dist, y * dist, np.sin(ang) * r * dist], axis=1)
    return pts[y >= 0] if half else pts


def look_at_pose(position, target):
    """The (4, 4) float64 camera-to-world pose at ``position`` whose -z axis passes through ``target``
    (get_camera_pose, scripts/data_utils.py:184-200): z = unit(position - target), x = unit((0, 0, 1) x z) -- or (1, 0, 0)
    where |z.z| >= 0.999 -- and y = z x x.  (Like the reference's, the pose of that pole branch is orthonormal only exactly at
    the pole.)"""
    position, target = np.asarray(position, dtype=np.float64), np.asarray(target, dtype=np.float64)
    z = position - target
    z = z / np.linalg.norm(z)
    if abs(z[2]) < 0.999:
        x = np.cross(np.array([0.0, 0.0, 1.0]), z)
        x = x / np.linalg.norm(x)
    else:
        x = np.array([1.0, 0.0, 0.0])
    pose = np.eye(4)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = x, np.cross(z, x), z, position
    return pose


def spheric_poses(num=30, radius=2.0, center=(0, 0, 0), vec_up=None):
    """The (3 num, 4, 4) float32 turntable of create_spheric_poses / pose_spherical (utils/vis_utils.py:46-119): ``num`` angles
    theta = 360 k / num at each of the elevations phi = 0, -15, -30 degrees.  One pose is, in float32 matrices multiplied in
    this order, A Ry(theta) Rx(phi) T(radius) -- T moves the camera along +z, Rx(phi) = [[1, 0, 0], [0, cos, -sin], [0, sin, cos]],
    Ry(theta) = [[cos, 0, -sin], [0, 1, 0], [sin, 0, cos]], A swaps y and z and negates x -- then, with vec_up, the frame
    (u1, u x u1, u) of the unit up vector u with u1 = (u.x, -u.z, u.y) in front of it; ``center`` is added to the position."""
    def one(theta, phi):
        th, ph = theta / 180.0 * np.pi, phi / 180.0 * np.pi
        move = np.eye(4, dtype=np.float32)
        move[2, 3] = radius
        rx = np.eye(4, dtype=np.float32)
        rx[1, 1], rx[1, 2], rx[2, 1], rx[2, 2] = np.cos(ph), -np.sin(ph), np.sin(ph), np.cos(ph)
        ry = np.eye(4, dtype=np.float32)
        ry[0, 0], ry[0, 2], ry[2, 0], ry[2, 2] = np.cos(th), -np.sin(th), np.sin(th), np.cos(th)
        axes = np.array([[-1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1]], dtype=np.float32)
        m = axes @ (ry @ (rx @ move))
        if vec_up is not None:
            u = np.asarray(vec_up) / np.linalg.norm(vec_up)
            u1 = np.array([u[0], -u[2], u[1]])
            frame = np.eye(4, dtype=np.float32)
            frame[:3, 0], frame[:3, 1], frame[:3, 2] = u1, np.cross(u, u1), u
            m = frame @ m
        if center is not None:
            m[:3, 3] += center
        return m
    angles = np.linspace(0, 360, int(num) + 1)[:-1]
    return np.stack([one(a, phi) for phi in (0.0, -15.0, -30.0) for a in angles], 0)


def make_rays(H, W, focal, center, c2w, near, far, idx, device="cuda"):
    """rays (H*W, 9) = [o, unit d, near, far, idx] on ``device``; ``focal`` = K[0][0] (the reference uses
    focal[0] for both axes, camera.py:47), ``center`` = (K[0][2], K[1][2]), ``c2w`` (3|4, 4) array or None."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("moco_flow_amd.camera.make_rays: this is the MI355X (HIP) path; no CPU implementation")
    out = torch.empty((H * W, 9), device=dev, dtype=torch.float32)
    mat = None
    if c2w is not None:
        m = np.asarray(c2w, dtype=np.float64)[:3, :4].astype(np.float32)      # camera.py:141 .float()
        mat = (C.c_float * 12)(*m.reshape(-1).tolist())
    L.launch(dev, "mf_make_rays", H, W, float(np.float32(focal)), float(np.float32(center[0])), float(np.float32(center[1])), mat,
             float(np.float32(near)), float(np.float32(far)), float(np.float32(idx)), out.data_ptr())
    return out


def near_far_from_aabb(aabb_verts, c2w):
    """camera.py:138-139: min / max distance from the camera origin to the AABB corners (host scalars)."""
    d = np.sqrt(np.sum((np.asarray(aabb_verts) - np.asarray(c2w)[:3, 3]) ** 2, axis=-1))
    return float(min(d)), float(max(d))


def project_aabb(aabb_verts, c2w, K):
    """calculate_2d_projections (camera.py:83-103): the 8 AABB corners in integer pixel coordinates (x = column,
    y = row), host side (8 points), same numpy operations in the same order as the reference."""
    pts = np.asarray(aabb_verts).transpose()
    homo = np.vstack([pts, np.ones((1, pts.shape[1]), dtype=np.float32)])
    cam = np.linalg.inv(np.asarray(c2w)) @ homo
    cam = cam[:3, :] / cam[3, :]
    cam[1:, :] *= -1
    pix = np.asarray(K) @ cam[:3, :]
    pix = (pix[:2, :] / pix[2, :]).transpose()
    return np.array(pix, dtype=np.int32)


def valid_rays_mask(aabb_verts, c2w, K, size, device="cuda"):
    """Camera.get_valid_rays_mask (camera.py:119-132): bool (H*W,) on ``device`` -- the filled convex hull of the
    projected AABB, written by mf_valid_rays_mask (no H x W host image, no cv2).  ``size`` = (H, W)."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("moco_flow_amd.camera.valid_rays_mask: this is the MI355X (HIP) path; no CPU implementation")
    H, W = int(size[0]), int(size[1])
    pix = np.ascontiguousarray(project_aabb(aabb_verts, c2w, K).reshape(-1, 2), dtype=np.int32)
    out = torch.empty(H * W, device=dev, dtype=torch.uint8)
    arr = (C.c_int32 * pix.size)(*pix.reshape(-1).tolist())
    L.launch(dev, "mf_valid_rays_mask", H, W, arr, pix.shape[0], out.data_ptr())
    return out.bool()
