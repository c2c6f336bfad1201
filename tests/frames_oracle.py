"""TEST INFRASTRUCTURE ONLY -- numpy restatement of csrc/mf_frames.hip (include/mocoflow_hip.h: mf_resize_u8, mf_composite_rows,
mf_background_plate), written from the recipes alone, plus the reference's float64 plate expression
(scripts/data_utils.py:150-163).  tests/test_frames_cpu.py holds it to PIL's own outputs (tests/golden/u_frames.npz, and live
PIL where it imports); the GPU tests hold the kernels to it."""
import math

import numpy as np

PRECISION_BITS = 22


def coeffs(n_in, n_out):
    """One axis of PIL's bilinear resample, per output index and in float64 -> bounds (n_out, 2), kk (n_out, ksize) int32."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((n_out, 2), dtype=np.int32)
    kk = np.zeros((n_out, ksize), dtype=np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(0, int(center - support + 0.5))
        n = min(n_in, int(center + support + 0.5)) - xmin
        w = [max(0.0, 1.0 - abs((x + xmin - center + 0.5) / fs)) for x in range(n)]
        total = 0.0
        for v in w:
            total += v
        if total != 0.0:
            w = [v / total for v in w]
        bounds[xx] = (xmin, n)
        for x in range(n):
            kk[xx, x] = int(0.5 + w[x] * (1 << PRECISION_BITS))
    return bounds, kk


def _pass(a, axis, n_out):
    """Resample `axis` of the int64 array a (values 0 .. 255) to n_out entries; returns values 0 .. 255."""
    bounds, kk = coeffs(a.shape[axis], n_out)
    a = np.moveaxis(a, axis, 0)
    out = np.empty((n_out,) + a.shape[1:], dtype=np.int64)
    for o in range(n_out):
        first, n = int(bounds[o, 0]), int(bounds[o, 1])
        k = kk[o, :n].astype(np.int64).reshape((n,) + (1,) * (a.ndim - 1))
        acc = (1 << (PRECISION_BITS - 1)) + (a[first:first + n] * k).sum(axis=0)
        assert acc.max(initial=0) < 2 ** 31
        out[o] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize(a, size):
    """a: (H0, W0, C) or (F, H0, W0, C) uint8, C in {1, 3, 4}; size = (H, W) -> uint8 of the same rank."""
    a = np.asarray(a)
    assert a.dtype == np.uint8
    stack = a if a.ndim == 4 else a[None]
    H, W = size
    if (H, W) == stack.shape[1:3]:
        return a.copy()
    v = stack.astype(np.int64)
    rgba = stack.shape[3] == 4
    if rgba:
        t = v[..., :3] * v[..., 3:] + 128
        v = np.concatenate([(t + (t >> 8)) >> 8, v[..., 3:]], axis=3)
    if W != stack.shape[2]:
        v = _pass(v, 2, W)
    if H != stack.shape[1]:
        v = _pass(v, 1, H)
    if rgba:
        c, al = v[..., :3], v[..., 3:]
        un = np.minimum(255, 255 * c // np.maximum(al, 1))
        v = np.concatenate([np.where((al == 0) | (al == 255), c, un), al], axis=3)
    out = v.astype(np.uint8)
    return out if a.ndim == 4 else out[0]


INV255 = np.float32(1.0) / np.float32(255.0)


def to_rows(u8):
    """(H, W, 3) uint8 -> (H W, 3) fp32: u * (1.0f / 255.0f), one rounding for the reciprocal and one for the product."""
    return (u8.reshape(-1, 3).astype(np.float32) * INV255).astype(np.float32)


def composite(rgba, background):
    """(H, W, 4) uint8 over fp32 rows (H W, 3) or one colour (3,): v a + bg (1 - a), every operation rounded once in fp32."""
    px = rgba.reshape(-1, 4).astype(np.float32) * INV255
    a = px[:, 3:4]
    na = np.float32(1.0) - a
    bg = np.broadcast_to(np.asarray(background, dtype=np.float32).reshape(-1, 3), (px.shape[0], 3))
    fg = (px[:, :3] * a).astype(np.float32)
    back = (bg * na).astype(np.float32)
    return (fg + back).astype(np.float32)


def plate(frames, masks, k):
    """frames (F, H, W, 3 | 4), masks (F, H, W) uint8 -> (H, W, 3) uint8: (key_k + 127) // 255 of the k-th smallest key u (255 - m)."""
    key = frames[..., :3].astype(np.int64) * (255 - masks.astype(np.int64))[..., None]
    kth = np.sort(key, axis=0)[k]
    return ((kth + 127) // 255).astype(np.uint8)


def plate_float64(frames, masks, k):
    """scripts/data_utils.py:150-163 in its own arithmetic: the float64 image np.sort(img / 255. * (1 - msk / 255.), axis=0)[k]."""
    img = frames[..., :3].astype(np.float64) / 255.
    msk = masks.astype(np.float64)[..., None] / 255.
    return np.sort(img * (1 - msk), axis=0)[k]


def plate_float64_bytes(frames, masks, k):
    return np.floor(255.0 * plate_float64(frames, masks, k) + 0.5).astype(np.uint8)


def plate_inputs(rng, F, H, W, C, soft):
    """Seeded plate inputs with the edge cases in them: few distinct byte values (ties across the frames), pixel 0 masked in
    every frame, pixel 1 in none; binary masks, or half of the entries soft."""
    frames = (rng.integers(0, 9, size=(F, H, W, C)) * 31).astype(np.uint8)
    masks = (rng.integers(0, 2, size=(F, H, W)) * 255).astype(np.uint8)
    if soft:
        masks = np.where(rng.random((F, H, W)) < 0.5, rng.integers(0, 256, size=(F, H, W)), masks).astype(np.uint8)
    masks.reshape(F, -1)[:, 0] = 255
    masks.reshape(F, -1)[:, 1] = 0
    return frames, masks
