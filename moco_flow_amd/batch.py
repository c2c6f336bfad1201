"""The ray batch of a training step, built on the device (reference: trainer/trainer_moco_flow.py:407-417 and the same lines
of trainer/trainer_nerf.py, fed by datasets/moco_flow_dataset.py:166-176, 190-196; the chain_global column of _shared_step,
trainer_moco_flow.py:308-312).

The reference keeps per frame the (H W, 9) ray table, the composited (H W, 3) image and the (H W, 3) background, and draws a
batch with torch.nonzero, torch.randperm and three gathers.  The batch is a pure function of the camera, the hull mask, the
image and a permutation:

    FrameRays          the per-frame constants; construction compacts the mask once (mf_mask_compact) and reads n_valid --
                       the one device -> host read, per frame and never per step
    FrameRays.sample   (rays, rgbs, background, sel_inds) of N_rand rays in ONE mf_ray_batch launch that reads none of those
                       tables: each ray is computed from its pixel by the device function mf_make_rays uses (bit-identical
                       rows), the pixel is composited from the 8-bit image as ToTensor and moco_flow_dataset.py:174 do

The kernel is deterministic; the randomness is the permutation, drawn by torch (or passed in).  No gradients."""
import ctypes as C

import numpy as np
import torch

from . import _lib as L

__all__ = ["FrameRays"]


def _image_kind(image, H, W):
    """MF_IMAGE_* of `image` (None, (H W, 3) fp32 rows, (H, W, 3) or (H, W, 4) uint8); RuntimeError for anything else."""
    if image is None:
        return L.MF_IMAGE_NONE
    if not isinstance(image, torch.Tensor):
        raise RuntimeError(f"moco_flow_amd.batch: image must be a tensor, got {type(image).__name__}")
    shape = tuple(image.shape)
    if image.dtype == torch.float32 and shape == (H * W, 3):
        kind = L.MF_IMAGE_ROWS
    elif image.dtype == torch.uint8 and shape == (H, W, 3):
        kind = L.MF_IMAGE_U8_RGB
    elif image.dtype == torch.uint8 and shape == (H, W, 4):
        kind = L.MF_IMAGE_U8_RGBA
    else:
        raise RuntimeError(f"moco_flow_amd.batch: image is {shape} {image.dtype}; fp32 rows ({H * W}, 3), or uint8 ({H}, {W}, 3) "
                           f"or ({H}, {W}, 4)")
    L.require_gpu(image, "batch.FrameRays.sample")
    return kind


def _background_kind(background, H, W):
    """MF_BACKGROUND_* of `background` (None, (H W, 3) fp32 rows, (3,) fp32 colour); RuntimeError for anything else."""
    if background is None:
        return L.MF_BACKGROUND_NONE
    if not isinstance(background, torch.Tensor):
        raise RuntimeError(f"moco_flow_amd.batch: background must be a tensor, got {type(background).__name__}")
    shape = tuple(background.shape)
    if background.dtype == torch.float32 and shape == (H * W, 3):
        kind = L.MF_BACKGROUND_ROWS
    elif background.dtype == torch.float32 and shape == (3,):
        kind = L.MF_BACKGROUND_COLOUR
    else:
        raise RuntimeError(f"moco_flow_amd.batch: background is {shape} {background.dtype}; fp32 rows ({H * W}, 3) or one fp32 "
                           "colour (3,)")
    L.require_gpu(background, "batch.FrameRays.sample")
    return kind


def _check_mask(rays_msk, H, W):
    if rays_msk is None:
        return
    if not isinstance(rays_msk, torch.Tensor) or rays_msk.dtype not in (torch.bool, torch.uint8) or tuple(rays_msk.shape) != (H * W,):
        what = f"{tuple(rays_msk.shape)} {rays_msk.dtype}" if isinstance(rays_msk, torch.Tensor) else type(rays_msk).__name__
        raise RuntimeError(f"moco_flow_amd.batch.FrameRays: rays_msk is {what}; a bool or uint8 tensor of shape ({H * W},) "
                           "(camera.valid_rays_mask's), or None")


def _check_perm(perm, n, device):
    if not isinstance(perm, torch.Tensor) or perm.dtype != torch.int64 or perm.dim() != 1:
        what = f"{tuple(perm.shape)} {perm.dtype}" if isinstance(perm, torch.Tensor) else type(perm).__name__
        raise RuntimeError(f"moco_flow_amd.batch: perm is {what}; a 1-D int64 tensor of positions into val_inds")
    if perm.numel() < n:
        raise RuntimeError(f"moco_flow_amd.batch: perm has {perm.numel()} entries, the batch needs {n}")
    L.require_gpu(perm, "batch.FrameRays.sample")
    if device is not None and perm.device != device:
        raise RuntimeError(f"moco_flow_amd.batch: perm is on {perm.device}, the frame on {device}")


class FrameRays:
    """The per-frame constants of a training batch.  H, W, focal, center, c2w, near, far, idx: as camera.make_rays takes them
    (the same fp32 casts).  rays_msk: (H W,) bool or uint8, device or host, as camera.valid_rays_mask returns it; None = every
    pixel.  Keeps ``val_inds`` = torch.nonzero(rays_msk).squeeze(1) (int64, on the device) and ``n_valid`` (host int)."""

    def __init__(self, H, W, focal, center, c2w, near, far, idx, rays_msk=None, device="cuda"):
        H, W = int(H), int(W)
        if H < 0 or W < 0 or H * W >= 2 ** 31:
            raise RuntimeError(f"moco_flow_amd.batch.FrameRays: H={H} W={W}; needs 0 <= H W < 2^31")
        _check_mask(rays_msk, H, W)
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("moco_flow_amd.batch.FrameRays: this is the MI355X (HIP) path; no CPU implementation")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.H, self.W, self.device = H, W, dev
        a = L.mf_ray_batch_args()
        a.H, a.W = H, W
        a.focal, a.cx, a.cy = float(np.float32(focal)), float(np.float32(center[0])), float(np.float32(center[1]))
        a.has_c2w = int(c2w is not None)
        if c2w is not None:
            m = np.asarray(c2w, dtype=np.float64)[:3, :4].astype(np.float32)      # camera.py:141 .float()
            a.c2w = (C.c_float * 12)(*m.reshape(-1).tolist())
        a.nearv, a.farv, a.idx = float(np.float32(near)), float(np.float32(far)), float(np.float32(idx))
        self._args = a
        n = H * W
        if n == 0:
            self.val_inds, self.n_valid = torch.empty(0, dtype=torch.int64, device=dev), 0
            return
        mask = None
        if rays_msk is not None:
            mask = rays_msk.to(dev).contiguous()
            mask = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
        inds = torch.empty(n, dtype=torch.int64, device=dev)
        count = torch.empty(1, dtype=torch.int64, device=dev)
        scratch = L.scratch(dev, "mf_mask_compact_scratch_bytes", n)
        L.launch(dev, "mf_mask_compact", L.ptr(mask), n, inds.data_ptr(), count.data_ptr(), scratch.data_ptr())
        self.n_valid = int(count.item())                    # the one device -> host read of a frame
        self.val_inds = inds if self.n_valid == n else inds[:self.n_valid].clone()     # keep 8 n_valid bytes, not 8 H W

    def resident_bytes(self):
        """Device bytes this frame keeps between steps (val_inds; the image and background are the caller's)."""
        return self.val_inds.numel() * self.val_inds.element_size()

    def sample(self, N_rand, image=None, background=None, perm=None, chain_idx=None, generator=None):
        """-> (rays (n, 9 | 10), rgbs (n, 3) | None, background (n, 3) | None, sel_inds (n,) int64), n = min(N_rand, n_valid).

        perm: int64 device tensor of >= n positions into val_inds -- the reference's torch.randperm(n_valid)[:N_rand]; None
        draws torch.randperm(n_valid, device=..., generator=generator).  sel_inds = val_inds[perm[:n]]; row k of rays is row
        sel_inds[k] of camera.make_rays(...) bit for bit, with column 9 = float32(chain_idx) when chain_idx is given.
        image: (H W, 3) fp32 rows (gathered), (H, W, 3) uint8 (u8.float() / 255 as the device evaluates it), (H, W, 4) uint8 RGBA
        (composited over the background, moco_flow_dataset.py:174), or None.  background: (H W, 3) fp32 rows, one (3,) fp32 colour, or None.
        An entry of perm outside [0, n_valid) is not dereferenced: its rows come back NaN and its sel_inds entry -1 (checking
        a device permutation would cost a synchronisation).  No host synchronisation."""
        N_rand = int(N_rand)
        if N_rand < 0:
            raise RuntimeError(f"moco_flow_amd.batch.FrameRays.sample: N_rand={N_rand}")
        H, W, dev = self.H, self.W, self.device
        image_kind = _image_kind(image, H, W)
        background_kind = _background_kind(background, H, W)
        if image_kind == L.MF_IMAGE_U8_RGBA and background_kind == L.MF_BACKGROUND_NONE:
            raise RuntimeError("moco_flow_amd.batch.FrameRays.sample: an RGBA image needs a background to composite over")
        for name, t in (("image", image), ("background", background)):
            if t is not None and t.device != dev:
                raise RuntimeError(f"moco_flow_amd.batch.FrameRays.sample: {name} is on {t.device}, the frame on {dev}")
        n = min(N_rand, self.n_valid)
        if perm is not None:
            _check_perm(perm, n, dev)
        cols = 9 if chain_idx is None else 10
        rays = torch.empty((n, cols), dtype=torch.float32, device=dev)
        rgbs = None if image is None else torch.empty((n, 3), dtype=torch.float32, device=dev)
        bkgd = None if background is None else torch.empty((n, 3), dtype=torch.float32, device=dev)
        sel = torch.empty(n, dtype=torch.int64, device=dev)
        if n == 0:                                         # nothing to launch
            return rays, rgbs, bkgd, sel
        if perm is None:
            perm = torch.randperm(self.n_valid, device=dev, generator=generator)
        perm = perm.contiguous()
        image = None if image is None else image.contiguous()
        background = None if background is None else background.contiguous()
        a = L.mf_ray_batch_args()
        C.memmove(C.byref(a), C.byref(self._args), C.sizeof(a))
        a.has_chain = int(chain_idx is not None)
        a.chain_idx = 0.0 if chain_idx is None else float(np.float32(chain_idx))
        a.val_inds, a.n_valid = self.val_inds.data_ptr(), self.n_valid
        a.perm, a.n_rows = perm.data_ptr(), n
        a.image, a.image_kind = L.ptr(image), image_kind
        a.background, a.background_kind = L.ptr(background), background_kind
        a.rays_out, a.rgbs_out, a.background_out, a.sel_out = rays.data_ptr(), L.ptr(rgbs), L.ptr(bkgd), sel.data_ptr()
        L.launch(dev, "mf_ray_batch", C.byref(a))
        return rays, rgbs, bkgd, sel
