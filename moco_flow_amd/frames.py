"""Frame ingest on the device: from decoded 8-bit frames to the tensors ``batch.FrameRays.sample``, ``metrics.image_metrics`` and
``vis.frame_sheet`` take (reference: datasets/moco_flow_dataset.py:45, 51-55, 169-176; scripts/data_utils.py:150-163).

    resize            ``T.Resize(size)`` on the PIL image -- PIL's antialiased bilinear resample, bit for bit (mf_resize_u8)
    composite         ``img[:3] * a + bkgd * (1 - a)`` over the whole frame -> (H W, 3) fp32 rows (mf_composite_rows); row p is the
                      row FrameRays.sample returns for pixel p, bit for bit
    to_rows           an (H, W, 3) byte image as (H W, 3) fp32 rows, ``u8.float() / 255`` as the device evaluates it
    background_plate  ``generate_background_image``: per pixel and channel the k-th smallest of img (1 - msk) over the frames, as
                      bytes (mf_background_plate) -- without the reference's float64 copy of every frame and its np.sort
    clean_mask        the matte background_plate takes, from the raw alpha: threshold at 196, keep the largest connected region
                      (scripts/data_utils.py:135-147, find_max_region :102-114), optionally fill its holes (mf_mask_label,
                      mf_mask_select, mf_mask_fill_holes) -- a contract of its own in exact integers, not cv2's contour tracing
    mask_regions      the regions themselves: labels, and the table of areas and bounding boxes (mf_mask_table_count / _emit)

Everything is integer arithmetic on bytes or fp32 rounded once per operation, so every result is pinned exactly.  The resize
coefficients are built here on the host in float64, as PIL's precompute_coeffs builds them, and uploaded once per size pair and
device.  No gradients; everything runs on the current stream of the inputs' device.  CPU tensors raise: there is no host path."""
import collections
import math

import numpy as np
import torch

from . import _lib as L

__all__ = ["resize", "composite", "to_rows", "background_plate", "resize_tables", "plate_index", "clean_mask", "mask_regions",
           "Regions"]

_PRECISION_BITS = 22           # PIL's PRECISION_BITS = 32 - 8 - 2
_INDEX_LIMIT = 2 ** 31         # the kernels index with 32 bits: a call stays below this many bytes per image stack
_tables_host = {}
_tables_device = {}


def resize_tables(n_in, n_out):
    """PIL's precompute_coeffs + normalize_coeffs_8bpc for the bilinear (triangle, support 1) filter along one axis of n_in ->
    n_out pixels, in float64: (bounds (n_out, 2) int32 = [first tap, tap count], kk (n_out, ksize) int32, ksize).  The taps of
    one output index are summed in order, as the C loop sums them (a pairwise sum differs in the last bit)."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise RuntimeError(f"moco_flow_amd.frames.resize_tables: n_in={n_in} n_out={n_out}; both must be >= 1")
    key = (n_in, n_out)
    if key not in _tables_host:
        scale = n_in / n_out
        fs = max(scale, 1.0)
        support = 1.0 * fs
        ksize = int(math.ceil(support)) * 2 + 1
        ss = 1.0 / fs
        center = (np.arange(n_out, dtype=np.float64) + 0.5) * scale
        first = np.maximum((center - support + 0.5).astype(np.int64), 0)                 # (int): truncation towards zero
        count = np.minimum((center + support + 0.5).astype(np.int64), n_in) - first
        w = np.zeros((n_out, ksize), dtype=np.float64)
        ww = np.zeros(n_out, dtype=np.float64)
        for x in range(ksize):
            arg = np.abs(((x + first) - center + 0.5) * ss)
            w[:, x] = np.where((x < count) & (arg < 1.0), 1.0 - arg, 0.0)
            ww = ww + w[:, x]
        nz = ww != 0.0
        w[nz] = w[nz] / ww[nz, None]
        kk = (0.5 + w * float(1 << _PRECISION_BITS)).astype(np.int64).astype(np.int32)    # the weights are >= 0: truncation
        bounds = np.stack([first, count], axis=1).astype(np.int32)
        _tables_host[key] = (bounds, kk, ksize)
    return _tables_host[key]


def _device_tables(n_in, n_out, device):
    key = (n_in, n_out, device)
    if key not in _tables_device:
        bounds, kk, ksize = resize_tables(n_in, n_out)
        _tables_device[key] = (torch.from_numpy(bounds).to(device), torch.from_numpy(kk).to(device), ksize)
    return _tables_device[key]


def _check_u8(t, what, name):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
        got = f"{tuple(t.shape)} {t.dtype}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise RuntimeError(f"moco_flow_amd.frames.{what}: {name} must be a uint8 tensor, got {got}")
    L.require_gpu(t, f"frames.{what}")


def resize(images, size):
    """images: (H0, W0, C) or (F, H0, W0, C) uint8 on the device, C in {1, 3, 4}; size: (H, W), as the YAML's img_size gives it
    (an int -- torchvision's "shorter side" -- raises).  Returns uint8 of the same rank, equal to
    ``Image.fromarray(a).resize((W, H), Image.BILINEAR)`` of PIL 12 per frame, bit for bit; RGBA is resampled premultiplied as
    PIL does (the identity returns the input's bytes).  A stack is resized in chunks of frames that keep every call inside
    32-bit indexing."""
    if isinstance(size, (int, np.integer)) or not isinstance(size, (tuple, list)) or len(size) != 2:
        raise RuntimeError(f"moco_flow_amd.frames.resize: size must be (H, W), got {size!r}")
    _check_u8(images, "resize", "images")
    H, W = int(size[0]), int(size[1])
    if images.dim() not in (3, 4) or images.shape[-1] not in (1, 3, 4):
        raise RuntimeError(f"moco_flow_amd.frames.resize: images is {tuple(images.shape)}; (H0, W0, C) or (F, H0, W0, C) with C in "
                           "{1, 3, 4}")
    stack = images if images.dim() == 4 else images.unsqueeze(0)
    F, H0, W0, C = (int(v) for v in stack.shape)
    if H < 0 or W < 0 or (F * H * W > 0 and H0 * W0 == 0):
        raise RuntimeError(f"moco_flow_amd.frames.resize: ({H0}, {W0}) -> ({H}, {W})")
    dev = stack.device
    out = torch.empty((F, H, W, C), dtype=torch.uint8, device=dev)
    if out.numel() == 0:                                    # nothing to launch
        return out if images.dim() == 4 else out[0]
    per_frame = max(H0 * W0, H0 * W, H * W) * C
    if per_frame >= _INDEX_LIMIT:
        raise RuntimeError(f"moco_flow_amd.frames.resize: one ({H0}, {W0}, {C}) -> ({H}, {W}) frame needs more than 32-bit indexing")
    stack = stack.contiguous()
    xb, xk, xks = _device_tables(W0, W, dev) if W != W0 else (None, None, 0)
    yb, yk, yks = _device_tables(H0, H, dev) if H != H0 else (None, None, 0)
    chunk = max(1, min(F, (_INDEX_LIMIT - 1) // per_frame))
    scratch = L.scratch(dev, "mf_resize_u8_scratch_bytes", chunk, H0, W0, C, H, W) if W != W0 and H != H0 else None
    with torch.cuda.device(dev):
        for f0 in range(0, F, chunk):
            n = min(chunk, F - f0)
            L.enqueue(dev, "mf_resize_u8", stack[f0].data_ptr(), n, H0, W0, C, H, W, L.ptr(xb), L.ptr(xk), xks, L.ptr(yb), L.ptr(yk),
                      yks, out[f0].data_ptr(), L.ptr(scratch))
    return out if images.dim() == 4 else out[0]


def _composite_background(background, H, W):
    """MF_BACKGROUND_* of `background`: None, (H W, 3) fp32 rows, one (3,) fp32 colour, or an (H, W, 3) uint8 image."""
    if background is None:
        return L.MF_BACKGROUND_NONE
    if not isinstance(background, torch.Tensor):
        raise RuntimeError(f"moco_flow_amd.frames.composite: background must be a tensor, got {type(background).__name__}")
    shape = tuple(background.shape)
    if background.dtype == torch.float32 and shape == (H * W, 3):
        kind = L.MF_BACKGROUND_ROWS
    elif background.dtype == torch.float32 and shape == (3,):
        kind = L.MF_BACKGROUND_COLOUR
    elif background.dtype == torch.uint8 and shape == (H, W, 3):
        kind = L.MF_BACKGROUND_U8
    else:
        raise RuntimeError(f"moco_flow_amd.frames.composite: background is {shape} {background.dtype}; fp32 rows ({H * W}, 3), one "
                           f"fp32 colour (3,) or a uint8 image ({H}, {W}, 3)")
    L.require_gpu(background, "frames.composite")
    return kind


def composite(image, background=None):
    """image: (H, W, 4) uint8 RGBA on the device, composited over `background` -- (H W, 3) fp32 rows, one (3,) fp32 colour or an
    (H, W, 3) uint8 image such as background_plate's (read as u8 / 255) -- as moco_flow_dataset.py:174 does; or (H, W, 3) uint8
    without a background: u8 / 255.  Returns the (H W, 3) fp32 rows that metrics.image_metrics and vis.frame_sheet take; row p is
    what FrameRays.sample(image=image, background=...) returns for pixel p, bit for bit."""
    _check_u8(image, "composite", "image")
    if image.dim() != 3 or image.shape[2] not in (3, 4):
        raise RuntimeError(f"moco_flow_amd.frames.composite: image is {tuple(image.shape)}; (H, W, 4) RGBA or (H, W, 3) RGB")
    H, W, C = (int(v) for v in image.shape)
    if H * W * 4 >= _INDEX_LIMIT:
        raise RuntimeError(f"moco_flow_amd.frames.composite: H={H} W={W}; needs 4 H W < 2^31")
    kind = _composite_background(background, H, W)
    if C == 4 and kind == L.MF_BACKGROUND_NONE:
        raise RuntimeError("moco_flow_amd.frames.composite: an RGBA image needs a background to composite over")
    if C == 3 and kind != L.MF_BACKGROUND_NONE:
        raise RuntimeError("moco_flow_amd.frames.composite: an RGB image has no alpha: it takes no background")
    dev = image.device
    if background is not None and background.device != dev:
        raise RuntimeError(f"moco_flow_amd.frames.composite: background is on {background.device}, the image on {dev}")
    rows = torch.empty((H * W, 3), dtype=torch.float32, device=dev)
    if H * W == 0:
        return rows
    image = image.contiguous()
    background = None if background is None else background.contiguous()
    L.launch(dev, "mf_composite_rows", image.data_ptr(), L.MF_IMAGE_U8_RGBA if C == 4 else L.MF_IMAGE_U8_RGB, H, W,
             L.ptr(background), kind, rows.data_ptr())
    return rows


def to_rows(image_u8):
    """An (H, W, 3) uint8 image on the device -> (H W, 3) fp32 rows, u8 * (1.0f / 255.0f): a plate or a resized background as
    FrameRays.sample's `background`."""
    _check_u8(image_u8, "to_rows", "image_u8")
    if image_u8.dim() != 3 or image_u8.shape[2] != 3:
        raise RuntimeError(f"moco_flow_amd.frames.to_rows: image_u8 is {tuple(image_u8.shape)}; (H, W, 3)")
    return composite(image_u8)


_PLATE_PATHS = {"auto": L.MF_PLATE_AUTO, "staged": L.MF_PLATE_STAGED, "streamed": L.MF_PLATE_STREAMED}


def plate_index(F, q=0.8):
    """k = int(F * q), the reference's int(num_images * 0.8) (data_utils.py:162); RuntimeError unless 1 <= F < 65536 and
    0 <= k < F."""
    F = int(F)
    if F < 1 or F >= 65536:
        raise RuntimeError(f"moco_flow_amd.frames.background_plate: F={F}; needs 1 <= F < 65536")
    k = int(F * q)
    if not 0 <= k < F:
        raise RuntimeError(f"moco_flow_amd.frames.background_plate: q={q} gives k={k}; needs 0 <= k < F={F}")
    return k


def background_plate(frames, masks, q=0.8, path="auto"):
    """scripts/data_utils.py:150-163.  frames: (F, H, W, 3 | 4) uint8 on the device (an alpha channel is ignored); masks: (F, H,
    W) uint8, 255 = foreground.  Returns the (H, W, 3) uint8 plate: per pixel and channel the k-th smallest, k = int(F * q) (the
    reference's int(num_images * 0.8)), of u (255 - m) over the frames, as (key + 127) // 255 -- floor(255 x + 0.5) of the
    reference's float64 value.  RuntimeError unless 0 <= k < F.  path: "auto" stages the keys in LDS while F fits and streams
    the frames beyond that; "staged" / "streamed" force one (the results are identical)."""
    _check_u8(frames, "background_plate", "frames")
    _check_u8(masks, "background_plate", "masks")
    if frames.dim() != 4 or frames.shape[3] not in (3, 4):
        raise RuntimeError(f"moco_flow_amd.frames.background_plate: frames is {tuple(frames.shape)}; (F, H, W, 3) or (F, H, W, 4)")
    F, H, W, C = (int(v) for v in frames.shape)
    if tuple(masks.shape) != (F, H, W):
        raise RuntimeError(f"moco_flow_amd.frames.background_plate: masks is {tuple(masks.shape)}; ({F}, {H}, {W})")
    if masks.device != frames.device:
        raise RuntimeError(f"moco_flow_amd.frames.background_plate: masks is on {masks.device}, the frames on {frames.device}")
    if path not in _PLATE_PATHS:
        raise RuntimeError(f"moco_flow_amd.frames.background_plate: path={path!r}; one of {sorted(_PLATE_PATHS)}")
    k = plate_index(F, q)
    if H * W * 4 >= _INDEX_LIMIT:
        raise RuntimeError(f"moco_flow_amd.frames.background_plate: H={H} W={W}; needs 4 H W < 2^31")
    dev = frames.device
    out = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    if H * W == 0:
        return out
    frames, masks = frames.contiguous(), masks.contiguous()
    L.launch(dev, "mf_background_plate", frames.data_ptr(), masks.data_ptr(), F, H, W, C, k, _PLATE_PATHS[path], out.data_ptr())
    return out


Regions = collections.namedtuple("Regions", ["labels", "counts", "table"])

# bytes of device memory (the labels and the kernels' scratch: 12 per pixel) that clean_mask / mask_regions hold per chunk of frames
SCRATCH_BUDGET = 1 << 30
_REGION_BYTES_PER_PIXEL = 12


def _alpha_plane(alpha, what):
    """(tensor to keep alive, address of pixel 0, pixel stride in bytes, F, H, W, single image) of the alpha argument of
    clean_mask / mask_regions.  A contiguous RGBA stack, or its channel view ``rgba[..., c]``, is read in place with stride 4."""
    _check_u8(alpha, what, "alpha")
    shape = tuple(int(v) for v in alpha.shape)
    rgba = alpha.dim() == 4 or (alpha.dim() == 3 and shape[-1] == 4)
    if alpha.dim() not in (2, 3, 4) or (alpha.dim() == 4 and shape[-1] != 4):
        raise RuntimeError(f"moco_flow_amd.frames.{what}: alpha is {shape}; (H, W) or (F, H, W) bytes, or (H, W, 4) / (F, H, W, 4) RGBA")
    single = alpha.dim() == (3 if rgba else 2)
    stack = alpha.unsqueeze(0) if single else alpha
    F, H, W = (int(v) for v in stack.shape[:3])
    if H * W >= _INDEX_LIMIT:
        raise RuntimeError(f"moco_flow_amd.frames.{what}: H={H} W={W}; needs H W < 2^31")
    if rgba:
        stack = stack.contiguous()
        return stack, stack.data_ptr() + 3, 4, F, H, W, single
    if F * H * W > 0 and not stack.is_contiguous() and tuple(stack.stride()) == (4 * H * W, 4 * W, 4):
        return stack, stack.data_ptr(), 4, F, H, W, single              # a channel of a contiguous RGBA stack
    stack = stack.contiguous()
    return stack, stack.data_ptr(), 1, F, H, W, single


def _region_args(what, thres, connectivity=8, min_area=0):
    if isinstance(thres, bool) or not isinstance(thres, (int, np.integer)) or not 0 <= int(thres) <= 256:
        raise RuntimeError(f"moco_flow_amd.frames.{what}: thres={thres!r}; an integer in [0, 256]")
    if connectivity not in (4, 8):
        raise RuntimeError(f"moco_flow_amd.frames.{what}: connectivity={connectivity!r}; 4 or 8")
    if isinstance(min_area, bool) or not isinstance(min_area, (int, np.integer)) or int(min_area) < 0:
        raise RuntimeError(f"moco_flow_amd.frames.{what}: min_area={min_area!r}; an integer >= 0")


def _region_chunk(F, H, W):
    """frames per call: inside the scratch budget and 32-bit indexing, at least one"""
    hw = max(H * W, 1)
    return max(1, min(F, (_INDEX_LIMIT - 1) // hw, SCRATCH_BUDGET // (_REGION_BYTES_PER_PIXEL * hw)))


def clean_mask(alpha, thres=196, largest=True, min_area=0, fill_holes=False):
    """scripts/data_utils.py:135-147 on the device.  alpha: (H, W) or (F, H, W) uint8, or (H, W, 4) / (F, H, W, 4) RGBA whose
    channel 3 is read in place (a 3-D tensor whose last dimension is 4 is RGBA).  Returns uint8 {0, 255} of shape (H, W) /
    (F, H, W): 255 where alpha >= thres and the pixel's 8-connected region has at least min_area pixels and, with `largest`, is
    the frame's largest (most pixels; ties go to the region that starts first in row-major order).  fill_holes: the zeros that
    no 4-connected path of zeros joins to the frame's border become 255.  A frame without a member gives zeros (the reference
    raises there, on np.argmax of an empty list).  This is what background_plate takes as `masks` and what
    ``raw[..., 3] = mask`` (:146) writes back.
    Not cv2's result in two documented ways: area is the pixel count, not contourArea's polygon area, and
    the one-pixel ring that the reference erases around every hole of the kept region is kept.
    Runs on the current stream without a host synchronisation; a stack goes through in chunks of frames under SCRATCH_BUDGET."""
    _region_args("clean_mask", thres, 8, min_area)
    stack, ptr, stride, F, H, W, single = _alpha_plane(alpha, "clean_mask")
    dev = stack.device
    out = torch.empty((F, H, W), dtype=torch.uint8, device=dev)
    if out.numel() > 0:
        chunk = _region_chunk(F, H, W)
        scratch = L.scratch(dev, "mf_mask_label_scratch_bytes", chunk, H, W)
        labels = torch.empty((chunk, H, W), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            for f0 in range(0, F, chunk):
                n = min(chunk, F - f0)
                L.enqueue(dev, "mf_mask_label", ptr + f0 * H * W * stride, stride, n, H, W, int(thres), 0, 8, labels.data_ptr(),
                          scratch.data_ptr())
                L.enqueue(dev, "mf_mask_select", labels.data_ptr(), n, H, W, int(bool(largest)), int(min_area), out[f0].data_ptr(),
                          scratch.data_ptr())
                if fill_holes:
                    L.enqueue(dev, "mf_mask_fill_holes", out[f0].data_ptr(), n, H, W, scratch.data_ptr())
    return out[0] if single else out


def mask_regions(alpha, thres=196, connectivity=8, below=False):
    """The connected regions of ``alpha >= thres`` (below: ``alpha < thres``) per frame; alpha as clean_mask takes it.  Returns
    Regions(labels, counts, table): labels int32 (H, W) / (F, H, W), the smallest row-major index y W + x of the pixel's region
    within its frame, -1 off the members; counts (F,) int64, the regions of each frame; table (sum counts, 7) int32 with rows
    (frame, label, area, x0, y0, x1, y1), bounds inclusive, in (frame, label) order.  One host read: the counts, which size the
    table."""
    _region_args("mask_regions", thres, connectivity)
    stack, ptr, stride, F, H, W, single = _alpha_plane(alpha, "mask_regions")
    dev = stack.device
    labels = torch.empty((F, H, W), dtype=torch.int32, device=dev)
    counts = torch.zeros((F,), dtype=torch.int64, device=dev)
    if labels.numel() == 0:
        return Regions(labels[0] if single else labels, counts, torch.empty((0, 7), dtype=torch.int32, device=dev))
    chunk = _region_chunk(F, H, W)
    scratch = L.scratch(dev, "mf_mask_label_scratch_bytes", chunk, H, W)
    with torch.cuda.device(dev):
        for f0 in range(0, F, chunk):
            n = min(chunk, F - f0)
            L.enqueue(dev, "mf_mask_label", ptr + f0 * H * W * stride, stride, n, H, W, int(thres), int(bool(below)),
                      int(connectivity), labels[f0].data_ptr(), scratch.data_ptr())
            L.enqueue(dev, "mf_mask_table_count", labels[f0].data_ptr(), n, H, W, counts[f0:].data_ptr())
        host = counts.cpu().numpy()                                       # the one host read
        table = torch.empty((int(host.sum()), 7), dtype=torch.int32, device=dev)
        row = 0
        for f0 in range(0, F, chunk):
            n = min(chunk, F - f0)
            c = int(host[f0:f0 + n].sum())
            if c > 0:
                L.enqueue(dev, "mf_mask_table_emit", labels[f0].data_ptr(), n, H, W, f0, c, table[row:].data_ptr(), scratch.data_ptr())
            row += c
    return Regions(labels[0] if single else labels, counts, table)
