"""Pictures on the device (reference: utils/vis_utils.py:28-43 ``visualize_depth``; trainer_moco_flow.py:475-482
``decode_results``; the sheets of visualize_frame / visualize_video, trainer_moco_flow.py:609-623, 644-659):

    visualize_depth   the reference's signature; depth plane -> (3, H, W) fp32 colours, on the device, no host sync
    decode_results    the trainer's method as a function
    frame_sheet       [gt | pred | depth | novel pred | novel depth] as 8-bit pixels ready for an encoder, from the rendered
                      rows in one mf_frame_sheet launch (plus one mf_depth_range per depth panel)
    write_png         a host-side 8-bit RGB PNG writer on zlib and struct alone

The reference colours depth with ``cv2.applyColorMap(x, cv2.COLORMAP_JET)``.  OPENCV RESTATED: cv2 is not available to this
project; ``colormap_lut`` restates OpenCV's Jet table from its closed form and is UNPINNED AGAINST cv2 ITSELF (as the kornia
functions of oracle/kornia_restated.py and mf_ssim are against kornia).  A caller who has cv2 pins it by passing
``cv2.applyColorMap(np.arange(256, dtype=np.uint8)[:, None], cmap)[:, 0]`` as ``cmap``.

The index arithmetic is the reference's fp32 arithmetic operation for operation (include/mocoflow_hip.h); its one deviation:
where ``astype(np.uint8)`` is undefined (255 x outside [0, 256) or NaN) the index is clamped to 0 .. 255.

No gradients.  Everything runs on the current stream of the inputs' device."""
import struct
import zlib

import torch

from . import _lib as L

__all__ = ["COLORMAP_JET", "colormap_lut", "visualize_depth", "decode_results", "frame_sheet", "write_png"]

COLORMAP_JET = 2          # cv2.COLORMAP_JET

_lut_host = {}
_lut_device = {}


def colormap_lut(cmap=COLORMAP_JET):
    """The (256, 3) uint8 host table of a colour map: entry i colours index i, column c becomes channel c of the picture.

    OPENCV RESTATED, UNPINNED AGAINST cv2 ITSELF.  Jet, with x = i / 255, in float64:
        r = clamp(min(4x - 1.5, 4.5 - 4x), 0, 1)   g = clamp(min(4x - 0.5, 3.5 - 4x), 0, 1)   b = clamp(min(4x + 0.5, 2.5 - 4x), 0, 1)
    each scaled by 255 and rounded to nearest, ties to even.  Channel order is the reference's quirk: applyColorMap returns
    BGR and Image.fromarray reads it as RGB, so column 0 -- channel 0 of visualize_depth's result -- is the b curve and
    column 2 the r curve.  Any other cmap integer raises NotImplementedError; a (256, 3) uint8 tensor is returned as it is."""
    if isinstance(cmap, torch.Tensor):
        if cmap.dtype != torch.uint8 or tuple(cmap.shape) != (256, 3):
            raise RuntimeError(f"moco_flow_amd.vis: a colour table must be a (256, 3) uint8 tensor, got {tuple(cmap.shape)} {cmap.dtype}")
        return cmap
    if isinstance(cmap, bool) or not isinstance(cmap, int) or cmap != COLORMAP_JET:
        raise NotImplementedError(f"moco_flow_amd.vis: colour map {cmap!r} is not built; COLORMAP_JET ({COLORMAP_JET}) or a "
                                  "(256, 3) uint8 table")
    if cmap not in _lut_host:
        x = torch.arange(256, dtype=torch.float64) / 255
        curve = lambda up, down: torch.minimum(4 * x + up, down - 4 * x).clamp(0, 1)
        r, g, b = curve(-1.5, 4.5), curve(-0.5, 3.5), curve(0.5, 2.5)
        _lut_host[cmap] = torch.round(torch.stack([b, g, r], dim=1) * 255).to(torch.uint8)     # torch.round: ties to even
    return _lut_host[cmap]


def _device_lut(cmap, device):
    """The table on `device`: built-in maps are uploaded once per device; a caller's table is taken where it lies (pass a
    device tensor to keep the upload out of the call)."""
    if isinstance(cmap, torch.Tensor):
        return colormap_lut(cmap).to(device).contiguous()
    key = (cmap, device)
    if key not in _lut_device:
        _lut_device[key] = colormap_lut(cmap).to(device)
    return _lut_device[key]


def _plane(depth, what):
    L.require_gpu(depth, what)
    return depth.detach().float().contiguous()     # a strided view is copied once


def _range_into(out2, plane, mi, ma):
    """Fill the device fp32 pair out2 = [mi, ma] as vis_utils.py:33-38 chooses it; returns nan_value."""
    if mi is not None and ma is not None:
        for slot, v in ((out2[0], mi), (out2[1], ma)):
            if isinstance(v, torch.Tensor):
                slot.copy_(v.detach().reshape(()))
            else:
                slot.fill_(float(v))
        return float(ma)
    n = plane.numel()
    scratch = L.scratch(plane.device, "mf_depth_range_scratch_bytes", n)
    L.launch(plane.device, "mf_depth_range", plane.data_ptr(), n, 0.0, out2.data_ptr(), scratch.data_ptr())
    return 0.0


def visualize_depth(depth, mi=None, ma=None, cmap=COLORMAP_JET):
    """vis_utils.py:28-43.  depth: (H, W) device tensor -> (3, H, W) fp32 on the same device.  With both mi and ma given
    they are the range and NaN becomes ma; otherwise NaN becomes 0 and the range is the plane's min and max (mf_depth_range).
    mi / ma are Python numbers (taken as fp32, as the device holds the range).  No host sync; capturable in a graph once
    the table is on the device (the first call per device uploads it)."""
    plane = _plane(depth, "visualize_depth")
    if plane.dim() != 2:
        raise RuntimeError(f"moco_flow_amd.visualize_depth: depth must be (H, W), got shape {tuple(plane.shape)}")
    dev = plane.device
    lut = _device_lut(cmap, dev)
    range2 = torch.empty(2, dtype=torch.float32, device=dev)
    nan_value = _range_into(range2, plane, mi, ma)
    out = torch.empty((3,) + tuple(plane.shape), dtype=torch.float32, device=dev)
    L.launch(dev, "mf_depth_colormap", plane.data_ptr(), plane.numel(), range2.data_ptr(), nan_value, lut.data_ptr(), out.data_ptr())
    return out


def decode_results(results, img_size):
    """trainer_moco_flow.py:475-482: (img_ori (H W, 3), img_pred (3, H, W) view, depth_ori (H W), depth_pred (3, H, W))."""
    H, W = img_size
    typ = 'fine' if 'rgb_fine' in results else 'coarse'
    img_ori = results['rgb_%s' % typ]
    img_pred = img_ori.view(H, W, 3).permute(2, 0, 1)
    depth_ori = results['depth_%s' % typ]
    depth_pred = visualize_depth(depth_ori.view(H, W))
    return img_ori, img_pred, depth_ori, depth_pred


def frame_sheet(panels, H, W, planar=False, cmap=COLORMAP_JET):
    """The sheet visualize_frame / visualize_video assemble, as pixels: panels side by side along the width.

    panels: a list of (H W, 3) row tensors (rendered rgb as render_rays / render_image return it, or ground-truth rgbs) and
    (H W,) / (H, W) depth tensors; a depth panel may be the tuple (depth, mi, ma) -- the range rule of visualize_depth, per
    panel.  At most 8.  Returns the (H, k W, 3) uint8 device tensor, quantised as torchvision's save_image does; with
    planar=True also the float (3, H, k W) stack the trainer hands to tb.add_image.  One mf_depth_range per depth panel
    without a range and ONE mf_frame_sheet; no permute, no float intermediate, no host sync."""
    if len(panels) < 1 or len(panels) > L.MF_SHEET_MAX_PANELS:
        raise RuntimeError(f"moco_flow_amd.frame_sheet: {len(panels)} panels, must be from 1 to {L.MF_SHEET_MAX_PANELS}")
    k = len(panels)
    items = (L.mf_sheet_panel * k)()
    keep, dev, range2s = [], None, None
    for j, entry in enumerate(panels):
        t, mi, ma = entry if isinstance(entry, (tuple, list)) else (entry, None, None)
        t = _plane(t, "frame_sheet")
        if dev is None:
            dev = t.device
            range2s = torch.zeros((k, 2), dtype=torch.float32, device=dev)
        elif t.device != dev:
            raise RuntimeError(f"moco_flow_amd.frame_sheet: panels on {dev} and {t.device}")
        if t.dim() == 2 and tuple(t.shape) == (H * W, 3) and mi is None and ma is None:
            kind, nan_value = L.MF_PANEL_RGB, 0.0
        elif tuple(t.shape) in ((H * W,), (H, W)):
            kind, nan_value = L.MF_PANEL_DEPTH, _range_into(range2s[j], t, mi, ma)
        else:
            raise RuntimeError(f"moco_flow_amd.frame_sheet: panel {j} has shape {tuple(t.shape)}; rgb rows are ({H * W}, 3), "
                               f"a depth plane is ({H * W},) or ({H}, {W})")
        keep.append(t)
        items[j].rows, items[j].kind, items[j].nan_value = t.data_ptr(), kind, nan_value
    lut = _device_lut(cmap, dev)
    sheet = torch.empty((H, k * W, 3), dtype=torch.uint8, device=dev)
    stack = torch.empty((3, H, k * W), dtype=torch.float32, device=dev) if planar else None
    if H * W == 0:                       # nothing to launch (and an empty tensor has no pointer to pass)
        return (sheet, stack) if planar else sheet
    L.launch(dev, "mf_frame_sheet", items, k, H, W, range2s.data_ptr(), lut.data_ptr(), sheet.data_ptr(), L.ptr(stack))
    return (sheet, stack) if planar else sheet


def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)


def write_png(path, sheet_u8, compress_level=6):
    """Write an (H, W, 3) uint8 tensor (frame_sheet's; device or host) as an 8-bit RGB PNG: filter 0 on every row, one IDAT
    chunk, stdlib zlib and struct only.  This is the one point of the picture path that copies to the host."""
    if sheet_u8.dtype != torch.uint8 or sheet_u8.dim() != 3 or sheet_u8.shape[2] != 3 or sheet_u8.shape[0] < 1 or sheet_u8.shape[1] < 1:
        raise RuntimeError(f"moco_flow_amd.write_png: needs an (H, W, 3) uint8 tensor with H, W >= 1, got {tuple(sheet_u8.shape)} {sheet_u8.dtype}")
    H, W = int(sheet_u8.shape[0]), int(sheet_u8.shape[1])
    rows = sheet_u8.detach().cpu().contiguous().view(H, W * 3)
    raw = torch.cat([torch.zeros((H, 1), dtype=torch.uint8), rows], dim=1).numpy().tobytes()      # filter byte 0 per row
    png = (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0))
           + _chunk(b"IDAT", zlib.compress(raw, compress_level)) + _chunk(b"IEND", b""))
    with open(path, "wb") as fh:
        fh.write(png)
