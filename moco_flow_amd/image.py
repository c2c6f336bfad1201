"""Full-image chunk driver on the device: the ``render`` method of the reference's
trainers (trainer/trainer_moco_flow.py:226-268, trainer/trainer_nerf.py:100-140) without its host
round trips -- the valid-ray selection, the per-chunk loop and the foreground scatter-back all stay in
GPU memory (the reference indexes with numpy masks and pulls ``opacity`` to the host, :255)."""
from __future__ import annotations

import ctypes as C
from typing import Callable, Dict, Optional

import torch

from . import _lib as L


def compose_image(rays_msk: Optional[torch.Tensor], opacity, rgb, depth, background):
    """mf_image_compose: (img (B,3), depth (B,)) from the rendered rays' colour / depth / opacity."""
    L.require_gpu(background, "image.compose_image")
    dev = background.device
    B = background.shape[0]
    img = torch.empty((B, 3), device=dev, dtype=torch.float32)
    dep = torch.empty((B,), device=dev, dtype=torch.float32)
    msk8 = rank = None
    if rays_msk is not None:
        m = torch.as_tensor(rays_msk, device=dev).reshape(-1).bool()
        msk8 = m.to(torch.uint8).contiguous()
        rank = (torch.cumsum(m.to(torch.int64), 0) - 1).contiguous()
    f = lambda t: t.detach().contiguous().float()
    opacity, rgb, depth, bgc = f(opacity), f(rgb), f(depth), f(background)
    L.launch(dev, "mf_image_compose", L.ptr(msk8), L.ptr(rank), B, opacity.data_ptr(), rgb.data_ptr(), depth.data_ptr(),
             bgc.data_ptr(), img.data_ptr(), dep.data_ptr())
    return img, dep


def render_image(rays, background, render: Callable[..., Dict[str, torch.Tensor]], N_rand: int,
                 rays_msk=None, occupancy=None, tighten: str = "none", clip_step: float = 0.5) -> Dict[str, torch.Tensor]:
    """``render(rays_chunk, background_chunk) -> result dict`` (e.g. a ``functools.partial`` of
    ``render_rays``) applied to the valid rays in chunks of ``N_rand`` and, when a mask is given,
    scattered back into full-image ``rgb_*`` / ``depth_*`` exactly as trainer_moco_flow.py:249-266 does:
    every other key stays per rendered ray.  ``rays`` / ``background`` / ``rays_msk`` may live on the host
    (they are moved once, not per chunk).

    ``occupancy``: an ``occupancy.OccupancyGrid`` of the frame.  The rays rendered are then those of ``rays_msk`` (all rays
    when it is None) that also hit the grid, taken from ``occupancy.cull(rays, tighten, clip_step)``'s table, and the image is
    always composed: a rendered pixel exactly as without a grid; a pixel of ``rays_msk`` that the grid culled gets
    (background, depth 8), the reference's "rendered, opacity 0" case; a pixel outside ``rays_msk`` (background, depth 10).
    Every other key has one row per KEPT ray.  ``tighten`` "none" renders the kept rays bit for bit as without a grid;
    "near" / "both" move their near / far to the clipped interval (``OccupancyGrid.cull`` has the caveat on "both").
    None: the function does exactly what it did before the argument existed."""
    dev = torch.device("cuda", torch.cuda.current_device()) if not (torch.is_tensor(rays) and rays.is_cuda) else rays.device
    rays = torch.as_tensor(rays).to(dev)
    background = torch.as_tensor(background).to(dev)
    if occupancy is not None:
        return _render_image_culled(rays, background, render, N_rand, rays_msk, occupancy, tighten, clip_step)
    sel_rays, sel_bg, m = rays, background, None
    if rays_msk is not None:
        m = torch.as_tensor(rays_msk).to(dev).reshape(-1).bool()
        sel_rays, sel_bg = rays[m], background[m]
    chunks = []
    for i in range(0, sel_rays.shape[0], N_rand):
        chunks.append(render(sel_rays[i:i + N_rand], sel_bg[i:i + N_rand]))
    if not chunks:                                   # no valid ray at all: the reference's empty-chunk result
        chunks.append(render(sel_rays[:0], sel_bg[:0]))
    results = {k: torch.cat([c[k] for c in chunks], 0) for k in chunks[0]}
    if rays_msk is not None:
        typ = "fine" if "rgb_fine" in results else "coarse"
        img, dep = compose_image(m, results[f"opacity_{typ}"], results[f"rgb_{typ}"], results[f"depth_{typ}"], background)
        results[f"rgb_{typ}"] = img
        results[f"depth_{typ}"] = dep
    return results


def _render_image_culled(rays, background, render, N_rand, rays_msk, occupancy, tighten, clip_step):
    """render_image behind an occupancy grid: rays / background on the device already."""
    dev = rays.device
    B = rays.shape[0]
    if rays_msk is not None:
        m = torch.as_tensor(rays_msk).to(dev).reshape(-1).bool()
        sel_rays, sel_bg = rays[m], background[m]
    else:
        m = torch.ones(B, dtype=torch.bool, device=dev)
        sel_rays, sel_bg = rays, background
    culled, hit = occupancy.cull(sel_rays.float(), tighten, clip_step)
    keep = hit.bool()
    sel_rays, sel_bg = culled[keep], sel_bg[keep]
    kept = torch.zeros(B, dtype=torch.bool, device=dev)           # the pixels that are rendered
    kept[m] = keep
    chunks = []
    for i in range(0, sel_rays.shape[0], N_rand):
        chunks.append(render(sel_rays[i:i + N_rand], sel_bg[i:i + N_rand]))
    if not chunks:                                   # every ray culled: the empty-chunk result, as for an all-false mask
        chunks.append(render(sel_rays[:0], sel_bg[:0]))
    results = {k: torch.cat([c[k] for c in chunks], 0) for k in chunks[0]}
    typ = "fine" if "rgb_fine" in results else "coarse"
    if sel_rays.shape[0]:
        img, dep = compose_image(kept, results[f"opacity_{typ}"], results[f"rgb_{typ}"], results[f"depth_{typ}"], background)
    else:                                            # nothing rendered (mf_image_compose takes no empty ray arrays)
        img, dep = background.detach().float().clone(), torch.full((B,), 10.0, device=dev)
    dep.masked_fill_(m & ~kept, 8.0)                 # culled inside the mask: "rendered, opacity 0" (img is the background already)
    results[f"rgb_{typ}"] = img
    results[f"depth_{typ}"] = dep
    return results
