"""moco_flow_amd -- MI355X (gfx950) implementation of MoCo-Flow's volume-rendering hot path.

Drop-in surface (same names / signatures as the reference's ``models`` package):
    Embedding, NeRF, NoF, get_model, get_loss, render_rays, sample_pdf
and ``moco_flow_amd.metrics`` for the reference's ``models.metrics`` (mse, psnr, ssim; plus image_metrics),
``moco_flow_amd.vis`` for ``utils.vis_utils.visualize_depth`` (plus decode_results, frame_sheet, write_png),
``moco_flow_amd.batch`` for the ray batch of a training step (FrameRays: selection, rays and pixels in one launch),
``moco_flow_amd.supervision`` for its SMPL point supervision (correspondence, point_losses: no compaction, no host read),
``moco_flow_amd.occupancy`` for a frame's occupancy grid (OccupancyGrid: culls and clips test-time rays in front of render_image),
``moco_flow_amd.raster`` for the pictures the reference draws with pyrender (render_mesh, smpl_views: the stage-1 SMPL views),
``moco_flow_amd.frames`` for frame ingest (resize as PIL does it, composite / to_rows, background_plate, clean_mask / mask_regions: bytes in, tensors out).
Every forward value comes from hand-written HIP kernels reached through the C ABI in include/mocoflow_hip.h
(libmocoflow_hip.so); CPU tensors and a missing library raise.  The backward is HIP as well -- of render_rays passes
(which record gradients in fp32 whatever set_precision says) and of module-level NeRF / NoF / Embedding calls; shapes it
is not built for raise NotImplementedError under grad.  There is no eager fallback (autograd.py).
"""
from .embedding import Embedding
from .factory import get_loss, get_model
from .losses import MSELoss
from .nerf import NeRF
from .nof import NoF
from .points import query_radiance, query_sigma, query_sigma_lattice
from .mesh import (export_obj, export_ply, extract_colored_mesh, extract_mesh, filter_components, marching_cubes, mesh_components,
                   simplify_mesh, smooth_mesh, vertex_normals, vertex_rings, MeshIndex, closest_point, sample_surface,
                   surface_distance, surface_stats, cast_rays, visible_from)
from . import metrics
from .metrics import image_metrics
from . import vis
from .vis import decode_results, frame_sheet, visualize_depth, write_png
from . import batch
from .batch import FrameRays
from . import supervision
from .supervision import Correspondence, correspondence, point_correspond, point_losses
from . import occupancy
from .occupancy import OccupancyGrid
from . import raster
from .raster import interpolate, project_vertices, rasterize, render_mesh, smpl_views
from . import frames
from .frames import Regions, background_plate, clean_mask, composite, mask_regions, resize, to_rows
from .autograd import set_dx_precision, set_wgrad_precision
from .rendering import render_rays, resample_merge, sample_pdf, set_precision, set_train_forward_precision

__all__ = ["Embedding", "NeRF", "NoF", "get_model", "get_loss", "render_rays", "sample_pdf",
           "resample_merge", "set_precision", "set_wgrad_precision", "set_dx_precision", "set_train_forward_precision", "query_sigma", "MSELoss",
           "marching_cubes", "mesh_components", "filter_components", "simplify_mesh", "vertex_rings", "smooth_mesh", "extract_mesh", "export_obj", "query_radiance", "extract_colored_mesh", "vertex_normals", "export_ply", "metrics", "image_metrics",
           "vis", "visualize_depth", "decode_results", "frame_sheet", "write_png", "batch", "FrameRays",
           "supervision", "Correspondence", "correspondence", "point_correspond", "point_losses",
           "occupancy", "OccupancyGrid", "query_sigma_lattice",
           "raster", "project_vertices", "rasterize", "interpolate", "render_mesh", "smpl_views",
           "frames", "resize", "composite", "to_rows", "background_plate", "clean_mask", "mask_regions", "Regions",
           "MeshIndex", "closest_point", "sample_surface", "surface_distance", "surface_stats", "cast_rays", "visible_from"]
