"""Occupancy grids: cull and clip test-time rays before the render pass (mf_occ_build, mf_ray_clip).

The reference renders every ray inside the hull of the projected AABB (MoCoFlowTrainer.render, trainer_moco_flow.py:226-268)
from the nearest to the farthest AABB corner (Camera.make_rays, utils/camera.py:134-148; rendering.py:239-249 spreads the
coarse samples over that whole interval).  A body fills a fraction of the hull and of the interval.  An ``OccupancyGrid`` is
one bit per cell of a lattice over the AABB, built from ONE ``query_sigma`` call at a frame's image index -- or, without any
network, from the frame's posed SMPL mesh (``from_mesh`` / ``from_smpl``: mf_voxel_mesh, mf_voxel_fill, mf_voxel_dilate,
mf_grid_edt for the exact Euclidean shell and the grid's squared-distance field); ``clip_rays``
marches rays through it, ``cull`` turns the result into a ray table, and ``image.render_image(..., occupancy=grid)`` renders
only the rays that hit.  A grid belongs to one frame index: it serves that frame's overfit view, its novel view and every
view of its orbit.  Opt-in: nothing changes for a caller that passes no grid."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib as L
from .points import query_sigma, query_sigma_lattice

__all__ = ["OccupancyGrid"]

_ACT = {"relu": L.MF_ACT_RELU, "softplus": L.MF_ACT_SOFTPLUS}
_TIGHTEN = ("none", "near", "both")
_SHELLS = ("box", "euclidean")
_EDT_ONE = 65536                                  # the integer weight of the longest cell edge (mf_grid_edt)


def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def _int3(v, what, least):
    """An int or a 3-tuple of ints >= ``least`` -> a 3-tuple."""
    t = (v,) * 3 if isinstance(v, (int, np.integer)) and not isinstance(v, bool) else tuple(v) if isinstance(v, (tuple, list)) else None
    if t is None or len(t) != 3 or any(isinstance(x, bool) or not isinstance(x, (int, np.integer)) or x < least for x in t):
        raise RuntimeError(f"OccupancyGrid: {what} must be an int or a 3-tuple of ints >= {least}, got {v!r}")
    return tuple(int(x) for x in t)


class OccupancyGrid:
    """``bits`` uint32 (Gx, Gy, ceil(Gz / 32)) on ``device``: cell (i, j, k) is bit k % 32 of ``bits[i, j, k // 32]``, padding
    bits zero; ``dims`` = (Gx, Gy, Gz) cells over the box ``lo`` .. ``hi`` (fp32 numpy (3,) each)."""

    def __init__(self, bits, dims, lo, hi, count=None):
        L.require_gpu(bits, "OccupancyGrid")
        self.bits = bits
        self.dims = tuple(int(g) for g in dims)
        self.lo = np.asarray(lo, dtype=np.float32).reshape(3).copy()
        self.hi = np.asarray(hi, dtype=np.float32).reshape(3).copy()
        self.device = bits.device
        self._count = count                       # device int64[1], written by the build
        if tuple(bits.shape) != (self.dims[0], self.dims[1], (self.dims[2] + 31) // 32) or bits.dtype != torch.int32:
            raise RuntimeError(f"OccupancyGrid: bits {tuple(bits.shape)} {bits.dtype} do not hold {self.dims} cells as int32 words")
        if not (self.lo < self.hi).all():
            raise RuntimeError(f"OccupancyGrid: empty or inverted box lo={self.lo.tolist()} hi={self.hi.tolist()}")
        # the cell edge in float64 from the fp32 box; what the kernel multiplies by is its fp32 reciprocal
        self.cell = (self.hi.astype(np.float64) - self.lo.astype(np.float64)) / np.asarray(self.dims, dtype=np.float64)
        self.inv_cell = (1.0 / self.cell).astype(np.float32)

    @classmethod
    def from_sigma(cls, volume, lo, hi, sigma_threshold, activate_type="softplus", dilate=1):
        """The grid of a raw-sigma lattice ``volume`` (Nx, Ny, Nz) on a 'cuda' device (z fastest, as ``query_sigma`` returns
        the lattice of ``from_field``) whose corner points are ``lo`` and ``hi``: (Nx-1, Ny-1, Nz-1) cells.  Cell (i, j, k) is
        occupied iff a lattice point of [i-r, i+1+r] x [j-r, j+1+r] x [k-r, k+1+r] (r = ``dilate`` in {0, 1, 2}, clipped to
        the lattice) has activate(sigma) > ``sigma_threshold``, strictly; a NaN counts as occupied.  ``activate_type``:
        "relu" | "softplus", as render_rays' nerf_activate_type.  No synchronisation."""
        L.require_gpu(volume, "OccupancyGrid.from_sigma")
        if volume.dim() != 3:
            raise RuntimeError(f"OccupancyGrid.from_sigma: volume must be (Nx, Ny, Nz), got shape {tuple(volume.shape)}")
        if activate_type not in _ACT:
            raise RuntimeError(f"OccupancyGrid.from_sigma: activate_type {activate_type!r} (relu | softplus)")
        nx, ny, nz = (int(n) for n in volume.shape)
        dev = volume.device
        scratch = L.scratch(dev, "mf_occ_build_scratch_bytes", nx, ny, nz)    # a bad shape is rejected here, before anything is copied
        vol = volume.detach().float().contiguous()
        bits = torch.empty((nx - 1, ny - 1, (nz - 1 + 31) // 32), dtype=torch.int32, device=dev)
        count = torch.empty(1, dtype=torch.int64, device=dev)
        L.launch(dev, "mf_occ_build", vol.data_ptr(), nx, ny, nz, _ACT[activate_type], float(np.float32(sigma_threshold)),
                 int(dilate), bits.data_ptr(), count.data_ptr(), scratch.data_ptr())
        return cls(bits, (nx - 1, ny - 1, nz - 1), lo, hi, count)

    @staticmethod
    def lattice_axes(N_grid, aabb):
        """The lattice's coordinates per axis, three fp32 numpy arrays, and its (Nx, Ny, Nz)."""
        n = (int(N_grid),) * 3 if np.isscalar(N_grid) else tuple(int(v) for v in N_grid)
        box = np.asarray(aabb, dtype=np.float64)
        if box.shape != (2, 3) or len(n) != 3:
            raise RuntimeError(f"OccupancyGrid: aabb must be (2, 3) and N_grid an int or a 3-tuple, got {box.shape} and {N_grid!r}")
        return [np.linspace(box[0, a], box[1, a], n[a]).astype(np.float32) for a in range(3)], n

    @staticmethod
    def lattice(N_grid, aabb, device):
        """``from_field``'s query points (N, 3) and their (Nx, Ny, Nz): np.linspace(lo_a, hi_a, N_a) in float64 cast to fp32,
        x slowest, z fastest -- NOT ``mesh.lattice``'s 'xy' order."""
        axes, n = OccupancyGrid.lattice_axes(N_grid, aabb)
        ax = [torch.from_numpy(x).to(device) for x in axes]
        pts = torch.stack([ax[0].view(-1, 1, 1).expand(*n), ax[1].view(1, -1, 1).expand(*n), ax[2].view(1, 1, -1).expand(*n)], -1)
        return pts.reshape(-1, 3), n

    @classmethod
    def from_field(cls, nerf, nerf_embedding_xyz, aabb, N_grid=128, sigma_threshold=1.0, activate_type="softplus", dilate=1,
                   bw_nof=None, nof_embeddings=None, ind=None, precision=None, within=None):
        """The grid of the networks over ``aabb`` ((2, 3): min and max corner, as ``rescale_AABB`` returns it): one
        ``query_sigma`` call on the lattice -- with ``bw_nof`` / ``nof_embeddings`` / ``ind`` through the backward flow at
        image index ``ind``, in ``precision`` -- then ``from_sigma``; bit-identical to those two steps by hand.

        ``N_grid``: lattice points per axis, an int or (Nx, Ny, Nz).  The lattice is np.linspace(lo_a, hi_a, N_a) in float64
        cast to fp32, laid out x slowest, z fastest.  This is NOT ``mesh.lattice``'s 'xy' order (there point (a, b, c) is
        (x[b], y[a], z[c])).

        ``sigma_threshold`` = 1.0 on the ACTIVATED density is a starting value: nobody has validated it on a trained
        checkpoint.  Too high a threshold hides thin or faint parts of the body; check a few frames against a render
        without the grid before relying on it.

        ``within`` (None leaves the path as it was): a coarser ``OccupancyGrid`` over the same box.  The lattice is then
        queried only in the bricks of 8 x 8 x 8 points that ``within`` marks, one lattice point of margin around each
        (``query_sigma_lattice`` with fill = -inf, which no activation lifts over a threshold >= 0), and ``from_sigma`` runs
        on that volume -- bit-identical to those two steps by hand.  This ADDS ONE HOST SYNCHRONISATION, the read of the
        active-brick count, which the dense path does not have.  What ``within`` does not mark stays empty here: a part it
        missed is missed again, whatever ``sigma_threshold`` is."""
        dev = next(nerf.parameters()).device
        L.require_gpu(next(nerf.parameters()), "OccupancyGrid.from_field")
        if within is not None:
            axes, _ = cls.lattice_axes(N_grid, aabb)
            box = np.asarray(aabb, dtype=np.float64)
            sigma = query_sigma_lattice(axes, nerf, nerf_embedding_xyz, within, fill=float("-inf"), bw_nof=bw_nof,
                                        nof_embeddings=nof_embeddings, ind=ind, precision=precision)
            return cls.from_sigma(sigma, box[0], box[1], sigma_threshold, activate_type, dilate)
        xyz, n = cls.lattice(N_grid, aabb, dev)
        box = np.asarray(aabb, dtype=np.float64)
        with torch.no_grad():
            sigma = query_sigma(xyz, nerf, nerf_embedding_xyz, bw_nof, nof_embeddings, ind, precision=precision)
            del xyz
            return cls.from_sigma(sigma.view(*n), box[0], box[1], sigma_threshold, activate_type, dilate)

    def step_length(self, step=0.5):
        """dt of a march: fp32(step * the shortest cell edge), in world units."""
        return float(np.float32(float(step) * float(self.cell.min())))

    def clip_rays(self, rays, step=0.5):
        """rays (R, >= 8) [o, d, near, far, ...] on the grid's device -> (t_first (R,), t_last (R,), hit (R,) uint8): the ray is
        clipped to the box and to [near, far], then sampled every dt = fp32(step * min cell edge); with kf / kl the first / last
        sample in an occupied cell, t_first = max(near, t_kf - dt), t_last = min(far, t_kl + dt), hit = 1.  No sample in an
        occupied cell: hit = 0, (near, far) unchanged.  A ray with a NaN or inf in its first 8 columns is never hidden: hit = 1,
        (near, far) unchanged.  Any row stride works (a view is not copied).

        Guarantee: with ``dilate >= 1`` at the build, ``step <= 0.5`` and unit directions (``camera.make_rays`` gives them;
        any length <= 1 will do), a ray that passes, inside [near, far], through a cell that was occupied before dilation is
        never missed, and [t_first, t_last] contains every such crossing: a point of the crossing at parameter t has the sample
        t_k <= t < t_k + dt in front of it, less than |d| dt <= half a cell edge away, hence at most one cell away along every
        axis, and dilation has set that cell.  Outside that regime ``step`` is accepted and the guarantee is not given.  (The
        march is bounded by the steps a unit direction needs through the box's diagonal; a shorter direction that runs out of
        them inside the box keeps hit = 1 and its ``far``.)"""
        L.require_gpu(rays, "OccupancyGrid.clip_rays")
        if rays.dim() != 2 or rays.shape[1] < 8 or rays.dtype != torch.float32:
            raise RuntimeError(f"OccupancyGrid.clip_rays: rays must be fp32 (R, >= 8), got {tuple(rays.shape)} {rays.dtype}")
        if rays.device != self.device:
            raise RuntimeError(f"OccupancyGrid.clip_rays: rays on {rays.device}, the grid on {self.device}")
        r = rays.detach()
        R = r.shape[0]
        if R <= 1 or r.stride(1) != 1 or r.stride(0) < 8:
            r = r.contiguous()
        stride = r.stride(0) if R > 1 else int(r.shape[1])
        dev = self.device
        t_first = torch.empty(R, dtype=torch.float32, device=dev)
        t_last = torch.empty(R, dtype=torch.float32, device=dev)
        hit = torch.empty(R, dtype=torch.uint8, device=dev)
        L.launch(dev, "mf_ray_clip", L.ptr0(r), stride, R, self.bits.data_ptr(), *self.dims, _f3(self.lo), _f3(self.hi),
                 _f3(self.inv_cell), self.step_length(step), L.ptr0(t_first), L.ptr0(t_last), L.ptr0(hit))
        return t_first, t_last, hit

    def cull(self, rays, tighten="none", step=0.5):
        """(rays_out, hit): ``rays_out`` a copy of ``rays`` with column 6 replaced by t_first (``tighten`` "near" or "both")
        and column 7 by t_last ("both"), ``hit`` (R,) uint8 as ``clip_rays`` returns it.  Rows that miss keep their near / far.

        Caveat on "both": the reference's last sample of a ray carries a delta of 1e10 (models/rendering.py:159), so whatever
        density sits at ``far`` is composited as opaque.  With the far AABB corner as ``far`` that sample lies in empty space;
        a tightened ``far`` puts it just behind the body instead -- within one step plus one dilated cell of the last occupied
        sample -- where a residual density shows up at full opacity.  "near" alone only moves samples out of the empty space
        in front of the body.  Either changes where the samples fall, so the picture differs from the unclipped render in the
        last places or more; "none" renders the kept rays exactly as before."""
        if tighten not in _TIGHTEN:
            raise RuntimeError(f"OccupancyGrid.cull: tighten {tighten!r} (none | near | both)")
        t_first, t_last, hit = self.clip_rays(rays, step)
        out = rays.detach().clone()
        if tighten in ("near", "both"):
            out[:, 6] = t_first
        if tighten == "both":
            out[:, 7] = t_last
        return out, hit

    def to_dense(self):
        """bool (Gx, Gy, Gz) on the grid's device."""
        shifts = torch.arange(32, device=self.device, dtype=torch.int32)
        b = (self.bits.unsqueeze(-1) >> shifts) & 1
        return b.reshape(self.dims[0], self.dims[1], -1)[:, :, :self.dims[2]].bool()

    def occupied_fraction(self):
        """Occupied cells / cells, a python float: the one call that synchronises (it reads the build's count)."""
        if self._count is None:
            self._count = self.to_dense().sum().reshape(1)
        return int(self._count.item()) / float(self.dims[0] * self.dims[1] * self.dims[2])

    # ---- grids from a mesh (csrc/mf_voxelize.hip) -----------------------------------------------------------------------------

    @classmethod
    def from_mesh(cls, verts, tris, aabb, dims=128, dilate=1, thickness=0.0, solid=True, return_dropped=False, shell="box"):
        """The grid of a triangle mesh -- ``verts`` (V, 3) fp32 and ``tris`` (T, 3) int64 on a 'cuda' device -- over ``aabb``
        ((2, 3): min and max corner, as ``from_field`` takes it) in ``dims`` cells (an int or (Gx, Gy, Gz), each 1 .. 1024).
        Three steps, in this order, every one decided in integers and so bit-identical from run to run:

        1. surface (mf_voxel_mesh): vertices go to grid coordinates by ``clip_rays``' cell rule, u = (p - lo) * inv_cell in fp32,
           and are snapped to 1/64 cell; a cell is set iff the closed snapped triangle meets the closed cell.  A triangle in a
           cell face sets the cells on both sides.  Triangles with an index outside [0, V), a NaN or inf vertex, or no area after
           snapping are skipped (``return_dropped=True`` returns ``(grid, dropped)`` with their number, and synchronises to read
           it; otherwise nothing synchronises).  Snapped coordinates saturate 1024 cells below the box and 2048 cells above its
           origin: a triangle that reaches further out than that is distorted.
        2. fill, if ``solid`` (mf_voxel_fill): + every empty cell that is not 6-connected through empty cells to the outside of the
           grid.  A mesh that is open, or cut by the box, leaks and fills nothing; a torus's hole stays empty; a closed shell
           inside a closed shell is filled through.
        3. box dilation (mf_voxel_dilate) by r_a = dilate_a + ceil(thickness / cell_a) cells along axis a, computed in float64 on
           the host from the grid's ``cell``: ``dilate`` in cells (an int or a 3-tuple, >= 0), ``thickness`` >= 0 in world units.
           The box of radii r is a deliberate SUPERSET of the Euclidean shell of ``thickness``: it keeps the contract in integers.

        The build's count lands where ``from_sigma`` puts it (``occupied_fraction`` reads it).

        (a) With the reference's ``thickness`` (0.2, datasets/moco_flow_dataset.py:87-142: a point is "inside" iff it lies
            within ``thickness`` of an SMPL vertex) and ``dilate >= 1``, every point of the box within ``thickness`` of a vertex,
            inside the box, of a non-skipped triangle falls, by ``clip_rays``' cell rule, in a set cell: the vertex's cell is set
            (snapping moves a vertex across a cell boundary only onto it, and a point on a boundary sets both sides), the point
            is at most ceil(thickness / cell_a) cells from it along axis a, and ``dilate`` absorbs the fp32 rounding of u.
        (b) The true surface lies within 1/128 cell of the snapped one along every axis, hence ``dilate >= 1`` covers it and
            meets the ``dilate >= 1`` premise of ``clip_rays``' guarantee.
        (c) What reaches beyond the SMPL shell by more than ``thickness`` is CULLED -- loose clothing and hair are the likely
            cases.  Check a few frames against an unculled render; no thickness has been validated on a trained checkpoint.

        ``shell="euclidean"`` (the default "box" is step 3 above, unchanged; any other string raises) replaces step 3 by
        ``dilated_euclidean(thickness)`` (mf_grid_edt: the cells within ``thickness`` of a set cell's index, in the integer
        metric of ``euclid_metric``) followed by the box dilation ``dilated(dilate_a + 1)``.  Guarantee (a) holds as it does
        for the box: with ``dilate >= 1``, every point of the box within ``thickness`` of a point of a cell set before the
        dilation falls in a set cell.  Two cells k apart leave a gap of max(|k_a| - 1, 0) cell_a along axis a between their
        points, so the cells that hold a point within t of a set cell are the ball of that gap metric, which is E(t) + box(1):
        the ellipsoid of index offsets with sum (k_a cell_a)^2 <= t^2 -- ``euclid_metric`` rounds it outwards -- grown by one
        cell per axis; ``dilate`` then absorbs the fp32 rounding of u and the 1/64 snapping as in (a).  (b) and ``clip_rays``'
        premise hold as before, and (c) applies unchanged.  The Euclidean shell is NOT a subset of the box shell in general:
        along axis a alone it reaches r_a + dilate_a + 1 cells against the box's dilate_a + ceil(thickness / cell_a), which is
        one cell more when thickness / cell_a is a whole number; away from the axes it is thinner (a box shell is sqrt(3)
        times too thick along its diagonal)."""
        L.require_gpu(verts, "OccupancyGrid.from_mesh")
        L.require_gpu(tris, "OccupancyGrid.from_mesh")
        if verts.dim() != 2 or verts.shape[1] != 3 or verts.dtype != torch.float32:
            raise RuntimeError(f"OccupancyGrid.from_mesh: verts must be fp32 (V, 3), got {tuple(verts.shape)} {verts.dtype}")
        if tris.dim() != 2 or tris.shape[1] != 3 or tris.dtype != torch.int64:
            raise RuntimeError(f"OccupancyGrid.from_mesh: tris must be int64 (T, 3), got {tuple(tris.shape)} {tris.dtype}")
        if tris.device != verts.device:
            raise RuntimeError(f"OccupancyGrid.from_mesh: verts on {verts.device}, tris on {tris.device}")
        box = np.asarray(aabb, dtype=np.float64)
        if box.shape != (2, 3):
            raise RuntimeError(f"OccupancyGrid.from_mesh: aabb must be (2, 3), got {box.shape}")
        dims = _int3(dims, "dims", 1)
        dilate = _int3(dilate, "dilate", 0)
        thickness = float(thickness)
        if not (0.0 <= thickness < math.inf):
            raise RuntimeError(f"OccupancyGrid.from_mesh: thickness={thickness} must be finite and >= 0")
        if shell not in _SHELLS:
            raise RuntimeError(f"OccupancyGrid.from_mesh: shell {shell!r} (box | euclidean)")
        dev = verts.device
        v, t = verts.detach().contiguous(), tris.detach().contiguous()
        bits = torch.empty((dims[0], dims[1], (dims[2] + 31) // 32), dtype=torch.int32, device=dev)
        surface = cls(bits, dims, box[0], box[1])                         # its lo, hi and inv_cell are what the kernel is given
        dropped = torch.empty(1, dtype=torch.int64, device=dev) if return_dropped else None
        V, T = int(v.shape[0]), int(t.shape[0])
        L.launch(dev, "mf_voxel_mesh", L.ptr0(v), V, L.ptr0(t), T, *dims, _f3(surface.lo), _f3(surface.hi), _f3(surface.inv_cell),
                 bits.data_ptr(), L.ptr(dropped))
        grid = surface.filled() if solid else surface
        if shell == "euclidean":
            grid = grid.dilated_euclidean(thickness).dilated(tuple(d + 1 for d in dilate))
        else:
            radii = tuple(dilate[a] + int(math.ceil(thickness / float(surface.cell[a]))) for a in range(3))
            grid = grid.dilated(radii)
        return (grid, int(dropped.item())) if return_dropped else grid

    @classmethod
    def from_smpl(cls, smpl, pose, betas, aabb, **kw):
        """``from_mesh`` on the posed body: ``smpl(pose, betas)[0]`` and ``smpl.faces`` (``smpl.SMPL``, skinned on the device),
        bit-identical to those two steps by hand.  ``kw``: ``from_mesh``'s keywords."""
        faces = getattr(smpl, "faces", None)
        if faces is None:
            raise RuntimeError("OccupancyGrid.from_smpl: the SMPL model carries no faces (its 'f' array)")
        with torch.no_grad():
            verts = smpl(pose, betas)[0]
        return cls.from_mesh(verts, faces, aabb, **kw)

    def filled(self):
        """A new grid over the same box: this one plus every empty cell that is not 6-connected through empty cells to the outside
        of the grid (mf_voxel_fill).  No synchronisation; the count is left to ``occupied_fraction``."""
        dev = self.device
        scratch = L.scratch(dev, "mf_voxel_fill_scratch_bytes", *self.dims)
        src = self.bits.contiguous()
        out = torch.empty_like(src)
        L.launch(dev, "mf_voxel_fill", src.data_ptr(), *self.dims, out.data_ptr(), scratch.data_ptr())
        return OccupancyGrid(out, self.dims, self.lo, self.hi)

    def dilated(self, radii):
        """A new grid over the same box: cell (i, j, k) is set iff a cell of [i - rx, i + rx] x [j - ry, j + ry] x [k - rz, k + rz],
        clipped to the grid, is set here (mf_voxel_dilate).  ``radii``: an int or (rx, ry, rz), >= 0, of any size.  Works on any
        grid, one from a field included.  No synchronisation; the new grid carries its count."""
        radii = _int3(radii, "radii", 0)
        if any(r >= 1 << 31 for r in radii):
            raise RuntimeError(f"OccupancyGrid.dilated: radii {radii} do not fit 32 bits")
        dev = self.device
        scratch = L.scratch(dev, "mf_voxel_dilate_scratch_bytes", *self.dims)
        src = self.bits.contiguous()
        out = torch.empty_like(src)
        count = torch.empty(1, dtype=torch.int64, device=dev)
        L.launch(dev, "mf_voxel_dilate", src.data_ptr(), *self.dims, *radii, out.data_ptr(), count.data_ptr(), scratch.data_ptr())
        return OccupancyGrid(out, self.dims, self.lo, self.hi, count)

    # ---- the Euclidean shell and the distance field (csrc/mf_distance.hip) ------------------------------------------------------

    @staticmethod
    def euclid_metric(cell, radius):
        """The integer metric of mf_grid_edt for float64 cell edges ``cell`` (3,) and a world ``radius`` >= 0 -> (w, R, r), all
        Python ints from float64 arithmetic on the host: with cmax = cell.max(), w_a = floor(65536 (cell_a / cmax)^2) in
        [1, 65536] (below 1 raises), R = ceil(65536 (radius / cmax)^2) (R >= 2^30, i.e. radius >= 128 cmax, raises) and
        r_a = isqrt(R // w_a), the reach in cells along axis a.  The floor and the ceil keep {sum w_a k_a^2 <= R} a superset
        of the real-valued ellipsoid {sum (k_a cell_a)^2 <= radius^2}; cubic cells give w = 65536 on every axis."""
        c = np.asarray(cell, dtype=np.float64).reshape(-1)
        radius = float(radius)
        if c.shape != (3,) or not (np.isfinite(c).all() and (c > 0).all()):
            raise RuntimeError(f"OccupancyGrid.euclid_metric: cell must be three finite edges > 0, got {cell!r}")
        if not (0.0 <= radius < math.inf):
            raise RuntimeError(f"OccupancyGrid.euclid_metric: radius={radius} must be finite and >= 0")
        cmax = float(c.max())
        ratios = [float(x) / cmax for x in c]
        w = tuple(int(math.floor(_EDT_ONE * (q * q))) for q in ratios)
        if min(w) < 1:
            raise RuntimeError(f"OccupancyGrid.euclid_metric: cell edges {c.tolist()} differ by more than a factor of 256")
        q = radius / cmax
        big = _EDT_ONE * (q * q)
        if not big < float(1 << 30) or int(math.ceil(big)) >= 1 << 30:
            raise RuntimeError(f"OccupancyGrid.euclid_metric: radius={radius} is not below 128 times the longest cell edge {cmax}")
        R = int(math.ceil(big))
        return w, R, tuple(math.isqrt(R // x) for x in w)

    def _edt(self, radius, want_d2, want_bits):
        w, R, _ = self.euclid_metric(self.cell, radius)
        dev = self.device
        scratch = L.scratch(dev, "mf_grid_edt_scratch_bytes", *self.dims)
        src = self.bits.contiguous()
        d2 = torch.empty(self.dims, dtype=torch.int32, device=dev) if want_d2 else None
        out = torch.empty_like(src) if want_bits else None
        count = torch.empty(1, dtype=torch.int64, device=dev) if want_bits else None
        L.launch(dev, "mf_grid_edt", src.data_ptr(), *self.dims, (C.c_int32 * 3)(*w), R, L.ptr(d2), L.ptr(out), L.ptr(count),
                 scratch.data_ptr())
        return d2, out, count, w, R

    def squared_distance(self, radius):
        """(d2, w, R): ``d2`` int32 (Gx, Gy, Gz) on the grid's device, the squared distance of every cell's index to the nearest
        set cell's in the metric ``euclid_metric(self.cell, radius)`` = (w, R, r), capped: d2 = min(R + 1, min over set cells
        of sum w_a k_a^2); an empty grid gives R + 1 everywhere.  The world distance between the two cells' centres is
        cmax * sqrt(d2 / 65536) with cmax = ``cell.max()`` -- exactly Euclidean for cubic cells, rounded down by the floor of
        w otherwise -- wherever d2 <= R; ``d2 <= R2`` for any R2 <= R re-thresholds at a smaller radius without voxelising
        again.  Each side at most 1024 cells.  No synchronisation."""
        d2, _, _, w, R = self._edt(radius, True, False)
        return d2, w, R

    def dilated_euclidean(self, radius):
        """A new grid over the same box: the cells with ``squared_distance(radius)`` <= R, i.e. within ``radius`` (world units)
        of a set cell, index to index, in the outward-rounded integer metric of ``euclid_metric`` (mf_grid_edt).  ``radius`` 0
        returns the same cells.  Each side at most 1024 cells.  No synchronisation; the new grid carries its count."""
        _, out, count, _, _ = self._edt(radius, False, True)
        return OccupancyGrid(out, self.dims, self.lo, self.hi, count)

    def _same_grid(self, other, what):
        if not isinstance(other, OccupancyGrid):
            raise RuntimeError(f"OccupancyGrid.{what}: the other operand is {type(other).__name__}, not an OccupancyGrid")
        if other.dims != self.dims or other.device != self.device or not (np.array_equal(other.lo, self.lo) and np.array_equal(other.hi, self.hi)):
            raise RuntimeError(f"OccupancyGrid.{what}: grids differ: {self.dims} over {self.lo.tolist()} .. {self.hi.tolist()} on "
                               f"{self.device} and {other.dims} over {other.lo.tolist()} .. {other.hi.tolist()} on {other.device}")

    def __and__(self, other):
        """The cells set in both grids (same ``dims``, box and device, else RuntimeError): the SMPL shell cut with a field's grid,
        say.  Word-wise on ``bits``; the count is left to ``occupied_fraction``."""
        self._same_grid(other, "__and__")
        return OccupancyGrid(self.bits & other.bits, self.dims, self.lo, self.hi)

    def __or__(self, other):
        """The cells set in either grid; as ``&``."""
        self._same_grid(other, "__or__")
        return OccupancyGrid(self.bits | other.bits, self.dims, self.lo, self.hi)
