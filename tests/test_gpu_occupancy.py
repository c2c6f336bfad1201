"""Occupancy grids on the device (-m gpu): mf_occ_build and mf_ray_clip against tests/occupancy_oracle.py, word for word and
value for value -- the oracle restates both kernels in fp32, so there is no tolerance -- then OccupancyGrid.from_field
against its two steps done by hand, and image.render_image behind a grid against the same call without one.

Floats are compared by value with NaN equal to NaN (numpy's array_equal(equal_nan=True)): the kernel and numpy may pick a
different sign for a zero out of max(-0, +0), nothing else can differ.  The softplus lattices are drawn so that no point is
within 16 ulp of the threshold except in the region sigma > 20 where softplus is the identity (occupancy_oracle.ambiguous):
the device's log1pf(expf(s)) and numpy's float64 value may differ in the last places, and only there could that decide the
comparison."""
import functools

import numpy as np
import pytest
import torch

import occupancy_oracle as O
from helpers import build_case
from streams_util import HOLD_MS, first_done, hold, independent_streams, poison

pytestmark = pytest.mark.gpu

LATTICE = (34, 6, 65)                       # cells (33, 5, 64): row words are [32 cells, 32 cells] exactly ...
LATTICE_PART = (34, 6, 60)                  # ... and here (33, 5, 59): a partial last word of 27 cells
LO, HI = (-1.0, -0.3, -1.2), (1.0, 0.3, 1.2)


@pytest.fixture(scope="module")
def M():
    import moco_flow_amd
    assert torch.cuda.is_available()
    moco_flow_amd._lib.lib()
    return moco_flow_amd


def _same(got, want, what):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    assert got.shape == np.shape(want) and np.array_equal(got, want, equal_nan=got.dtype.kind == "f"), what


def _words(grid):
    return grid.bits.cpu().numpy().view(np.uint32)


def _lattice_values(n, act, tau, seed):
    """Raw sigma around the threshold: a sparse set of active points, values equal to tau exactly (relu; softplus: tau > 20, where
    the activation is the identity), +-inf and NaN, one active point at every corner of the lattice, and lone active points that
    set exactly cell 31 / cell 32 of a row at dilate = 0 (z-points 31 / 33 are shared with cells 30 / 33)."""
    rng = np.random.default_rng(seed)
    exact = act == "relu" or tau > 20                                  # the activation is the identity around tau
    edge = tau if exact else float(np.log(np.expm1(tau)))             # the raw sigma whose activation is tau
    spread = 1.0 if tau < 20 else 4.0
    s = (edge - 0.2 * spread - np.abs(rng.normal(0.0, spread, n))).astype(np.float32)         # everything inactive ...
    pick = rng.random(n) < max(0.005, 1.0 / s.size)
    s[pick] = (edge + 0.05 * spread + np.abs(rng.normal(0.0, spread, n)))[pick].astype(np.float32)   # ... but a few
    flat = s.reshape(-1)
    k = min(5, max(1, flat.size // 30))
    special = rng.permutation(flat.size)[:6 * k]
    flat[special[0:2 * k]] = np.float32(tau) if exact else np.float32(edge - 0.01)            # equal to tau: not active
    flat[special[2 * k:3 * k]] = np.nextafter(np.float32(tau), np.float32(np.inf)) if exact else np.float32(edge + 0.01)
    flat[special[3 * k:4 * k]] = np.inf
    flat[special[4 * k:5 * k]] = -np.inf
    flat[special[5 * k:6 * k]] = np.nan
    if n[2] > 34:
        i = n[0] // 2
        s[i:i + 2, 1:3, 28:38] = edge - 3.0
        s[i, 2, 32] = edge + 3.0                                                              # sets cells 31 and 32 of row (i, 1)
        s[i + 4:i + 6, 1:3, 27:37] = edge - 3.0
        s[i + 4, 2, 31] = edge + 3.0                                                          # cells 30 and 31 of row (i + 4, 1)
        for c in np.ndindex(2, 2, 2):
            s[tuple(-ci for ci in c)] = edge + 3.0                                            # index 0 or -1 on every axis
    assert np.isnan(s).any() and np.isinf(s).any()
    assert not O.ambiguous(s, act, tau).any()
    return s


@pytest.mark.parametrize("n", [LATTICE, LATTICE_PART, (3, 3, 3)])
@pytest.mark.parametrize("act,tau", [("relu", 0.75), ("softplus", 1.0), ("softplus", 24.0)])
def test_build_equals_the_oracle(M, n, act, tau):
    """The words, their padding bits and the count, for dilate = 0, 1, 2."""
    s = _lattice_values(n, act, tau, seed=sum(n) + int(tau))
    vol = torch.from_numpy(s).cuda()
    for dilate in (0, 1, 2):
        grid = M.OccupancyGrid.from_sigma(vol, LO, HI, tau, act, dilate)
        want, count = O.build(s, act, tau, dilate)
        got = _words(grid)
        assert grid.dims == (n[0] - 1, n[1] - 1, n[2] - 1) and got.shape == want.shape
        assert np.array_equal(got, want), (n, act, tau, dilate, int((got != want).sum()))
        rest = grid.dims[2] % 32
        if rest:
            assert (got[:, :, -1] >> np.uint32(rest) == 0).all()                              # the padding bits are zero
        dense = O.unpack(got, grid.dims[2])
        pop = int(dense.sum())
        assert pop == count and int(grid._count.item()) == pop
        assert grid.occupied_fraction() == pop / dense.size
        _same(grid.to_dense(), dense, "to_dense")
        if dilate == 0 and n[2] > 34:
            assert 0 < pop < dense.size
            assert dense[0, 0, 0] and dense[-1, -1, -1] and dense[0, -1, 0] and dense[-1, 0, -1]
            i = n[0] // 2
            assert dense[i, 1, 31] and dense[i, 1, 32] and not dense[i, 1, 30] and not dense[i, 1, 33]
            assert dense[i + 4, 1, 30] and dense[i + 4, 1, 31] and not dense[i + 4, 1, 32]
    again = M.OccupancyGrid.from_sigma(vol, LO, HI, tau, act, 2)
    assert torch.equal(again.bits, grid.bits) and torch.equal(again._count, grid._count)      # two runs: bit-identical


def test_build_of_a_non_contiguous_volume(M):
    s = _lattice_values((12, 7, 40), "relu", 0.75, seed=1)
    vol = torch.from_numpy(np.ascontiguousarray(s.transpose(2, 0, 1))).cuda().permute(1, 2, 0)     # same values, other strides
    assert not vol.is_contiguous()
    grid = M.OccupancyGrid.from_sigma(vol, LO, HI, 0.75, "relu", 1)
    assert np.array_equal(_words(grid), O.build(s, "relu", 0.75, 1)[0])


# ------------------------------------------------------------------------------------------------ the march
BALL_C, BALL_R = (0.2, 0.05, -0.3), 0.22


@pytest.fixture(scope="module")
def ball(M):
    """The (33, 5, 64) grid with a ball set: (grid, dense bool array, raw sigma)."""
    s = O.ball_lattice(LATTICE, LO, HI, BALL_C, BALL_R)
    grid = M.OccupancyGrid.from_sigma(torch.from_numpy(s).cuda(), LO, HI, 1.0, "softplus", 1)
    dense = O.build_dense(s, "softplus", 1.0, 1)
    assert np.array_equal(_words(grid), O.pack(dense)) and 0 < dense.sum() < dense.size // 8
    return grid, dense, s


def _clip_oracle(grid, dense, rays, step=0.5):
    lo, hi, inv, dt = O.grid_constants(grid.dims, grid.lo, grid.hi, step)
    assert np.array_equal(inv, grid.inv_cell) and float(dt) == grid.step_length(step)
    return O.clip(rays.detach().cpu().numpy(), dense, lo, hi, inv, dt)


def _check_clip(grid, dense, rays, what, step=0.5):
    want = _clip_oracle(grid, dense, rays, step)
    got = grid.clip_rays(rays, step)
    assert got[2].dtype == torch.uint8 and got[0].dtype == torch.float32
    _same(got[2], want[2], f"{what}: hit")
    _same(got[0], want[0], f"{what}: t_first")
    _same(got[1], want[1], f"{what}: t_last")
    return want


def _aimed_rays(R, seed):
    """Unit rays from outside and inside the box at points around the ball, with near / far in front of, inside and behind it."""
    rng = np.random.default_rng(seed)
    lo, hi = np.array(LO), np.array(HI)
    target = np.where(rng.random((R, 1)) < 0.6, np.array(BALL_C) + rng.normal(0.0, 0.25, (R, 3)), rng.uniform(lo, hi, (R, 3)))
    o = rng.normal(0.0, 1.0, (R, 3))
    o = o / np.linalg.norm(o, axis=1, keepdims=True) * rng.uniform(0.5, 5.0, (R, 1))
    o[3::7] = rng.uniform(lo, hi, (len(o[3::7]), 3))                                          # origins inside the box
    d = target - o
    dist = np.linalg.norm(d, axis=1)
    d32 = (d / dist[:, None]).astype(np.float32)
    d32 /= np.linalg.norm(d32, axis=1, keepdims=True)
    near, far = np.zeros(R), dist + 4.0
    k = np.arange(R) % 5
    near[k == 1] = (dist * rng.uniform(0.7, 1.2, R))[k == 1]
    far[k == 2] = (dist * rng.uniform(0.8, 1.3, R))[k == 2]
    near[k == 3], far[k == 3] = (dist - 0.1)[k == 3], (dist + 0.1)[k == 3]
    return torch.from_numpy(np.concatenate([o, d32, near[:, None], far[:, None], np.full((R, 1), 0.25)], 1).astype(np.float32)).cuda()


@pytest.mark.parametrize("R", [1, 63, 64, 65, 1000])
def test_clip_ray_counts(M, ball, R):
    grid, dense, _ = ball
    rays = _aimed_rays(R, seed=R)
    want = _check_clip(grid, dense, rays, f"R={R}")
    if R >= 63:
        assert 0 < want[2].sum() < R
    again = grid.clip_rays(rays)
    for a, b in zip(again, grid.clip_rays(rays)):                                             # two runs: bit-identical
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
    assert grid.clip_rays(rays[:0])[2].shape == (0,)                                          # R = 0 launches nothing


def test_clip_hand_built_rays(M, ball):
    grid, dense, _ = ball
    cx, cy, cz = BALL_C
    nan, inf = float("nan"), float("inf")
    rows = [
        # parallel to each axis through the ball (two components of d are exactly 0), inside the slab
        [-3, cy, cz, 1, 0, 0, 0, 9], [cx, -3, cz, 0, 1, 0, 0, 9], [cx, cy, -3, 0, 0, 1, 0, 9], [3, cy, cz, -1, 0, 0, 0, 9],
        # parallel to an axis, outside the slab of another (d_a == 0 and o_a outside [lo_a, hi_a])
        [-3, 0.31, cz, 1, 0, 0, 0, 9], [-3, cy, 1.21, 1, 0, 0, 0, 9], [1.01, cy, -3, 0, 0, 1, 0, 9], [cx, -0.30001, -3, 0, 0, 1, 0, 9],
        # on the slab's faces exactly: inside (the first one passes the dilated ball, the second an empty edge of the box)
        [-3, 0.3, cz, 1, 0, 0, 0, 9], [-3, -0.3, -1.2, 1, 0, 0, 0, 9],
        # origin inside the box: in the ball, beside it looking at it, beside it looking away
        [cx, cy, cz, 0, 0, 1, 0, 9], [cx - 0.6, cy, cz, 1, 0, 0, 0, 9], [cx - 0.6, cy, cz, -1, 0, 0, 0, 9],
        # missing the box entirely
        [-3, 2, 0, 1, 0, 0, 0, 9], [-3, 0, 0, 0.6, 0.8, 0, 0, 9], [0, 0, 5, 0, 0, 1, 0, 9],
        # through the box, through empty cells only
        [-3, cy, 0.9, 1, 0, 0, 0, 9], [-0.8, -3, 0.9, 0, 1, 0, 0, 9], [-3, -0.2, 1.0, 0.8, 0, -0.6, 0, 9],
        # near / far cutting the box segment (it runs from t = 2 to 4, the ball about 2.98 .. 3.42): before, inside, after
        [-3, cy, cz, 1, 0, 0, 0, 2.5], [-3, cy, cz, 1, 0, 0, 0, 3.2], [-3, cy, cz, 1, 0, 0, 0, 3.9],
        [-3, cy, cz, 1, 0, 0, 2.5, 9], [-3, cy, cz, 1, 0, 0, 3.2, 9], [-3, cy, cz, 1, 0, 0, 3.9, 9],
        [-3, cy, cz, 1, 0, 0, 3.1, 3.3], [-3, cy, cz, 1, 0, 0, 0, 1.5], [-3, cy, cz, 1, 0, 0, 4.5, 9],
        # near > far
        [-3, cy, cz, 1, 0, 0, 5, 1], [-3, cy, cz, 1, 0, 0, 3.3, 3.1],
        # never hidden: a NaN origin, an inf direction, a NaN far, an inf near
        [nan, cy, cz, 1, 0, 0, 0, 9], [-3, cy, cz, 1, inf, 0, 0, 9], [-3, cy, cz, 1, 0, 0, 0, nan], [-3, 2, 0, 1, 0, 0, -inf, 9],
        # a direction of length zero, inside the ball and outside the box; a short direction that runs out of steps
        [cx, cy, cz, 0, 0, 0, 0, 9], [-3, cy, cz, 0, 0, 0, 0, 9], [cx, cy, cz, 1e-4, 0, 0, 0, 9], [-0.9, -0.2, 1.0, 0, 1e-4, 0, 0, 9],
    ]
    rays = torch.tensor([r + [0.25] for r in rows], dtype=torch.float32).cuda()
    t_first, t_last, hit = _check_clip(grid, dense, rays, "hand-built")
    assert hit[0:4].tolist() == [1, 1, 1, 1] and hit[4:8].tolist() == [0, 0, 0, 0] and hit[8:10].tolist() == [1, 0]
    assert hit[10:13].tolist() == [1, 1, 0] and hit[13:19].tolist() == [0] * 6
    assert hit[19:28].tolist() == [0, 1, 1, 1, 1, 0, 1, 0, 0] and hit[28:30].tolist() == [0, 0]
    assert hit[30:34].tolist() == [1, 1, 1, 1] and hit[34:38].tolist() == [1, 0, 1, 1]
    assert 2.5 < t_first[0] < 2.98 and 3.42 < t_last[0] < 3.9                                 # the ball plus dilation plus a step
    assert t_first[10] == 0 and 2.5 < t_first[22] < 2.98 and t_first[23] == np.float32(3.2)
    assert t_last[20] == np.float32(3.2) and t_last[21] == t_last[0] and t_first[21] == t_first[0]
    for r in (30, 31, 33):
        assert t_first[r] == rays[r, 6].item() and t_last[r] == rays[r, 7].item()
    assert np.isnan(t_last[32]) and t_first[32] == 0
    assert t_last[36] == 9 and t_last[37] == 9 and t_first[37] == 0                           # out of steps: kept whole from there


def test_clip_full_frame(M, ball):
    """All 291 600 rays of a 540 x 540 frame: every lane position of every workgroup, 1140 workgroups."""
    from moco_flow_amd import camera
    grid, dense, _ = ball
    c2w = np.array([[1, 0, 0, 0.1], [0, 1, 0, 0.0], [0, 0, 1, 4.0]], dtype=np.float64)
    rays = camera.make_rays(540, 540, 1.2 * 540, (270, 270), c2w, 2.0, 6.0, -0.25)
    want = _check_clip(grid, dense, rays, "540 x 540")
    n_hit = int(want[2].sum())
    print(f"\n540 x 540: {n_hit} of {len(want[2])} rays hit")
    assert 1000 < n_hit < 291600 // 4


def test_clip_layout(M, ball):
    """A 10-column table, a 9-column view of it (row stride 10), every other row of a table (row stride 18), a transposed
    table (copied by the binding): each equals its contiguous copy and the oracle."""
    grid, dense, _ = ball
    rays9 = _aimed_rays(301, seed=9)
    rays10 = torch.cat([rays9, torch.full((301, 1), 0.5, device="cuda")], 1)
    want = _check_clip(grid, dense, rays10, "10 columns")
    for name, view in (("rows of 10, 9 seen", rays10[:, :9]), ("every other row", rays10[::2]), ("transposed", rays10.t().contiguous().t())):
        assert not view.is_contiguous(), name
        got, ref = grid.clip_rays(view), grid.clip_rays(view.contiguous())
        sel = slice(None, None, 2) if name == "every other row" else slice(None)
        for g, r, w in zip(got, ref, want):
            assert torch.equal(g.view(torch.int32) if g.dtype == torch.float32 else g, r.view(torch.int32) if r.dtype == torch.float32 else r), name
            _same(g, w[sel], name)
    out, hit = grid.cull(rays10[:, :9], "both")
    assert out.shape == (301, 9) and out.is_contiguous()
    _same(out[:, 6], want[0], "cull: near")
    _same(out[:, 7], want[1], "cull: far")
    _same(hit, want[2], "cull: hit")
    assert torch.equal(out[:, :6], rays9[:, :6]) and torch.equal(out[:, 8], rays9[:, 8])
    near_only, _ = grid.cull(rays10, "near")
    _same(near_only[:, 6], want[0], "near")
    assert torch.equal(near_only[:, 7], rays10[:, 7]) and torch.equal(near_only[:, 8:], rays10[:, 8:])
    none, _ = grid.cull(rays10, "none")
    assert torch.equal(none, rays10) and none.data_ptr() != rays10.data_ptr()


def test_other_steps_are_accepted(M, ball):
    grid, dense, _ = ball
    rays = _aimed_rays(200, seed=4)
    for step in (0.25, 1.0, 3.0):
        _check_clip(grid, dense, rays, f"step={step}", step)
    with pytest.raises(RuntimeError, match="65536"):
        grid.clip_rays(rays, 1e-4)
    with pytest.raises(RuntimeError, match="positive"):
        grid.clip_rays(rays, 0.0)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        grid.clip_rays(rays.cpu())


# ------------------------------------------------------------------------------------------------ from_field
@pytest.mark.parametrize("nof", ["none", "bw"])
def test_from_field_equals_its_two_steps(M, nof):
    """from_field == from_sigma(query_sigma(lattice)) word for word, canonical and through a backward NoF at an image index;
    the lattice is the oracle's (x slowest, z fastest)."""
    n = (9, 6, 34)
    case = dict(n=8, S=8, M=0, extra="ind" if nof == "bw" else "dir", regime="dense", nof=nof)
    embs, nerfs, kw = build_case(M, case, 0, device="cuda")
    aabb = np.array([[-0.9, -0.5, -1.1], [0.8, 0.6, 1.0]])
    flow = dict(bw_nof=kw["nof_models"][0], nof_embeddings=kw["nof_embeddings"], ind=-0.25) if nof == "bw" else {}
    pts, shape = O.lattice(n, aabb)
    xyz, shape_t = M.OccupancyGrid.lattice(n, aabb, "cuda")
    assert shape == n and shape_t == n and np.array_equal(xyz.cpu().numpy(), pts)
    with torch.no_grad():
        sigma = M.query_sigma(torch.from_numpy(pts).cuda(), nerfs[0], embs[0], precision="f32", **flow)
    sig = sigma.cpu().numpy().reshape(n)
    tau = float(np.median(np.log1p(np.exp(sig.astype(np.float64)))))                          # half the points active
    by_hand = M.OccupancyGrid.from_sigma(sigma.view(*n), aabb[0], aabb[1], tau, "softplus", 1)
    grid = M.OccupancyGrid.from_field(nerfs[0], embs[0], aabb, N_grid=n, sigma_threshold=tau, precision="f32", **flow)
    assert grid.dims == (8, 5, 33) and torch.equal(grid.bits, by_hand.bits)
    assert np.array_equal(grid.lo, aabb[0].astype(np.float32)) and np.array_equal(grid.hi, aabb[1].astype(np.float32))
    frac = grid.occupied_fraction()
    assert 0 < frac <= 1 and frac == by_hand.occupied_fraction()
    clear = ~O.ambiguous(sig, "softplus", tau)
    if clear.all():                                                                           # (else the oracle cannot say)
        assert np.array_equal(_words(grid), O.build(sig, "softplus", tau, 1)[0])
    cube = M.OccupancyGrid.from_field(nerfs[0], embs[0], aabb, N_grid=5, sigma_threshold=tau, dilate=0, precision="f32", **flow)
    assert cube.dims == (4, 4, 4) and tuple(cube.bits.shape) == (4, 4, 1)


# ------------------------------------------------------------------------------------------------ render_image
H = W = 24
N_RAND = 16


@pytest.fixture(scope="module")
def frame(M):
    """A 24 x 24 frame looking at the AABB [-1, 1]^3 from z = 4: rays, background, the hull mask, a render callable that
    records the ray tables it is given, and a grid with a ball in the middle of the box."""
    from moco_flow_amd import camera
    case = dict(n=8, S=8, M=8, extra="dir", regime="dense", test=True)
    embs, nerfs, kw = build_case(M, case, 0, device="cuda")
    focal = 1.2 * W
    c2w = np.array([[1, 0, 0, 0.0], [0, 1, 0, 0.0], [0, 0, 1, 4.0], [0, 0, 0, 1.0]], dtype=np.float64)
    K = np.array([[focal, 0, W / 2], [0, focal, H / 2], [0, 0, 1]], dtype=np.float64)
    corners = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float32)
    near, far = camera.near_far_from_aabb(corners, c2w)
    rays = camera.make_rays(H, W, focal, (W / 2, H / 2), c2w, near, far, -0.25)
    msk = camera.valid_rays_mask(corners, c2w, K, (H, W))
    bg = torch.rand(H * W, 3, generator=torch.Generator().manual_seed(3)).cuda()
    s = O.ball_lattice(17, (-1, -1, -1), (1, 1, 1), (0.1, -0.1, 0.0), 0.45)
    grid = M.OccupancyGrid.from_sigma(torch.from_numpy(s).cuda(), (-1, -1, -1), (1, 1, 1), 1.0, "softplus", 1)
    dense = O.build_dense(s, "softplus", 1.0, 1)
    seen = []
    fwd = functools.partial(M.render_rays, nerf_embeddings=embs, nerf_models=nerfs, **kw)

    def render(r, b):
        seen.append(r.detach().clone())
        with torch.no_grad():
            return fwd(r, b)
    return dict(rays=rays, bg=bg, msk=msk, grid=grid, dense=dense, render=render, seen=seen)


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def test_render_image_behind_a_grid(M, frame):
    from moco_flow_amd import image
    f = frame
    rays, bg, msk, grid = f["rays"], f["bg"], f["msk"], f["grid"]
    _, _, hit = _clip_oracle(grid, f["dense"], rays[msk])
    keep = torch.from_numpy(hit.astype(bool)).cuda()
    n_hull, n_keep = int(msk.sum()), int(keep.sum())
    assert 0 < n_hull < H * W and N_RAND < n_keep < n_hull                                   # culled and kept hull rays, several chunks
    kept = torch.zeros(H * W, dtype=torch.bool, device="cuda")
    kept[msk] = keep
    culled = msk & ~kept

    plain = image.render_image(rays, bg, f["render"], N_RAND, msk)
    explicit = image.render_image(rays, bg, f["render"], N_RAND, msk, occupancy=None)
    assert plain.keys() == explicit.keys()
    for k in plain:                                                                           # occupancy=None: today's dict
        assert torch.equal(_bits(plain[k]), _bits(explicit[k])), k

    f["seen"].clear()
    got = image.render_image(rays, bg, f["render"], N_RAND, msk, occupancy=grid)
    assert len(f["seen"]) == -(-n_keep // N_RAND) > 1
    assert torch.equal(torch.cat(f["seen"]), rays[kept])                                      # tighten="none": the rays as they were
    assert got.keys() == plain.keys()
    for typ in ("rgb_fine", "depth_fine"):
        assert torch.equal(_bits(got[typ][kept]), _bits(plain[typ][kept])), typ               # kept pixels: bit-identical
    assert torch.equal(got["rgb_fine"][culled], bg[culled]) and bool((got["depth_fine"][culled] == 8).all())
    assert torch.equal(got["rgb_fine"][~msk], bg[~msk]) and bool((got["depth_fine"][~msk] == 10).all())
    assert got["rgb_fine"].shape == (H * W, 3) and got["depth_fine"].shape == (H * W,)
    rank = keep.nonzero().squeeze(1)                                                          # position of a kept ray among the hull rays
    for k in plain:
        if k in ("rgb_fine", "depth_fine"):
            continue
        assert got[k].shape[0] == n_keep, k                                                   # one row per kept ray
        assert torch.equal(_bits(got[k]), _bits(plain[k][rank])), k

    # no mask: all rays are candidates, the image is composed all the same
    f["seen"].clear()
    full = image.render_image(rays, bg, f["render"], 64, None, occupancy=grid)
    _, _, hit_all = _clip_oracle(grid, f["dense"], rays)
    kept_all = torch.from_numpy(hit_all.astype(bool)).cuda()
    assert torch.equal(torch.cat(f["seen"]), rays[kept_all]) and torch.equal(kept_all[msk], keep)
    assert bool((full["depth_fine"][~kept_all] == 8).all()) and torch.equal(full["rgb_fine"][~kept_all], bg[~kept_all])
    assert torch.equal(_bits(full["rgb_fine"][kept]), _bits(plain["rgb_fine"][kept]))

    # a grid that culls every ray: every per-ray key is the render callable's empty-chunk result (what an all-false mask
    # renders), the hull pixels are "rendered, opacity 0", the others not rendered
    empty = M.OccupancyGrid.from_sigma(torch.full((5, 5, 5), -5.0, device="cuda"), (-1, -1, -1), (1, 1, 1), 1.0)
    assert empty.occupied_fraction() == 0
    f["seen"].clear()
    none = image.render_image(rays, bg, f["render"], N_RAND, msk, occupancy=empty)
    assert len(f["seen"]) == 1 and f["seen"][0].shape == (0, 9)
    ref = f["render"](rays[:0], bg[:0])
    assert none.keys() == ref.keys() == plain.keys()
    for k in ref:
        if k == "depth_fine":
            assert bool((none[k][msk] == 8).all()) and bool((none[k][~msk] == 10).all()) and none[k].shape == (H * W,)
        elif k == "rgb_fine":
            assert torch.equal(none[k], bg)
        else:
            assert none[k].shape == ref[k].shape and none[k].shape[0] == 0 and none[k].dtype == ref[k].dtype, k


@pytest.mark.parametrize("tighten", ["near", "both"])
def test_render_image_tightened(M, frame, tighten):
    """The table the render callable receives carries the oracle's t_first (and t_last) in columns 6 (and 7).  A ray with a
    NaN origin and one with a NaN far are kept, reach the render pass with their near / far untouched, and render what they
    render without a grid -- every per-ray output row and the composed pixel are bit-identical to that call, NaNs included.

    MEASURED on an MI355X: the fused render pass gives the NaN-origin ray opacity_coarse = opacity_fine = 1.0, not NaN (a NaN
    coordinate turns every pre-activation of the first layer into NaN, and the ReLU's max(x, 0) returns 0 for it), so "renders
    NaN" cannot be asserted of such a ray without changing the render kernels; what is asserted is that the grid never hides
    it and never changes what it renders."""
    from moco_flow_amd import image
    f = frame
    rays, bg, msk, grid = f["rays"].clone(), f["bg"], f["msk"], f["grid"]
    hull_px = msk.nonzero().squeeze(1)
    bad = [int(hull_px[5]), int(hull_px[-7])]
    rays[bad[0], 0] = float("nan")
    rays[bad[1], 7] = float("nan")
    t_first, t_last, hit = _clip_oracle(grid, f["dense"], rays[msk])
    keep = hit.astype(bool)
    pos = [int(msk[:b].sum()) for b in bad]                                                   # the two among the hull rays
    assert hit[pos[0]] == 1 and hit[pos[1]] == 1 and 0 < keep.sum() < len(keep)
    clean = _clip_oracle(grid, f["dense"], f["rays"][msk])[2]
    assert clean[pos[0]] == 0 and clean[pos[1]] == 0                                          # kept because they are not finite
    f["seen"].clear()
    got = image.render_image(rays, bg, f["render"], N_RAND, msk, occupancy=grid, tighten=tighten)
    table = torch.cat(f["seen"]).cpu().numpy()
    src = rays[msk].cpu().numpy()[keep]
    assert table.shape == src.shape
    _same(table[:, 6], t_first[keep], "column 6")
    _same(table[:, 7], t_last[keep] if tighten == "both" else src[:, 7], "column 7")
    _same(table[:, :6], src[:, :6], "o, d")
    _same(table[:, 8], src[:, 8], "idx")
    finite = np.isfinite(src[:, :8]).all(1)
    assert (~finite).sum() == 2 and (t_first[keep][finite] >= src[finite, 6]).all() and (t_first[keep] > src[:, 6]).any()
    assert (t_last[keep][finite] <= src[finite, 7]).all() and (t_last[keep] < src[:, 7]).any()
    plain = image.render_image(rays, bg, f["render"], N_RAND, msk)
    for b, p_ in zip(bad, pos):
        row = int(keep[:p_].sum())
        _same(table[row], rays[b].cpu().numpy(), "a non-finite ray reaches the render pass as it was")
        nan_keys = []
        for k in plain:
            if k in ("rgb_fine", "depth_fine"):
                assert torch.equal(_bits(got[k][b]), _bits(plain[k][b])), k                   # the composed pixel
            else:
                assert torch.equal(_bits(got[k][row]), _bits(plain[k][p_])), k                # the ray's own rows
                if bool(torch.isnan(plain[k][p_]).any()):
                    nan_keys.append(k)
        print(f"\ntighten={tighten}: non-finite ray at pixel {b}: NaN in {nan_keys or 'no per-ray output'}")
    with pytest.raises(RuntimeError, match="tighten"):
        image.render_image(rays, bg, f["render"], N_RAND, msk, occupancy=grid, tighten="far")


# ------------------------------------------------------------------------------------------------ streams
def test_build_and_clip_on_a_side_stream(M, ball):
    """Build + clip on stream B behind a hold: the lattice and the rays hold NaN until a copy ON B, behind the hold, fills
    them, and the blocks the outputs take were filled with 0xFF on B behind the hold.  A launch on any other stream reads
    NaN (every cell set, every ray kept whole) or is overwritten.  Equal to the serial result, bit for bit."""
    _, _, s = ball
    vol0, rays0 = torch.from_numpy(s).cuda(), _aimed_rays(500, seed=11)

    def fn(vol, rays):
        grid = M.OccupancyGrid.from_sigma(vol, LO, HI, 1.0, "softplus", 1)
        return (grid.bits, grid._count) + grid.clip_rays(rays)
    want = tuple(t.clone() for t in fn(vol0, rays0))
    torch.cuda.synchronize()
    _, b = independent_streams()
    xs = [torch.full_like(vol0, float("nan")), torch.full_like(rays0, float("nan"))]
    torch.cuda.synchronize()
    b.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(b):
        hold(b, HOLD_MS)
        for x, x0 in zip(xs, (vol0, rays0)):
            x.copy_(x0)
        filled, marker = torch.cuda.Event(), torch.cuda.Event()
        filled.record(b)
        marker.record(torch.cuda.default_stream())
        poison([t.numel() * t.element_size() for t in want])
        assert first_done(marker, filled), "producer was not delayed: the default stream did not run while B was held"
        got = fn(*xs)
        delayed = filled.query() is False
    b.synchronize()
    assert delayed, "producer was not delayed"
    for g, w in zip(got, want):
        assert torch.equal(_bits(g), _bits(w))
    assert 0 < int(want[4].sum()) < 500
