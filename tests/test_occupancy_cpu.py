"""moco_flow_amd.occupancy without a GPU: the header, the ABI version and the ctypes prototypes of mf_occ_build / mf_ray_clip,
their host-side argument validation through the loaded library (every refusal comes before any launch), and two properties
of the numpy restatement (tests/occupancy_oracle.py) that the GPU tests then hold the kernels to: the dilation rule, and the
conservativeness of the march that OccupancyGrid.clip_rays promises."""
import ctypes
import os

import numpy as np
import pytest
import torch

import occupancy_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_lists_the_entries_and_the_abi_stays_16():
    import moco_flow_amd
    import moco_flow_amd._lib as L
    text = open(os.path.join(ROOT, "include", "mocoflow_hip.h")).read()
    additive = text[text.index("additive entries since, version unchanged"):text.index("#define MF_ABI_VERSION")]
    for name in ("mf_occ_build", "mf_occ_build_scratch_bytes", "mf_ray_clip"):
        assert name in additive, name
    assert "#define MF_ABI_VERSION 16" in text
    for entry in ("mf_occ_build (serves", "mf_ray_clip (serves"):                   # each entry cites the lines it serves
        doc = text[text.index(entry):]
        doc = doc[:doc.index("*/")]
        for cite in ("trainer_moco_flow.py:226-268", "utils/camera.py:134-148", "rendering.py:239-249"):
            assert cite in doc, (entry, cite)
    C = ctypes
    want = {"mf_occ_build_scratch_bytes": (C.c_int64, [C.c_int64, C.c_int64, C.c_int64]),
            "mf_occ_build": (C.c_int32, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_float, C.c_int32,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
            "mf_ray_clip": (C.c_int32, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                        C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])}
    lib = L.lib()
    for sym, (res, args) in want.items():
        assert L.SYMBOLS[sym] == (res, args), sym
        fn = getattr(lib, sym)
        assert fn.restype is res and list(fn.argtypes) == args, sym
    assert lib.mf_version() == 16 and L.MF_ABI_VERSION == 16
    assert moco_flow_amd.OccupancyGrid is moco_flow_amd.occupancy.OccupancyGrid
    for n in ("occupancy", "OccupancyGrid"):
        assert n in moco_flow_amd.__all__


def _f3(*v):
    return (ctypes.c_float * 3)(*v)


def test_build_validates_on_the_host():
    import moco_flow_amd._lib as L
    lib = L.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    build = lambda nx=3, ny=3, nz=3, act=1, tau=1.0, r=1, sigma=p, bits=p, count=None, scratch=None: \
        lib.mf_occ_build(sigma, nx, ny, nz, act, tau, r, bits, count, scratch, None)
    for bad in ((1, 3, 3), (3, 1, 3), (3, 3, 1), (0, 3, 3), (3, -2, 3)):           # a lattice dimension < 2
        assert build(*bad) == -1 and b"each side >= 2" in lib.mf_last_error(), bad
        assert lib.mf_occ_build_scratch_bytes(*bad) == -1 and b"each side >= 2" in lib.mf_last_error(), bad
    assert build((1 << 11) + 1, (1 << 11) + 1, (1 << 9) + 1) == -1 and b"2^31" in lib.mf_last_error()   # exactly 2^31 cells
    assert build(2, 2, (1 << 31) + 1) == -1 and b"2^31" in lib.mf_last_error()
    assert lib.mf_occ_build_scratch_bytes(2, 2, 1 << 31) == -1
    assert build(act=2) == -1 and b"activation=2" in lib.mf_last_error()
    assert build(r=3) == -1 and b"dilate=3" in lib.mf_last_error()
    assert build(r=-1) == -1 and b"dilate=-1" in lib.mf_last_error()
    assert build(tau=float("nan")) == -1 and b"NaN" in lib.mf_last_error()
    assert build(sigma=None) == -1 and b"null" in lib.mf_last_error()
    assert build(bits=None) == -1 and b"null" in lib.mf_last_error()               # a null output
    assert build(count=p) == -1 and b"scratch" in lib.mf_last_error()
    # one double per workgroup of 256 words
    assert lib.mf_occ_build_scratch_bytes(3, 3, 3) == 8
    assert lib.mf_occ_build_scratch_bytes(34, 6, 65) == 16                           # 33 * 5 * 2 = 330 words
    assert lib.mf_occ_build_scratch_bytes(128, 128, 128) == 8 * 253                  # 127 * 127 * 4 = 64516 words


def test_ray_clip_validates_on_the_host():
    import moco_flow_amd._lib as L
    lib = L.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)

    def clip(rays=p, stride=9, R=4, bits=p, g=(4, 4, 4), lo=(-1, -1, -1), hi=(1, 1, 1), inv=(2, 2, 2), dt=0.25,
             t_first=p, t_last=p, hit=p):
        return lib.mf_ray_clip(rays, stride, R, bits, g[0], g[1], g[2], _f3(*lo) if lo else None, _f3(*hi) if hi else None,
                               _f3(*inv) if inv else None, dt, t_first, t_last, hit, None)

    assert clip(dt=0.0) == -1 and b"positive" in lib.mf_last_error()
    assert clip(dt=-0.25) == -1 and b"positive" in lib.mf_last_error()
    assert clip(dt=float("nan")) == -1 and b"positive" in lib.mf_last_error()
    assert clip(lo=(1, -1, -1), hi=(-1, 1, 1)) == -1 and b"inverted box on axis 0" in lib.mf_last_error()
    assert clip(lo=(-1, -1, 1), hi=(1, 1, 1)) == -1 and b"box on axis 2" in lib.mf_last_error()       # empty
    # |hi - lo| = 2 sqrt(3) = 3.4641: floor(3.4641 / dt) + 2 steps.  dt = 5.29e-5 -> 65485 steps (accepted, with R = 0),
    # dt = 5.28e-5 -> 65609
    assert clip(dt=5.28e-5) == -1 and b"65536" in lib.mf_last_error()
    assert clip(dt=5.28e-5, R=0) == -1                                               # refused whatever R is
    assert clip(dt=5.29e-5, R=0) == 0
    for out in ("t_first", "t_last", "hit"):                                         # a null output
        assert clip(**{out: None}) == -1 and b"null output" in lib.mf_last_error(), out
    assert clip(rays=None) == -1 and b"null rays" in lib.mf_last_error()
    assert clip(bits=None) == -1 and b"null rays or bits" in lib.mf_last_error()
    assert clip(lo=None) == -1 and b"null lo" in lib.mf_last_error()
    assert clip(stride=7) == -1 and b"ray_stride=7" in lib.mf_last_error()
    assert clip(R=-1) == -1 and b"n_rays=-1" in lib.mf_last_error()
    assert clip(g=(0, 4, 4)) == -1 and b"cells" in lib.mf_last_error()
    assert clip(g=(1 << 11, 1 << 10, 1 << 10)) == -1 and b"2^31" in lib.mf_last_error()
    assert clip(inv=(2, 0, 2)) == -1 and b"inv_cell[1]" in lib.mf_last_error()
    assert clip(R=0, rays=None, t_first=None, t_last=None, hit=None) == 0           # R = 0: nothing is launched


def test_cpu_tensors_raise():
    from moco_flow_amd.occupancy import OccupancyGrid
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        OccupancyGrid.from_sigma(torch.zeros(3, 3, 3), (-1, -1, -1), (1, 1, 1), 1.0)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        OccupancyGrid(torch.zeros(2, 2, 1, dtype=torch.int32), (2, 2, 2), (-1, -1, -1), (1, 1, 1))


@pytest.mark.parametrize("dilate", [0, 1, 2])
def test_dilation_is_a_max_filter_of_the_thresholded_lattice(dilate):
    """The oracle's build against the rule spelled out cell by cell: cell (i, j, k) is set iff some lattice point of
    [i-r, i+1+r] x [j-r, j+1+r] x [k-r, k+1+r], clipped to the lattice, exceeds tau."""
    rng = np.random.default_rng(3 + dilate)
    n = (6, 4, 36)
    sigma = rng.normal(0.0, 1.0, n).astype(np.float32)
    tau = 1.6                                                                        # about 5 % of the points
    sigma[2, 1, 7] = np.nan                                                          # counts as set
    sigma[4, 2, 20] = np.float32(tau)                                                # equal: not set
    on = ~(np.where(sigma < 0, 0, sigma) <= np.float32(tau))
    assert on[2, 1, 7] and not on[4, 2, 20] and 0 < on.sum() < on.size // 4
    want = np.zeros((n[0] - 1, n[1] - 1, n[2] - 1), dtype=bool)
    r = dilate
    for i in range(n[0] - 1):
        for j in range(n[1] - 1):
            for k in range(n[2] - 1):
                want[i, j, k] = on[max(i - r, 0):i + 2 + r, max(j - r, 0):j + 2 + r, max(k - r, 0):k + 2 + r].any()
    got = O.build_dense(sigma, "relu", tau, dilate)
    assert np.array_equal(got, want)
    words, count = O.build(sigma, "relu", tau, dilate)
    assert words.shape == (5, 3, 2) and words.dtype == np.uint32 and count == want.sum()
    assert np.array_equal(O.unpack(words, 35), want)
    assert (words[:, :, 1] >> np.uint32(3) == 0).all()                               # 35 cells: bits 3 .. 31 of the second word are padding


def _random_rays(rng, R, lo, hi):
    """Unit-direction rays aimed at random points of the box from outside and inside it, with assorted [near, far]."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    target = rng.uniform(lo, hi, (R, 3))
    o = rng.normal(0.0, 1.0, (R, 3))
    o = o / np.linalg.norm(o, axis=1, keepdims=True) * rng.uniform(0.2, 3.0, (R, 1)) * np.linalg.norm(hi - lo)
    o[::9] = rng.uniform(lo, hi, (len(o[::9]), 3))                                   # origins inside the box
    d = target - o
    dist = np.linalg.norm(d, axis=1, keepdims=True)
    d = d / dist
    d32 = d.astype(np.float32)
    d32 = d32 / np.linalg.norm(d32, axis=1, keepdims=True).astype(np.float32)
    near = np.zeros(R)
    far = dist[:, 0] + np.linalg.norm(hi - lo)
    cutn, cutf = np.arange(R) % 4 == 1, np.arange(R) % 4 == 2                        # near / far cutting the box segment
    near[cutn] = dist[cutn, 0] * rng.uniform(0.6, 1.1, cutn.sum())
    far[cutf] = dist[cutf, 0] * rng.uniform(0.9, 1.3, cutf.sum())
    rays = np.concatenate([o, d32, near[:, None], far[:, None], np.zeros((R, 1))], 1).astype(np.float32)
    return rays


def test_march_is_conservative():
    """200 random rays against random sparse grids of (9, 7, 12) cells, about 5 % set, dilated by 1 cell, step = 0.5: a dense
    walk at 1 / 64 of a cell (float64) through the UNDILATED grid finds the parameters at which a ray is inside a set cell
    within [near, far]; every ray with such a parameter has hit = 1 and every such parameter lies in [t_first, t_last]."""
    G = (9, 7, 12)
    lo, hi = np.array([-1.0, -0.7, -1.3]), np.array([0.8, 0.9, 1.1])
    crossing = 0
    for trial in range(4):
        rng = np.random.default_rng(100 + trial)
        raw = rng.random(G) < 0.05
        dil = np.zeros(G, dtype=bool)                                                # dilation of the CELLS by one cell
        for c in np.argwhere(raw):
            dil[max(c[0] - 1, 0):c[0] + 2, max(c[1] - 1, 0):c[1] + 2, max(c[2] - 1, 0):c[2] + 2] = True
        rays = _random_rays(rng, 50, lo, hi)
        lo32, hi32, inv, dt = O.grid_constants(G, lo, hi, 0.5)
        t_first, t_last, hit = O.clip(rays, dil, lo32, hi32, inv, dt)
        edge = (hi32.astype(np.float64) - lo32.astype(np.float64)) / np.array(G)
        fine = edge.min() / 64
        for r in range(len(rays)):
            o, d, near, far = rays[r, 0:3].astype(np.float64), rays[r, 3:6].astype(np.float64), float(rays[r, 6]), float(rays[r, 7])
            t = np.arange(near, far, fine)
            p = o + d * t[:, None]
            c = np.floor((p - lo32.astype(np.float64)) / edge).astype(np.int64)
            inside = ((c >= 0) & (c < np.array(G))).all(1)
            occ = np.zeros(len(t), dtype=bool)
            occ[inside] = raw[c[inside, 0], c[inside, 1], c[inside, 2]]
            if occ.any():
                crossing += 1
                assert hit[r] == 1, (trial, r)
                assert t_first[r] <= t[occ].min() and t[occ].max() <= t_last[r], (trial, r, t_first[r], t[occ].min(), t[occ].max(), t_last[r])
            assert t_first[r] >= np.float32(near) and t_last[r] <= np.float32(far)
        assert 0 < hit.sum() < len(rays)                                             # some culled, some kept
    assert crossing >= 20


def test_build_rule_dilated_covers_the_cell_dilation():
    """The build's rule at dilate = 1 (lattice points of [i-1, i+2]^3) sets at least every cell next to a cell set at
    dilate = 0: what the conservativeness argument needs from it."""
    rng = np.random.default_rng(7)
    sigma = np.where(rng.random((10, 8, 13)) < 0.02, 5.0, -5.0).astype(np.float32)
    raw, d1 = O.build_dense(sigma, "softplus", 1.0, 0), O.build_dense(sigma, "softplus", 1.0, 1)
    assert raw.any() and not O.ambiguous(sigma, "softplus", 1.0).any()
    for c in np.argwhere(raw):
        assert d1[max(c[0] - 1, 0):c[0] + 2, max(c[1] - 1, 0):c[1] + 2, max(c[2] - 1, 0):c[2] + 2].all()


def test_march_on_hand_computed_values():
    """One set cell in a 4 x 4 x 4 grid over [0, 4]^3, dt = 0.5: an axis-parallel ray through it, one beside it, one outside
    the slab, a NaN ray and near > far."""
    dense = np.zeros((4, 4, 4), dtype=bool)
    dense[2, 1, 1] = True
    lo, hi, inv, dt = O.grid_constants((4, 4, 4), (0, 0, 0), (4, 4, 4), 0.5)
    assert dt == 0.5 and (inv == 1).all()
    nan = float("nan")
    rays = np.array([[-1, 1.5, 1.5, 1, 0, 0, 0, 10, 0],          # enters at t = 1; samples at 1 + k/2; cell x = 2 for t in [3, 4)
                     [-1, 2.5, 1.5, 1, 0, 0, 0, 10, 0],          # same, one cell beside: miss
                     [-1, 4.5, 1.5, 1, 0, 0, 0, 10, 0],          # d_y == 0 outside the slab: miss
                     [-1, 1.5, 1.5, 1, 0, 0, 3.25, 10, 0],       # near inside the cell: samples at 3.25, 3.75, ...
                     [-1, 1.5, 1.5, 1, 0, 0, 0, 2.9, 0],         # far in front of the cell: miss
                     [-1, 1.5, 1.5, 1, 0, 0, 6, 2, 0],           # near > far: miss
                     [nan, 1.5, 1.5, 1, 0, 0, 0, 10, 0],         # never hidden
                     [-1, 1.5, 1.5, 1, 0, 0, 0, nan, 0]], dtype=np.float32)
    t_first, t_last, hit = O.clip(rays, dense, lo, hi, inv, dt)
    assert hit.tolist() == [1, 0, 0, 1, 0, 0, 1, 1]
    assert t_first[0] == 2.5 and t_last[0] == 4.0                # kf = 4 (t = 3), kl = 5 (t = 3.5)
    assert t_first[3] == 3.25 and t_last[3] == 4.25              # kf = 0: max(near, 2.75); kl = 1 (t = 3.75)
    for r in (1, 2, 4, 5):
        assert t_first[r] == rays[r, 6] and t_last[r] == rays[r, 7]
    assert t_first[6] == 0 and t_last[6] == 10 and t_first[7] == 0 and np.isnan(t_last[7])
