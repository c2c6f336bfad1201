"""moco_flow_amd.batch without a GPU: the package's exports and ctypes prototypes, the host-side argument validation of
mf_mask_compact / mf_ray_batch (include/mocoflow_hip.h) and of FrameRays' Python layer -- every refusal comes before any
launch --, and the torch restatement of the reference lines (tests/batch_oracle.py) on hand-computed values."""
import ctypes

import pytest
import torch

import batch_oracle as O


@pytest.fixture(scope="module")
def B():
    import moco_flow_amd
    return moco_flow_amd.batch


def test_package_exports_batch():
    import moco_flow_amd
    import moco_flow_amd._lib as L
    assert hasattr(moco_flow_amd, "batch") and moco_flow_amd.FrameRays is moco_flow_amd.batch.FrameRays
    assert set(moco_flow_amd.batch.__all__) == {"FrameRays"}
    for n in ("batch", "FrameRays"):
        assert n in moco_flow_amd.__all__ and hasattr(moco_flow_amd, n)
    lib = L.lib()
    C = ctypes
    want = {"mf_mask_compact_scratch_bytes": (C.c_int64, [C.c_int64]),
            "mf_mask_compact": (C.c_int32, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
            "mf_ray_batch": (C.c_int32, [C.POINTER(L.mf_ray_batch_args), C.c_void_p])}
    for sym, (res, args) in want.items():
        assert L.SYMBOLS[sym] == (res, args), sym
        fn = getattr(lib, sym)
        assert fn.restype is res and list(fn.argtypes) == args, sym
    assert lib.mf_version() == 16 and L.MF_ABI_VERSION == 16


def test_args_struct_layout():
    """The POD of include/mocoflow_hip.h, field by field: natural alignment, pointers on 8-byte boundaries."""
    import moco_flow_amd._lib as L
    A = L.mf_ray_batch_args
    off = {name: getattr(A, name).offset for name, _ in A._fields_}
    assert [off[k] for k in ("H", "W", "focal", "cx", "cy", "has_c2w", "c2w")] == [0, 4, 8, 12, 16, 20, 24]
    assert [off[k] for k in ("nearv", "farv", "idx", "has_chain", "chain_idx")] == [72, 76, 80, 84, 88]
    assert [off[k] for k in ("val_inds", "n_valid", "perm", "n_rows")] == [96, 104, 112, 120]
    assert [off[k] for k in ("image", "image_kind", "background", "background_kind")] == [128, 136, 144, 152]
    assert [off[k] for k in ("rays_out", "rgbs_out", "background_out", "sel_out")] == [160, 168, 176, 184]
    assert ctypes.sizeof(A) == 192
    assert (L.MF_IMAGE_NONE, L.MF_IMAGE_ROWS, L.MF_IMAGE_U8_RGB, L.MF_IMAGE_U8_RGBA) == (0, 1, 2, 3)
    assert (L.MF_BACKGROUND_NONE, L.MF_BACKGROUND_ROWS, L.MF_BACKGROUND_COLOUR) == (0, 1, 2)


def test_mask_compact_abi_validates_on_the_host():
    import moco_flow_amd._lib as L
    lib = L.lib()
    buf = (ctypes.c_int64 * 8)()
    p = ctypes.addressof(buf)
    # 8 bytes per workgroup; a workgroup takes 4096 bytes of the mask per trip; the grid stops growing at 1024 workgroups
    assert lib.mf_mask_compact_scratch_bytes(0) == 0
    assert lib.mf_mask_compact_scratch_bytes(1) == 8 and lib.mf_mask_compact_scratch_bytes(4096) == 8
    assert lib.mf_mask_compact_scratch_bytes(4097) == 16
    assert lib.mf_mask_compact_scratch_bytes(540 * 540) == 8 * 72
    assert lib.mf_mask_compact_scratch_bytes(4096 * 1024) == 8 * 1024
    assert lib.mf_mask_compact_scratch_bytes(4096 * 1024 + 1) == 8 * 513          # two trips each
    assert lib.mf_mask_compact_scratch_bytes(1 << 40) == 8 * 1024
    assert lib.mf_mask_compact_scratch_bytes(-1) == -1 and b"negative" in lib.mf_last_error()
    assert lib.mf_mask_compact(p, -4, p, p, p, None) == -1 and b"negative" in lib.mf_last_error()
    assert lib.mf_mask_compact(p, 4, p, None, p, None) == -1 and b"count" in lib.mf_last_error()
    assert lib.mf_mask_compact(p, 4, None, p, p, None) == -1 and b"inds_out" in lib.mf_last_error()
    assert lib.mf_mask_compact(p, 4, p, p, None, None) == -1 and b"scratch" in lib.mf_last_error()


def _args(L, **kw):
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    a = L.mf_ray_batch_args()
    a.H, a.W, a.focal, a.cx, a.cy = 4, 5, 10.0, 2.5, 2.0
    a.nearv, a.farv = 1.0, 2.0
    a.val_inds, a.n_valid, a.perm, a.n_rows = p, 20, p, 3
    a.rays_out, a.sel_out = p, p
    for k, v in kw.items():
        setattr(a, k, v)
    a._keep = buf
    return a, p


def test_ray_batch_abi_validates_on_the_host():
    import moco_flow_amd._lib as L
    lib = L.lib()
    call = lambda **kw: lib.mf_ray_batch(ctypes.byref(_args(L, **kw)[0]), None)
    _, p = _args(L)
    assert lib.mf_ray_batch(None, None) == -1 and b"null" in lib.mf_last_error()
    assert call(H=-1) == -1 and b"H=-1" in lib.mf_last_error()
    assert call(focal=0.0) == -1 and b"focal" in lib.mf_last_error()
    assert call(H=1 << 16, W=1 << 15, n_valid=0) == -1 and b"2^31" in lib.mf_last_error()      # H W = 2^31
    assert call(n_rows=-1) == -1 and b"n_rows=-1" in lib.mf_last_error()
    assert call(n_rows=1 << 31) == -1
    assert call(n_valid=21) == -1 and b"n_valid=21" in lib.mf_last_error()                      # more than H W
    assert call(image_kind=4) == -1 and b"image_kind=4" in lib.mf_last_error()
    assert call(background_kind=3) == -1 and b"background_kind=3" in lib.mf_last_error()
    assert call(image=p, rgbs_out=p, image_kind=L.MF_IMAGE_U8_RGBA) == -1 and b"needs a background" in lib.mf_last_error()
    assert call(image=p + 2, rgbs_out=p, image_kind=L.MF_IMAGE_U8_RGBA, background=p,
                background_kind=L.MF_BACKGROUND_COLOUR) == -1 and b"aligned" in lib.mf_last_error()
    for missing in ("val_inds", "perm", "rays_out"):
        assert call(**{missing: None}) == -1 and b"null" in lib.mf_last_error(), missing
    assert call(image_kind=L.MF_IMAGE_ROWS) == -1 and b"null image" in lib.mf_last_error()
    assert call(image=p, image_kind=L.MF_IMAGE_ROWS) == -1 and b"rgbs_out" in lib.mf_last_error()
    assert call(background_kind=L.MF_BACKGROUND_ROWS) == -1 and b"null background" in lib.mf_last_error()
    assert call(background_out=p) == -1 and b"without a background" in lib.mf_last_error()
    assert call(n_rows=0, val_inds=None, perm=None, rays_out=None) == 0                       # nothing is launched


def test_cpu_tensors_raise(B):
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        B.FrameRays(4, 5, 10.0, (2.5, 2.0), None, 1.0, 2.0, 0.0, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        B.FrameRays(4, 5, 10.0, (2.5, 2.0), None, 1.0, 2.0, 0.0, rays_msk=torch.ones(20, dtype=torch.bool), device="cpu")
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        B._image_kind(torch.zeros(20, 3), 4, 5)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        B._image_kind(torch.zeros(4, 5, 4, dtype=torch.uint8), 4, 5)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        B._background_kind(torch.zeros(3), 4, 5)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        B._check_perm(torch.arange(8), 8, None)


def test_bad_shapes_and_dtypes_raise(B):
    frame = lambda **kw: B.FrameRays(4, 5, 10.0, (2.5, 2.0), None, 1.0, 2.0, 0.0, **kw)
    for bad in (torch.ones(19, dtype=torch.bool), torch.ones(4, 5, dtype=torch.bool), torch.ones(20), torch.ones(20, dtype=torch.int64),
                [1] * 20):
        with pytest.raises(RuntimeError, match="rays_msk"):
            frame(rays_msk=bad)
    with pytest.raises(RuntimeError, match="H W < 2\\^31"):
        B.FrameRays(1 << 16, 1 << 15, 10.0, (2.5, 2.0), None, 1.0, 2.0, 0.0)
    with pytest.raises(RuntimeError, match="H=-1"):
        B.FrameRays(-1, 5, 10.0, (2.5, 2.0), None, 1.0, 2.0, 0.0)
    for bad in (torch.zeros(20, 3, dtype=torch.float64), torch.zeros(20, 4), torch.zeros(4, 5, 3), torch.zeros(5, 4, 3, dtype=torch.uint8),
                torch.zeros(4, 5, 2, dtype=torch.uint8), torch.zeros(20, 3, dtype=torch.uint8), "image"):
        with pytest.raises(RuntimeError, match="image"):
            B._image_kind(bad, 4, 5)
    for bad in (torch.zeros(4), torch.zeros(3, dtype=torch.float64), torch.zeros(20, 3, dtype=torch.uint8), torch.zeros(4, 5, 3), 0.5):
        with pytest.raises(RuntimeError, match="background"):
            B._background_kind(bad, 4, 5)
    for bad in (torch.arange(8, dtype=torch.int32), torch.arange(8).view(2, 4), torch.arange(8.0), list(range(8))):
        with pytest.raises(RuntimeError, match="perm"):
            B._check_perm(bad, 8, None)
    with pytest.raises(RuntimeError, match="7 entries, the batch needs 8"):
        B._check_perm(torch.arange(7), 8, None)
    assert B._image_kind(None, 4, 5) == 0 and B._background_kind(None, 4, 5) == 0


def test_oracle_on_hand_computed_values():
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    # one opaque, one transparent, one half-covered pixel over the colour (0.25, 0.5, 1)
    u8 = torch.tensor([[[255, 0, 51, 255], [10, 20, 30, 0], [255, 255, 0, 128]]], dtype=torch.uint8)
    bg = f([0.25, 0.5, 1.0])
    rgbs, back = O.composite(u8, bg, 1, 3)
    a = f(128.0) / f(255.0)
    assert rgbs.shape == (3, 3) and back.shape == (3, 3) and torch.equal(back, bg.expand(3, 3))
    assert torch.equal(rgbs[0], f([255.0, 0.0, 51.0]) / 255)                 # alpha 1: v * 1 + bg * 0
    assert torch.equal(rgbs[1], bg)
    assert torch.equal(rgbs[2], torch.stack([a + f(0.25) * (1 - a), a + f(0.5) * (1 - a), f(0.0) * a + f(1.0) * (1 - a)]))
    # rows as background, RGB input
    rows = torch.arange(9, dtype=torch.float32).view(3, 3) / 8
    rgbs, back = O.composite(u8, rows, 1, 3)
    assert torch.equal(back, rows) and torch.equal(rgbs[1], rows[1])
    rgb_only, none = O.composite(u8[..., :3].contiguous(), None, 1, 3)
    assert none is None and torch.equal(rgb_only, u8[0, :, :3].float() / 255)
    # selection: mask 0 1 1 0 1 -> val_inds 1 2 4; perm 2 0 1 -> pixels 4 1 2
    msk = torch.tensor([0, 1, 1, 0, 1], dtype=torch.bool)
    rays = torch.arange(45, dtype=torch.float32).view(5, 9)
    r, c, b, sel = O.select(rays, msk, rays[:, :3], None, torch.tensor([2, 0, 1]), 2)
    assert sel.tolist() == [4, 1] and torch.equal(r, rays[[4, 1]]) and torch.equal(c, rays[[4, 1], :3]) and b is None
    chained = O.chain_column(r, 0.1)
    assert chained.shape == (2, 10) and torch.equal(chained[:, :9], r) and torch.equal(chained[:, 9], f([0.1, 0.1]))
