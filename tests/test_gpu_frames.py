"""Frame ingest on the device (moco_flow_amd/frames.py, csrc/mf_frames.hip) against PIL's recorded outputs and the reference's
float64 plate expression (tests/golden/u_frames.npz) and against the numpy oracle (tests/frames_oracle.py, held to both by
tests/test_frames_cpu.py).  Every comparison is exact: the resize and the plate are integer arithmetic, the composite is fp32
rounded once per operation.  Sizes sit at the unit's own constants -- one workgroup's share and one either side of it, the
frame count at which the plate stops staging its keys in LDS -- and at shapes that are no multiple of anything."""
import json
import os
import re

import numpy as np
import pytest
import torch

import frames_oracle as FO

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = open(os.path.join(os.path.dirname(HERE), "moco_flow_amd", "csrc", "mf_frames.hip")).read()
_const = lambda name: int(re.search(r"\b%s = (\d+)" % name, _SRC).group(1))
RESIZE_SHARE = _const("kResizeThreads")                                       # output pixels of one resize workgroup
COMPOSITE_SHARE = _const("kCompositeThreads") * _const("kCompositePerThread")   # pixels of one composite workgroup
PLATE_TILE = _const("kPlateTilePixels")                                       # pixels of one staged plate workgroup
PLATE_BOUND = _const("kPlateLdsMaxFrames")                                    # the most frames whose keys fit in LDS
_GOLDEN = np.load(os.path.join(HERE, "golden", "u_frames.npz"))
_CASES = json.loads(str(_GOLDEN["cases"]))
DEV = "cuda"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _rgba(rng, shape):
    a = rng.integers(0, 256, size=tuple(shape) + (4,), dtype=np.uint8)
    fixed = rng.choice(np.array([0, 1, 3, 128, 254, 255], dtype=np.uint8), size=shape)
    a[..., 3] = np.where(rng.random(shape) < 0.6, fixed, a[..., 3])
    return a


# ---- resize ----

def test_fixture_covers_the_workgroup_share():
    sizes = {name: H * W for name, (_, H, W) in _CASES["resize"].items()}
    assert (sizes["share_minus"], sizes["share_exact"], sizes["share_plus"]) == (RESIZE_SHARE - 1, RESIZE_SHARE, RESIZE_SHARE + 1)


@pytest.mark.parametrize("case", sorted(_CASES["resize"]))
def test_resize_equals_pil(case):
    from moco_flow_amd import frames
    src, H, W = _CASES["resize"][case]
    a, want = _GOLDEN["in_" + src], _GOLDEN["resize_" + case]
    x = _dev(a)
    got = frames.resize(x, (H, W))
    assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape and got.is_contiguous()
    assert np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(frames.resize(x, (H, W)), got)                          # the same call, the same bytes
    one = frames.resize(x[-1], [H, W])                                         # a single frame keeps its rank
    assert tuple(one.shape) == want.shape[1:] and np.array_equal(one.cpu().numpy(), want[-1])
    assert np.array_equal(x.cpu().numpy(), a)                                  # the input is left alone


@pytest.mark.parametrize("C", [1, 3, 4])
def test_resize_odd_shapes_and_frame_strides(C):
    """Widths that are no multiple of 4 or of a wave, a non-integer ratio both ways, three frames of different content."""
    from moco_flow_amd import frames
    rng = np.random.default_rng(40 + C)
    for (H0, W0), (H, W) in (((41, 53), (17, 20)), ((19, 21), (30, 67)), ((41, 53), (41, 23)), ((41, 53), (13, 53)), ((7, 130), (3, 129))):
        a = _rgba(rng, (3, H0, W0)) if C == 4 else rng.integers(0, 256, size=(3, H0, W0, C), dtype=np.uint8)
        want = FO.resize(a, (H, W))
        assert not np.array_equal(want[0], want[1]) and not np.array_equal(want[1], want[2])
        assert np.array_equal(frames.resize(_dev(a), (H, W)).cpu().numpy(), want), ((H0, W0), (H, W))


def test_resize_identity_empty_and_views():
    from moco_flow_amd import frames
    x = _dev(_GOLDEN["in_a4"])
    same = frames.resize(x, (37, 53))
    assert torch.equal(same, x) and same.data_ptr() != x.data_ptr()            # a copy: no premultiply round trip
    assert tuple(frames.resize(x, (0, 5)).shape) == (3, 0, 5, 4) and tuple(frames.resize(x[:0], (4, 5)).shape) == (0, 4, 5, 4)
    view = x[:, 3:30, 5:47]                                                    # a strided view is resized as its contiguous copy
    assert np.array_equal(frames.resize(view, (11, 13)).cpu().numpy(), FO.resize(_GOLDEN["in_a4"][:, 3:30, 5:47], (11, 13)))
    with pytest.raises(RuntimeError, match=r"size must be \(H, W\)"):
        frames.resize(x, 16)
    with pytest.raises(RuntimeError):
        frames.resize(x[..., :2], (4, 4))


# ---- composite ----

@pytest.mark.parametrize("shape", [(1, COMPOSITE_SHARE - 1), (32, COMPOSITE_SHARE // 32), (25, (COMPOSITE_SHARE + 1) // 25), (3, 5)])
def test_composite_equals_oracle_and_the_batch_rows(shape):
    from moco_flow_amd import FrameRays, frames
    H, W = shape
    n = H * W
    assert n in (COMPOSITE_SHARE - 1, COMPOSITE_SHARE, COMPOSITE_SHARE + 1, 15)
    rng = np.random.default_rng(n)
    rgba = _rgba(rng, (H, W))
    rgba[0, :3, 3] = (0, 255, 77)                                              # transparent, opaque and in between
    rows = rng.random((n, 3), dtype=np.float32)
    colour = np.array([0.25, 1.0, 0.1], dtype=np.float32)
    plate = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    image = _dev(rgba)
    frame = FrameRays(H, W, 50.0, (W / 2, H / 2), None, 1.0, 2.0, 0.0, rays_msk=None, device=DEV)
    perm = torch.arange(n, device=DEV)
    for bg, bg_np in ((_dev(rows), rows), (_dev(colour), colour), (_dev(plate), FO.to_rows(plate))):
        got = frames.composite(image, bg)
        assert got.dtype == torch.float32 and tuple(got.shape) == (n, 3)
        assert np.array_equal(got.cpu().numpy(), FO.composite(rgba, bg_np))
        batch_bg = frames.to_rows(bg) if bg.dtype == torch.uint8 else bg
        assert torch.equal(got, frame.sample(n, image, batch_bg, perm=perm)[1])         # row for row what a training batch gets
    # buffers that are only 4-byte aligned take the unvectorised loads and stores
    off = torch.empty(n * 3 + 1, dtype=torch.float32, device=DEV)
    off[1:] = _dev(rows).reshape(-1)
    assert np.array_equal(frames.composite(image, off[1:].view(n, 3)).cpu().numpy(), FO.composite(rgba, rows))
    # an RGB image: bytes to rows
    assert np.array_equal(frames.to_rows(_dev(plate)).cpu().numpy(), FO.to_rows(plate))
    assert torch.equal(frames.to_rows(_dev(plate)), frame.sample(n, _dev(plate), None, perm=perm)[1])
    assert torch.equal(frames.composite(_dev(plate)), frames.to_rows(_dev(plate)))


def test_composite_refusals():
    from moco_flow_amd import frames
    image = _dev(_rgba(np.random.default_rng(0), (4, 6)))
    for bad in (None, torch.zeros(4, device=DEV), torch.zeros((24, 3), dtype=torch.float64, device=DEV), torch.zeros((4, 6, 4), dtype=torch.uint8, device=DEV)):
        with pytest.raises(RuntimeError):
            frames.composite(image, bad)
    with pytest.raises(RuntimeError, match="no alpha"):
        frames.composite(image[..., :3], torch.zeros(3, device=DEV))
    with pytest.raises(RuntimeError):
        frames.to_rows(image)
    assert tuple(frames.composite(image[:0], torch.zeros(3, device=DEV)).shape) == (0, 3)


# ---- background plate ----

@pytest.mark.parametrize("case", sorted(_CASES["plate"]))
def test_plate_equals_the_float64_expression(case):
    from moco_flow_amd import frames
    F, H, W, C, k, soft = _CASES["plate"][case]
    fr, ms = _GOLDEN[f"plate_{case}_frames"], _GOLDEN[f"plate_{case}_masks"]
    want = np.floor(255.0 * _GOLDEN[f"plate_{case}_f64"] + 0.5).astype(np.uint8)
    got = frames.background_plate(_dev(fr), _dev(ms))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (H, W, 3)
    assert np.array_equal(got.cpu().numpy(), want)
    for path in ("staged", "streamed"):                                        # both kernels, the same bytes
        assert torch.equal(frames.background_plate(_dev(fr), _dev(ms), path=path), got), path


@pytest.mark.parametrize("F", [1, 2, 5, PLATE_BOUND - 1, PLATE_BOUND, PLATE_BOUND + 1])
def test_plate_frame_counts_around_the_lds_bound(F):
    """PLATE_BOUND + 1 frames no longer fit in LDS: "auto" streams them (and "staged" refuses)."""
    from moco_flow_amd import frames
    rng = np.random.default_rng(F)
    for C, soft in ((4, True), (3, False)):
        fr, ms = FO.plate_inputs(rng, F, 8, 8, C, soft)
        if C == 4:
            fr[..., :3] = rng.integers(0, 256, size=fr[..., :3].shape)        # every byte value, not only the tied ones
        want = FO.plate(fr, ms, int(F * 0.8))
        assert (want.reshape(-1, 3)[0] == 0).all()                            # masked in every frame
        got = frames.background_plate(_dev(fr), _dev(ms))
        assert np.array_equal(got.cpu().numpy(), want), (F, C)
        assert torch.equal(frames.background_plate(_dev(fr), _dev(ms)), got)
        assert torch.equal(frames.background_plate(_dev(fr), _dev(ms), path="streamed"), got)
        for q, k in ((0.0, 0), (1.0 - 0.5 / F, F - 1)):                       # the smallest and the largest key
            assert np.array_equal(frames.background_plate(_dev(fr), _dev(ms), q=q).cpu().numpy(), FO.plate(fr, ms, k)), (F, C, q)
    if F > PLATE_BOUND:
        with pytest.raises(RuntimeError, match="staged"):
            frames.background_plate(_dev(fr), _dev(ms), path="staged")


@pytest.mark.parametrize("shape", [(1, PLATE_TILE - 1), (8, PLATE_TILE // 8), (5, (PLATE_TILE + 1) // 5), (7, 37)])
def test_plate_pixel_counts_around_the_tile(shape):
    from moco_flow_amd import frames
    H, W = shape
    assert H * W in (PLATE_TILE - 1, PLATE_TILE, PLATE_TILE + 1, 259)
    rng = np.random.default_rng(H * W)
    for C, soft in ((3, True), (4, False)):
        fr, ms = FO.plate_inputs(rng, 9, H, W, C, soft)
        want = FO.plate(fr, ms, 7)
        for path in ("auto", "staged", "streamed"):
            assert np.array_equal(frames.background_plate(_dev(fr), _dev(ms), path=path).cpu().numpy(), want), (C, path)


def test_plate_refusals():
    from moco_flow_amd import frames
    fr, ms = (_dev(a) for a in FO.plate_inputs(np.random.default_rng(1), 5, 4, 6, 4, True))
    for q in (1.0, -0.3):
        with pytest.raises(RuntimeError, match="k="):
            frames.background_plate(fr, ms, q=q)
    with pytest.raises(RuntimeError):
        frames.background_plate(fr, ms[:4])
    with pytest.raises(RuntimeError):
        frames.background_plate(fr[..., :2], ms)
    with pytest.raises(RuntimeError, match="path"):
        frames.background_plate(fr, ms, path="lds")
    assert tuple(frames.background_plate(fr[:, :0], ms[:, :0]).shape) == (0, 6, 3)


# ---- from raw frames to validation rows ----

def test_raw_frames_to_composited_rows():
    from moco_flow_amd import frames
    rng = np.random.default_rng(77)
    raw = _rgba(rng, (5, 37, 53))
    masks = FO.plate_inputs(rng, 5, 37, 53, 4, True)[1]
    plate = frames.background_plate(_dev(raw), _dev(masks))
    small = frames.resize(_dev(raw)[0], (16, 20))
    small_plate = frames.resize(plate, (16, 20))
    rows = frames.composite(small, frames.to_rows(small_plate))
    want_plate = FO.plate(raw, masks, 4)
    want_small, want_small_plate = FO.resize(raw[0], (16, 20)), FO.resize(want_plate, (16, 20))
    assert np.array_equal(plate.cpu().numpy(), want_plate) and np.array_equal(small_plate.cpu().numpy(), want_small_plate)
    assert np.array_equal(rows.cpu().numpy(), FO.composite(want_small, FO.to_rows(want_small_plate)))
    assert torch.equal(rows, frames.composite(small, small_plate))             # the byte plate as the background: the same rows
