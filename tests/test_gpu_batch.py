"""moco_flow_amd.batch on the device (mf_batch.hip) against the eager op sequence of the reference it replaces: the full
camera.make_rays table, torch.nonzero, the gathers, and the torch restatement of the dataset's compositing
(tests/batch_oracle.py).

Every comparison is EXACT -- torch.equal, no tolerance anywhere: the compaction is integer work, a batch row comes from the
very device function mf_make_rays evaluates for that pixel, a gather copies, and the 8-bit compositing is the torch
expression operation for operation as the device evaluates it (/ 255 is there a product with the fp32 reciprocal of 255; then
every product, difference and sum rounded once).

Sizes: one byte, one wave of the compaction +- 1, 37 x 53 (no multiple of a wave or a workgroup), 300 x 300 (22 workgroups:
the scan of the counts), and one mask past the point where the compaction's grid stops growing (its constants are read from
the unit), where every workgroup takes a second trip."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import batch_oracle as O
from helpers import RENDER_CASES, build_case, load_golden

pytestmark = pytest.mark.gpu

_SRC = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "moco_flow_amd", "csrc", "mf_batch.hip")).read()
_const = lambda name: int(re.search(r"\b%s = (\d+)" % name, _SRC).group(1))
TILE = _const("kCompactThreads") * _const("kCompactPerLane")       # mask bytes of one workgroup trip
MAX_BLOCKS = _const("kCompactMaxBlocks")
BIG_N = MAX_BLOCKS * TILE + TILE + 5                               # two trips per workgroup, the last one ragged
assert 37 * 53 < TILE < 300 * 300 < MAX_BLOCKS * TILE

FRAMES = [(37, 53), (300, 300)]
NEAR, FAR, IDX = 1.37, 5.11, 0.375


@pytest.fixture(scope="module")
def M():
    import moco_flow_amd
    return moco_flow_amd


def intrinsics(H, W):
    """focal and an off-centre principal point."""
    return 61.7, (0.31 * W + 1.25, 0.77 * H - 0.5)


@functools.lru_cache(maxsize=None)
def golden_c2w():
    return load_golden("u_camera")["in_c2w"]


@functools.lru_cache(maxsize=None)
def full_rays(H, W, with_c2w):
    """The (H W, 9) table the reference keeps per frame: computed once, shared, never written."""
    from moco_flow_amd import camera
    focal, center = intrinsics(H, W)
    return camera.make_rays(H, W, focal, center, golden_c2w() if with_c2w else None, NEAR, FAR, IDX)


@functools.lru_cache(maxsize=None)
def frame_mask(H, W):
    """A seeded hull-like mask: a disc with a ragged rim, about half of the frame."""
    gen = torch.Generator().manual_seed(H * 1000 + W)
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    r = ((y - 0.45 * H) / (0.42 * H)) ** 2 + ((x - 0.55 * W) / (0.42 * W)) ** 2
    return (r + 0.2 * torch.rand(H, W, generator=gen) < 1.0).reshape(-1).cuda()


@functools.lru_cache(maxsize=None)
def frame(H, W, with_c2w, masked=True):
    import moco_flow_amd
    focal, center = intrinsics(H, W)
    return moco_flow_amd.FrameRays(H, W, focal, center, golden_c2w() if with_c2w else None, NEAR, FAR, IDX,
                                   rays_msk=frame_mask(H, W) if masked else None)


@functools.lru_cache(maxsize=None)
def pictures(H, W):
    """(rgba uint8 (H, W, 4) with alpha 0, 255 and random values; fp32 image rows; background rows; one colour), on the device."""
    gen = torch.Generator().manual_seed(H * 7 + W)
    rgba = torch.randint(0, 256, (H, W, 4), dtype=torch.uint8, generator=gen)
    third = torch.randint(0, 3, (H, W), generator=gen)
    rgba[..., 3][third == 0] = 0
    rgba[..., 3][third == 1] = 255
    assert (rgba[..., 3] == 0).any() and (rgba[..., 3] == 255).any() and ((rgba[..., 3] > 0) & (rgba[..., 3] < 255)).any()
    rows = torch.rand(H * W, 3, generator=gen)
    back = torch.rand(H * W, 3, generator=gen)
    colour = torch.tensor([0.25, 0.6, 0.9])
    return rgba.cuda(), rows.cuda(), back.cuda(), colour.cuda()


def seeded_perm(n_valid, seed=0):
    return torch.randperm(n_valid, generator=torch.Generator().manual_seed(seed)).cuda()


def raw_compact(mask, n):
    """mf_mask_compact on a device uint8 tensor (or None) -> (the whole n-entry output buffer, prefilled with -7; count)."""
    import moco_flow_amd._lib as L
    lib = L.lib()
    inds = torch.full((max(n, 1),), -7, dtype=torch.int64, device="cuda")
    count = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    scratch = torch.empty(max(int(lib.mf_mask_compact_scratch_bytes(n)), 8), dtype=torch.uint8, device="cuda")
    L.check(lib.mf_mask_compact(L.ptr(mask), n, inds.data_ptr(), count.data_ptr(), scratch.data_ptr(),
                                L.current_stream(inds.device)), "mf_mask_compact")
    return inds[:n], int(count.item())


def masks_of(n):
    gen = torch.Generator().manual_seed(n)
    one_at = lambda k: torch.zeros(n, dtype=torch.uint8).index_fill_(0, torch.tensor([k]), 1)
    other = torch.tensor([0, 255, 2, 128, 0, 1], dtype=torch.uint8)[torch.randint(0, 6, (n,), generator=gen)]
    kinds = {"zeros": torch.zeros(n, dtype=torch.uint8), "ones": torch.ones(n, dtype=torch.uint8), "first": one_at(0),
             "last": one_at(n - 1), "d0.01": (torch.rand(n, generator=gen) < 0.01).to(torch.uint8),
             "d0.5": (torch.rand(n, generator=gen) < 0.5).to(torch.uint8), "other bytes": other}
    if n == BIG_N:                                  # the second trip: a full share, a ragged end, a dense draw
        kinds = {k: kinds[k] for k in ("ones", "last", "d0.5")}
    return kinds


@pytest.mark.parametrize("n", [1, 63, 64, 65, 37 * 53, 300 * 300, BIG_N])
def test_compaction_equals_nonzero(n):
    for kind, mask in masks_of(n).items():
        mask = mask.cuda()
        want = torch.nonzero(mask).squeeze(1)
        buf, count = raw_compact(mask, n)
        assert count == want.numel(), (n, kind)
        assert torch.equal(buf[:count], want), (n, kind)
        assert bool((buf[count:] == -7).all()), (n, kind)          # nothing is written past the count
        again, count2 = raw_compact(mask, n)
        assert count2 == count and torch.equal(again, buf), (n, kind)
    ident, count = raw_compact(None, n)
    assert count == n and torch.equal(ident, torch.arange(n, device="cuda"))


def test_compaction_of_nothing():
    buf, count = raw_compact(torch.zeros(1, dtype=torch.uint8, device="cuda"), 0)
    assert count == 0 and buf.numel() == 0
    assert raw_compact(None, 0)[1] == 0


@pytest.mark.parametrize("H,W", FRAMES)
def test_frame_keeps_val_inds(M, H, W):
    mask = frame_mask(H, W)
    want = O.val_inds(mask)
    assert 0 < want.numel() < H * W
    for given in (mask, mask.cpu(), mask.to(torch.uint8), mask.to(torch.uint8).cpu() * 255):
        f = M.FrameRays(H, W, *intrinsics(H, W), None, NEAR, FAR, IDX, rays_msk=given)
        assert f.val_inds.dtype == torch.int64 and f.val_inds.is_cuda and torch.equal(f.val_inds, want)
        assert f.n_valid == want.numel() and isinstance(f.n_valid, int)
        assert f.resident_bytes() == 8 * want.numel()
    f = frame(H, W, False, masked=False)
    assert f.n_valid == H * W and torch.equal(f.val_inds, torch.arange(H * W, device="cuda"))


@pytest.mark.parametrize("with_c2w", [True, False])
@pytest.mark.parametrize("H,W", FRAMES)
def test_rays_equal_rows_of_the_full_table(H, W, with_c2w):
    table, f = full_rays(H, W, with_c2w), frame(H, W, with_c2w)
    perm = seeded_perm(f.n_valid, seed=W)
    for N_rand in (1, 64, 1000, f.n_valid + 10):
        n = min(N_rand, f.n_valid)
        rays, rgbs, back, sel = f.sample(N_rand, perm=perm)
        assert rgbs is None and back is None
        assert sel.shape == (n,) and sel.dtype == torch.int64 and torch.equal(sel, f.val_inds[perm[:n]])
        assert rays.shape == (n, 9) and rays.dtype == torch.float32 and rays.is_contiguous()
        assert torch.equal(rays, table[sel]), (H, W, with_c2w, N_rand)
        chained, _, _, sel10 = f.sample(N_rand, perm=perm, chain_idx=-0.3)
        assert chained.shape == (n, 10) and torch.equal(sel10, sel)
        assert torch.equal(chained[:, :9], rays) and torch.equal(chained, O.chain_column(table[sel], -0.3))
        assert bool((chained[:, 9] == torch.tensor(-0.3, dtype=torch.float32)).all())
    # the whole reference sequence, from the mask
    want = O.select(table, frame_mask(H, W), None, None, perm, 64)
    got = f.sample(64, perm=perm)
    assert torch.equal(got[0], want[0]) and torch.equal(got[3], want[3])


def test_rays_without_a_mask():
    H, W = FRAMES[0]
    f = frame(H, W, True, masked=False)
    perm = seeded_perm(H * W, seed=3)
    rays, _, _, sel = f.sample(H * W + 1, perm=perm)
    assert torch.equal(sel, perm) and torch.equal(rays, full_rays(H, W, True)[perm])


@pytest.mark.parametrize("H,W", FRAMES)
def test_drawn_permutation(H, W):
    f = frame(H, W, True)
    draw = lambda seed: f.sample(64, generator=torch.Generator(device="cuda").manual_seed(seed))
    rays, _, _, sel = draw(11)
    assert sel.shape == (64,) and sel.unique().numel() == 64
    assert bool(torch.isin(sel, f.val_inds).all())
    assert torch.equal(rays, full_rays(H, W, True)[sel])
    again = draw(11)
    assert torch.equal(again[3], sel) and torch.equal(again[0], rays)
    assert not torch.equal(draw(12)[3], sel)
    everything = f.sample(f.n_valid, generator=torch.Generator(device="cuda").manual_seed(1))[3]
    assert torch.equal(everything.sort().values, f.val_inds)


@pytest.mark.parametrize("H,W", FRAMES)
def test_pixels(H, W):
    rgba, rows, back, colour = pictures(H, W)
    f = frame(H, W, True)
    perm = seeded_perm(f.n_valid, seed=H)
    for N_rand in (1, 64, 1000):
        n = min(N_rand, f.n_valid)
        sel = f.val_inds[perm[:n]]
        # fp32 rows are gathered
        rays, rgbs, bg, got_sel = f.sample(N_rand, image=rows, background=back, perm=perm)
        assert torch.equal(got_sel, sel) and torch.equal(rays, full_rays(H, W, True)[sel])
        assert rgbs.shape == (n, 3) and torch.equal(rgbs, rows[sel]) and torch.equal(bg, back[sel])
        _, rgbs, bg, _ = f.sample(N_rand, image=rows, background=colour, perm=perm)
        assert torch.equal(rgbs, rows[sel]) and torch.equal(bg, colour.expand(n, 3))
        _, rgbs, bg, _ = f.sample(N_rand, image=rows, perm=perm)
        assert torch.equal(rgbs, rows[sel]) and bg is None
        _, rgbs, bg, _ = f.sample(N_rand, background=back, perm=perm)
        assert rgbs is None and torch.equal(bg, back[sel])
        # 8-bit RGB: ToTensor
        rgb8 = rgba[..., :3].contiguous()
        _, rgbs, bg, _ = f.sample(N_rand, image=rgb8, perm=perm)
        assert bg is None and torch.equal(rgbs, (rgb8.view(-1, 3).float() / 255)[sel])
        assert torch.equal(rgbs, O.composite(rgb8, None, H, W)[0][sel])
        # 8-bit RGBA over both background forms: moco_flow_dataset.py:174 in fp32 on the device, then gathered
        for given in (back, colour):
            want_rgbs, want_bg = O.composite(rgba, given, H, W)
            _, rgbs, bg, _ = f.sample(N_rand, image=rgba, background=given, perm=perm)
            assert torch.equal(rgbs, want_rgbs[sel]), (H, W, N_rand, tuple(given.shape))
            assert torch.equal(bg, want_bg[sel])
    with pytest.raises(RuntimeError, match="needs a background"):
        f.sample(8, image=rgba, perm=perm)


def test_whole_reference_sequence_with_rgba():
    """trainer_moco_flow.py:407-417 over datasets/moco_flow_dataset.py:169-176, 194-196 as the oracle restates them, every
    output of one call."""
    H, W = FRAMES[0]
    rgba, _, _, colour = pictures(H, W)
    f = frame(H, W, True)
    perm = seeded_perm(f.n_valid, seed=9)
    rgbs_all, back_all = O.composite(rgba, colour, H, W)
    want = O.select(full_rays(H, W, True), frame_mask(H, W), rgbs_all, back_all, perm, 100)
    got = f.sample(100, image=rgba, background=colour, perm=perm, chain_idx=0.5)
    assert torch.equal(got[0], O.chain_column(want[0], 0.5))
    for a, b in zip(got[1:], want[1:]):
        assert torch.equal(a, b)


def test_empty_batches(M):
    H, W = FRAMES[0]
    rgba, rows, back, colour = pictures(H, W)
    none_valid = M.FrameRays(H, W, *intrinsics(H, W), golden_c2w(), NEAR, FAR, IDX, rays_msk=torch.zeros(H * W, dtype=torch.bool))
    assert none_valid.n_valid == 0 and none_valid.val_inds.shape == (0,) and none_valid.val_inds.dtype == torch.int64
    for f, N_rand in ((none_valid, 64), (frame(H, W, True), 0)):
        rays, rgbs, bg, sel = f.sample(N_rand, image=rgba, background=back)
        assert rays.shape == (0, 9) and rgbs.shape == (0, 3) and bg.shape == (0, 3) and sel.shape == (0,)
        assert rays.dtype == rgbs.dtype == bg.dtype == torch.float32 and sel.dtype == torch.int64 and rays.is_cuda
        rays, rgbs, bg, sel = f.sample(N_rand, chain_idx=0.25)
        assert rays.shape == (0, 10) and rgbs is None and bg is None and sel.shape == (0,)
    empty = M.FrameRays(0, 7, 10.0, (1.0, 1.0), None, NEAR, FAR, IDX)
    assert empty.n_valid == 0 and empty.sample(5)[0].shape == (0, 9)
    torch.cuda.synchronize()


def test_out_of_range_perm_gives_nan_rows():
    H, W = FRAMES[0]
    rgba, rows, back, colour = pictures(H, W)
    f = frame(H, W, True)
    perm = seeded_perm(f.n_valid, seed=4)[:9].clone()
    perm[2], perm[5], perm[7] = f.n_valid, -1, 1 << 40
    bad = torch.tensor([2, 5, 7], device="cuda")
    good = torch.tensor([0, 1, 3, 4, 6, 8], device="cuda")
    for image, background in ((rows, back), (rgba, colour)):
        rays, rgbs, bg, sel = f.sample(9, image=image, background=background, perm=perm, chain_idx=0.5)
        torch.cuda.synchronize()                                   # no fault
        assert bool(torch.isnan(rays[bad]).all()) and bool(torch.isnan(rgbs[bad]).all()) and bool(torch.isnan(bg[bad]).all())
        assert sel[bad].tolist() == [-1, -1, -1]
        want_sel = f.val_inds[perm[good]]
        assert torch.equal(sel[good], want_sel)
        assert torch.equal(rays[good], O.chain_column(full_rays(H, W, True)[want_sel], 0.5))
        want_rgbs, want_bg = (rows, back) if image is rows else O.composite(rgba, colour, H, W)
        assert torch.equal(rgbs[good], want_rgbs[want_sel]) and torch.equal(bg[good], want_bg[want_sel])


def test_sample_refuses_before_launching():
    H, W = FRAMES[0]
    rgba, rows, back, colour = pictures(H, W)
    f = frame(H, W, True)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        f.sample(8, image=rows.cpu())
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        f.sample(8, background=colour.cpu())
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        f.sample(8, perm=torch.arange(8))
    with pytest.raises(RuntimeError, match="image"):
        f.sample(8, image=rows[:-1])
    with pytest.raises(RuntimeError, match="perm"):
        f.sample(8, perm=torch.arange(8, device="cuda", dtype=torch.int32))
    with pytest.raises(RuntimeError, match="7 entries"):
        f.sample(8, perm=torch.arange(7, device="cuda"))


def test_batch_feeds_render_rays(M):
    """The tensors are accepted as they come (contiguous, fp32): canonical NeRF, 64 rays x 16 samples."""
    H, W = FRAMES[0]
    rgba, _, back, _ = pictures(H, W)
    f = frame(H, W, True)
    perm = seeded_perm(f.n_valid, seed=2)
    rays, rgbs, bg, sel = f.sample(64, image=rgba, background=back, perm=perm)
    eager_rays, eager_bg = full_rays(H, W, True)[sel], back[sel]
    embs, nerfs, kw = build_case(M, dict(RENDER_CASES["r_nerf_dir_dense"], S=16), 5, device="cuda")
    with torch.no_grad():
        got = M.render_rays(rays, bg, embs, nerfs, **kw)
        want = M.render_rays(eager_rays, eager_bg, embs, nerfs, **kw)
    assert set(got) == set(want) and got["rgb_coarse"].shape == (64, 3)
    for k in want:
        assert torch.equal(got[k], want[k]), k
