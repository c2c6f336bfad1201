"""moco_flow_amd.metrics on the device (mf_metrics.hip) against the CPU restatement (tests/metrics_oracle.py).

The SSIM map's bar is measured per case, not fixed: the reference arithmetic in fp32 is itself noisy in flat regions through
the cancellation in sigma = f(a^2) - mu^2 (2e-4 .. 9e-4 max-abs from its own float64 evaluation on these inputs), so with
e_ref = max |oracle_fp32 - oracle_fp64| the kernel must sit within 2 e_ref of the float64 oracle -- the factor 2 because a
separable, differently ordered sum is a different rounding of the same cancellation.  The mean: the same with its own e_ref,
floored at 1e-6.  Each case prints both pairs."""
import functools

import pytest
import torch

import metrics_oracle as O

pytestmark = pytest.mark.gpu

TILE_H, TILE_W = 16, 32          # mf_metrics.hip: kSsimTileH, kSsimTileW
SQERR_SHARE = 256 * 8            # mf_metrics.hip: elements of one sqerr workgroup before the grid stops growing

SQERR_MAX_BLOCKS = 1024          # mf_metrics.hip: kSqerrMaxBlocks
FINISH_THREADS = 256             # mf_metrics.hip: kFinishThreads -- the finishing workgroup takes ceil(partial rows / 256) trips

# (1, 3, 160, 320): 10 x 10 x 3 = 300 workgroups, so the finish takes two trips; every other shape finishes in one
MAP_SHAPES = [(1, 3, 37, 53), (2, 3, 6, 7), (1, 3, TILE_H + 1, 2 * TILE_W + 1), (1, 1, TILE_H, TILE_W), (1, 3, 11, 300), (1, 3, 160, 320)]
MAP_CASES = [(s, ws) for s in MAP_SHAPES for ws in (3, 7, 11) if ws // 2 < min(s[2], s[3])]


@pytest.fixture(scope="module")
def M():
    import moco_flow_amd
    return moco_flow_amd.metrics


@functools.lru_cache(maxsize=None)
def reference(shape, ws):
    """(pred, gt, fp64 map, e_ref of the map, fp64 mean, e_ref of the mean), computed once per case on the CPU."""
    pred, gt = O.frame_pair(shape, seed=1000 + shape[2] * 7 + shape[3])
    m64 = O.ssim_map(pred.double(), gt.double(), ws)
    m32 = O.ssim_map(pred, gt, ws)
    e_map = (m32.double() - m64).abs().max().item()
    e_mean = abs(m32.mean().item() - m64.mean().item())
    return pred, gt, m64, e_map, m64.mean().item(), max(e_mean, 1e-6)


def ssim_raw(M, a, b, ws, want_map=True):
    """(map, sums) of one mf_ssim call on (B, C, H, W) tensors of any strides."""
    out, sums = M._ssim_launch(a, a.stride(), b, b.stride(), tuple(a.shape), ws, 1.0, want_map)
    return out, sums


@pytest.mark.parametrize("shape,ws", MAP_CASES, ids=[f"{'x'.join(map(str, s))}-ws{w}" for s, w in MAP_CASES])
def test_ssim_map_and_mean(M, shape, ws):
    pred, gt, m64, e_map, mean64, e_mean = reference(shape, ws)
    a, b = pred.cuda(), gt.cuda()
    got = M.ssim(a, b, reduction='none', window_size=ws)                    # 1 - 2 map, metrics.py:22
    got_map = ((1 - got.double().cpu()) / 2)
    err_map = (got_map - m64).abs().max().item()
    mean = M.ssim(a, b, window_size=ws)
    assert mean.dim() == 0 and mean.dtype == torch.float32 and mean.is_cuda
    err_mean = abs(mean.item() - mean64)
    print(f"\nssim {shape} ws={ws}: map e_ref {e_map:.3e} err {err_map:.3e} | mean e_ref {e_mean:.3e} err {err_mean:.3e}")
    raw_map, sums = ssim_raw(M, a, b, ws)
    assert (raw_map.double().cpu() - m64).abs().max().item() <= 2 * e_map
    assert err_map <= 2 * e_map + 2.5e-7       # (1 - 2 m) and back: two fp32 roundings of a value in [-1, 1]
    assert err_mean <= 2 * e_mean
    # the same launch's squared error
    sq64 = ((pred.double() - gt.double()) ** 2).sum().item()
    assert abs(sums[1].item() - sq64) <= 1e-6 * sq64


def test_ssim_default_window_is_3(M):
    pred, gt, m64, e_map, mean64, e_mean = reference((1, 3, 37, 53), 3)
    assert abs(M.ssim(pred.cuda(), gt.cuda()).item() - mean64) <= 2 * e_mean


def test_ssim_strides_bitwise(M):
    H, W = 37, 53
    pred, gt = O.frame_pair((1, 3, H, W), seed=5)
    a, b = pred.cuda(), gt.cuda()
    ref_map, ref_sums = ssim_raw(M, a, b, 7)
    # rendered rows: (H W, 3), viewed as (1, 3, H, W) with strides (., 1, 3W, 3)
    rows_a = a[0].permute(1, 2, 0).reshape(H * W, 3).contiguous()
    rows_b = b[0].permute(1, 2, 0).reshape(H * W, 3).contiguous()
    va, vb = rows_a.view(H, W, 3).permute(2, 0, 1)[None], rows_b.view(H, W, 3).permute(2, 0, 1)[None]
    assert va.stride()[1:] == (1, 3 * W, 3) and va.data_ptr() == rows_a.data_ptr()
    m, s = ssim_raw(M, va, vb, 7)
    assert torch.equal(m, ref_map) and torch.equal(s, ref_sums)
    # channels 1..3 of a (B, 4, H, W) tensor; the other image stays contiguous: the two stride sets are independent
    a4 = torch.full((1, 4, H, W), 7.0, device="cuda")
    a4[:, 1:] = a
    assert a4[:, 1:].storage_offset() == H * W                          # B = 1: only the base pointer moves
    m, s = ssim_raw(M, a4[:, 1:], b, 7)
    assert torch.equal(m, ref_map) and torch.equal(s, ref_sums)
    # B = 2: the slice's batch stride is 4 H W, no longer C H W, so the view is not contiguous
    pred2, gt2 = O.frame_pair((2, 3, H, W), seed=6)
    a2, b2 = pred2.cuda(), gt2.cuda()
    ref_map2, ref_sums2 = ssim_raw(M, a2, b2, 7)
    a24 = torch.full((2, 4, H, W), 7.0, device="cuda")
    a24[:, 1:] = a2
    v2 = a24[:, 1:]
    assert not v2.is_contiguous() and v2.stride() == (4 * H * W, H * W, W, 1)
    m, s = ssim_raw(M, v2, b2, 7)
    assert torch.equal(m, ref_map2) and torch.equal(s, ref_sums2)


def test_ssim_constant_images_closed_form(M):
    shape = (2, 3, 2 * TILE_H + 3, 2 * TILE_W + 5)                      # spans tile boundaries in both directions
    for p, q in ((1.0, 1.0), (0.3, 0.8), (1.0, 0.0), (0.0, 0.4)):
        a, b = torch.full(shape, p, device="cuda"), torch.full(shape, q, device="cuda")
        want = (2 * p * q + 1e-4) / (p * p + q * q + 1e-4)
        for ws in (3, 11):
            m, sums = ssim_raw(M, a, b, ws)
            err = (m.double() - want).abs().max().item()
            print(f"\nconstant p={p} q={q} ws={ws}: max err {err:.3e}")
            assert err <= 1e-3
            assert abs(sums[0].item() / a.numel() - want) <= 1e-3


def test_ssim_empty_and_detached(M):
    z = torch.zeros((0, 3, 8, 8), device="cuda")
    _, sums = ssim_raw(M, z, z, 3, want_map=False)
    assert sums.tolist() == [0.0, 0.0]
    pred, gt = O.frame_pair((1, 3, 9, 9), seed=2)
    a = pred.cuda().requires_grad_(True)
    out = M.ssim(a, gt.cuda())
    assert not out.requires_grad


@functools.lru_cache(maxsize=None)
def flat_pair(n):
    gen = torch.Generator().manual_seed(n % 9973)
    return torch.rand(n, generator=gen), torch.rand(n, generator=gen)


SQERR_SIZES = [1, 63, 64, 65, SQERR_SHARE - 1, SQERR_SHARE, SQERR_SHARE + 1, 540 * 540 * 3]


@pytest.mark.parametrize("n", SQERR_SIZES)
def test_mse_psnr_unmasked_and_elementwise_mask(M, n):
    a, b = flat_pair(n)
    ga, gb = a.cuda(), b.cuda()
    sq = (a.double() - b.double()) ** 2
    out = M._sqerr(ga, gb, None, "mse")
    print(f"\nsqerr n={n}: sum {out[0].item():.9e} oracle {sq.sum().item():.9e} count {out[1].item():.0f}")
    assert abs(out[0].item() - sq.sum().item()) <= 1e-6 * sq.sum().item()
    assert out[1].item() == n
    got = M.mse(ga, gb)
    assert got.dim() == 0 and got.dtype == torch.float32 and got.is_cuda
    assert got.item() == pytest.approx(sq.mean().item(), rel=1e-6)
    assert M.psnr(ga, gb).item() == pytest.approx(-10 * torch.log10(sq.mean()).item(), rel=1e-6, abs=1e-5)
    mask = torch.rand(n, generator=torch.Generator().manual_seed(n + 1)) < 0.4
    mask[0] = True
    out = M._sqerr(ga, gb, mask.cuda(), "mse")
    assert out[1].item() == int(mask.sum())
    assert abs(out[0].item() - sq[mask].sum().item()) <= 1e-6 * sq[mask].sum().item()
    assert M.mse(ga, gb, mask.cuda()).item() == pytest.approx(O.mse(a.double(), b.double(), mask).item(), rel=1e-6)


# ---- exact sums: inputs that are multiples of 1/16 in [0, 1].  Every fp32 difference is a multiple of 1/16, every square a multiple
# of 2^-8 below 1, and a sum of up to 2^22 of them has at most 30 significant bits: exact in float64 WHATEVER the order of the
# additions, so `==` holds for any correct reduction and a lost, doubled or misplaced partial row shows as a wrong integer.

def sixteenths(shape, seed):
    return torch.randint(0, 17, shape, generator=torch.Generator().manual_seed(seed)).float() / 16


def exact_sqerr(a, b, mask=None):
    d = (a * 16).long() - (b * 16).long()
    sq = d * d
    return int((sq if mask is None else sq[mask]).sum()) / 256


def test_sqerr_exact_block_cap_binds_finish_takes_four_trips(M):
    n = SQERR_MAX_BLOCKS * SQERR_SHARE + 1                               # one element more than 1024 workgroups' first trip
    assert -(-n // SQERR_SHARE) > SQERR_MAX_BLOCKS and SQERR_MAX_BLOCKS // FINISH_THREADS == 4
    a, b = sixteenths((n,), 31), sixteenths((n,), 32)
    ga, gb = a.cuda(), b.cuda()
    out = M._sqerr(ga, gb, None, "mse").cpu()
    print(f"\nsqerr n={n}: sum {out[0].item()!r} exact {exact_sqerr(a, b)!r} count {out[1].item()!r}")
    assert out[0].item() == exact_sqerr(a, b)
    assert out[1].item() == n
    mask = torch.rand(n, generator=torch.Generator().manual_seed(33)) < 0.4
    out = M._sqerr(ga, gb, mask.cuda(), "mse").cpu()
    print(f"masked: sum {out[0].item()!r} exact {exact_sqerr(a, b, mask)!r} count {out[1].item()!r} of {int(mask.sum())}")
    assert out[0].item() == exact_sqerr(a, b, mask)
    assert out[1].item() == int(mask.sum())


def test_ssim_squared_error_exact_finish_takes_two_trips(M):
    shape = (1, 3, 160, 320)
    wgs = shape[1] * -(-shape[2] // TILE_H) * -(-shape[3] // TILE_W)
    assert wgs == 300 and FINISH_THREADS < wgs <= 2 * FINISH_THREADS
    a, b = sixteenths(shape, 41), sixteenths(shape, 42)
    _, sums = ssim_raw(M, a.cuda(), b.cuda(), 3, want_map=False)
    print(f"\nssim {shape}: squared error {sums[1].item()!r} exact {exact_sqerr(a, b)!r}")
    assert sums[1].item() == exact_sqerr(a, b)


@pytest.mark.parametrize("N", [1, 21, 683, 540 * 540])
def test_mse_psnr_row_mask(M, N):
    a, b = flat_pair(3 * N)
    a, b = a.view(N, 3), b.view(N, 3)
    mask = torch.rand(N, generator=torch.Generator().manual_seed(N)) < 0.5
    mask[N // 2] = True
    ga, gb, gm = a.cuda(), b.cuda(), mask.cuda()
    sq = ((a.double() - b.double()) ** 2)[mask]
    out = M._sqerr(ga, gb, gm, "mse")
    assert out[1].item() == 3 * int(mask.sum())
    assert abs(out[0].item() - sq.sum().item()) <= 1e-6 * sq.sum().item()
    assert M.psnr(ga, gb, gm).item() == pytest.approx(O.psnr(a.double(), b.double(), mask).item(), rel=1e-6, abs=1e-5)
    # any other reduction: the elementwise values, masked as value[valid_mask]
    el = M.mse(ga, gb, gm, reduction='none')
    assert el.shape == (int(mask.sum()), 3)
    assert torch.equal(el.cpu(), ((a - b) ** 2)[mask])
    assert torch.equal(M.mse(ga, gb, reduction='none').cpu(), (a - b) ** 2)


def test_mse_mask_selecting_nothing_is_nan(M):
    a, b = flat_pair(65)
    none = torch.zeros(65, dtype=torch.bool, device="cuda")
    out = M._sqerr(a.cuda(), b.cuda(), none, "mse")
    assert out.tolist() == [0.0, 0.0]
    assert torch.isnan(M.mse(a.cuda(), b.cuda(), none))
    assert torch.isnan(M.psnr(a.cuda(), b.cuda(), none))
    e = torch.zeros(0, device="cuda")
    assert torch.isnan(M.mse(e, e))


def test_image_metrics_equals_separate_calls(M):
    H, W = 37, 53
    pred, gt = O.frame_pair((1, 3, H, W), seed=8)
    rows_p = pred[0].permute(1, 2, 0).reshape(H * W, 3).contiguous().cuda()
    rows_g = gt[0].permute(1, 2, 0).reshape(H * W, 3).contiguous().cuda()
    got = M.image_metrics(rows_p, rows_g, H, W)
    assert set(got) == {"mse", "psnr", "ssim"}
    for v in got.values():
        assert v.dim() == 0 and v.dtype == torch.float32 and v.is_cuda
    vp, vg = rows_p.view(H, W, 3).permute(2, 0, 1)[None], rows_g.view(H, W, 3).permute(2, 0, 1)[None]
    assert got["ssim"].item() == M.ssim(vp, vg).item()
    assert got["mse"].item() == pytest.approx(M.mse(rows_p, rows_g).item(), rel=1e-6)
    assert got["psnr"].item() == pytest.approx(M.psnr(rows_p, rows_g).item(), rel=1e-6)
    # the launch behind it is the strided call's, bit for bit
    _, s_rows = M._ssim_launch(rows_p, (0, 1, 3 * W, 3), rows_g, (0, 1, 3 * W, 3), (1, 3, H, W), 3, 1.0, False)
    _, s_view = ssim_raw(M, vp, vg, 3, want_map=False)
    assert torch.equal(s_rows, s_view)
    assert got["ssim"].item() == (s_view[0] / (3 * H * W)).float().item()
    assert got["mse"].item() == (s_view[1] / (3 * H * W)).float().item()
    got7 = M.image_metrics(rows_p, rows_g, H, W, window_size=7)
    assert got7["ssim"].item() == M.ssim(vp, vg, window_size=7).item()


def test_determinism(M):
    pred, gt = O.frame_pair((2, 3, 45, 70), seed=11)
    a, b = pred.cuda(), gt.cuda()
    m1, s1 = ssim_raw(M, a, b, 5)
    m2, s2 = ssim_raw(M, a, b, 5)
    assert torch.equal(m1, m2) and torch.equal(s1, s2)
    fa, fb = flat_pair(540 * 540 * 3)
    fa, fb = fa.cuda(), fb.cuda()
    assert torch.equal(M._sqerr(fa, fb, None, "mse"), M._sqerr(fa, fb, None, "mse"))


def test_side_stream(M):
    pred, gt = O.frame_pair((1, 3, 37, 53), seed=12)
    a, b = pred.cuda(), gt.cuda()
    m0, s0 = ssim_raw(M, a, b, 3)
    e0 = M.mse(a, b)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        m1, s1 = ssim_raw(M, a, b, 3)
        e1 = M.mse(a, b)
    s.synchronize()
    assert torch.equal(m0, m1) and torch.equal(s0, s1) and torch.equal(e0, e1)


def test_refusals(M):
    a = torch.rand(1, 3, 5, 5)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        M.ssim(a, a)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        M.mse(a, a)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        M.image_metrics(a.view(-1, 3), a.view(-1, 3), 5, 5)
    g = a.cuda()
    with pytest.raises(RuntimeError, match="shapes differ"):
        M.ssim(g, g[:, :, :4])
    with pytest.raises(RuntimeError, match="shapes differ"):
        M.psnr(g, g[:, :2])
    with pytest.raises(RuntimeError, match="window_size"):
        M.ssim(g, g, window_size=11)                                     # reflects by 5 on a 5 x 5 image
    with pytest.raises(RuntimeError, match="window_size"):
        M.ssim(g, g, window_size=4)
    with pytest.raises(RuntimeError, match="valid_mask"):
        M.mse(g, g, torch.ones(2, dtype=torch.bool, device="cuda"))
    with pytest.raises(RuntimeError, match="rows must be"):
        M.image_metrics(g.view(-1, 3), g.view(-1, 3), 6, 5)
