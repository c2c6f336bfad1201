"""The fused render passes at the launch shapes the fixture-sized tests never reach (-m gpu).

Each launcher (mf_render.hip: f32; mf_render_bf16.hip: bf16x3 and the fast bf16 mode) picks G rays per group -- the smallest G
whose G S samples fill whole tiles, else the best-filling G <= 64, then up to 8 times that while the per-CU makespan does not
grow -- and launches min(n_groups, #CUs) persistent workgroups.  At the BASELINE shapes every workgroup owns ONE group, every S
fills tiles exactly and every MoCo ray carries the same image index.  Here:

  * n_rays > 64 #CUs (G <= 64 in both launchers): every workgroup runs its persistent loop at least twice, over an uneven share
    of groups, the bf16 kernels' cross-group prefetch of the next group's NoF bias rows (double buffer by `seq & 1`) included;
  * odd S (37, 129, 100, 255, 257: no G <= 64 fills a 128- or 256-sample tile, the "no exact fit" branch), S = 256, the largest
    S of each (precision, network) (G = 1) and, for the bf16 MoCo passes, the smallest (a tile spans up to 34 rays' bias rows);
  * per-ray varied image indices (helpers.varied_indices), so that a kernel staging another ray's bias row, or reading another
    ray's NeRF(ind) input, renders different numbers.

The kernel renders the whole batch; the oracle a subset of its rays (helpers.subset_rays: first, last, a seeded draw between) --
per-ray outputs do not depend on the batch around them (tests/test_oracle_golden.py).  The batch-wide consensus vectors
nof_*_disp_* (alpha >= 0.01 mask, all-true if none) are compared only where the oracle sees the whole batch.  Bars are the
existing ones: 1e-4 max-rel for f32 and bf16x3 (test_c3_full_size_*), the oracle-of-its-arithmetic bars of
tests/test_gpu_bf16_oracle.py for the fast mode, helpers._check_grads_vs_float64 for the fp32 training step's gradients."""
import pytest
import torch

from cases import RENDER_CASES
from helpers import TOL, _check_grads_vs_float64, build_case, relerr, subset_rays, varied_indices

pytestmark = pytest.mark.gpu

NETS = {"nerf": "r_nerf_dir_dense", "moco": "r_moco_global"}     # C2's NeRF(dir); C3's MoCo (local + global chains, NeRF(ind), quat NoFs)
PRECISIONS = ["f32", "bf16x3", "bf16"]

# The envelope of the fused passes, pinned: the largest S each (precision, network) renders -- one group of one ray fills the
# 160 KiB of LDS -- and, for the bf16 MoCo passes, the smallest (two buffers of per-ray NoF bias rows for every ray a tile
# touches: (tile - 1) / S + 2 of them).  Found by render_rays on one ray over S = 1 .. 16384; a silently moved envelope fails here.
S_MAX = {("nerf", "f32"): 1356, ("nerf", "bf16x3"): 2585, ("nerf", "bf16"): 4428,
         ("moco", "f32"): 640, ("moco", "bf16x3"): 1664, ("moco", "bf16"): 2278}
S_MIN = {("nerf", "f32"): 1, ("nerf", "bf16x3"): 1, ("nerf", "bf16"): 1,
         ("moco", "f32"): 1, ("moco", "bf16x3"): 8, ("moco", "bf16"): 12}
MSG_TOO_LONG = "n_samples={S} exceeds the {m} samples a workgroup can stage"
MSG_TOO_SHORT = "n_samples={S} leaves no room for the per-ray NoF bias rows of a tile"

# oracle subsets: about 256 rays for the fp32 oracle, 64 for the bf16 one, fewer where S is large (samples per oracle call)
SUBSET = {"cpu_ref": (256, 65536), "bf16_ref": (64, 16384)}


def _shapes(net, prec):
    """((a, b), S, full) of one (network, precision): n_rays = a #CUs + b.  full: the oracle renders the whole batch (n <= 1024),
    so the batch-wide consensus vectors are compared too."""
    out = [((128, 37), 64, False),        # > 64 #CUs: >= 2 groups per workgroup whatever the device, uneven shares
           ((64, 129), 37, False),        # odd S: the no-exact-fit branch (G ~ 38 in f32, ~ 62 in fast bf16: some workgroups own two groups)
           ((64, 3), 129, False),
           ((0, 5003), 100, False), ((0, 4001), 255, False), ((0, 2049), 257, False),
           ((0, 2000), 256, False),       # the shipped configs' 128 + 128
           ((0, 1), 40, True), ((0, 3), 40, True),    # one partial group of a large-G S
           ((2, 1), S_MAX[net, prec], False)]          # G = 1: the largest S, two groups per workgroup
    if net == "moco":     # short rays: a fast tile spans 17 rays' bias rows at S = 16, and the smallest S (S = 1 is degenerate in the
        # reference itself: test_composite_backward_unit) -- 23 rows at S = 12 in the fast mode, 17 at S = 8 in bf16x3
        out += [((0, 777), 16, True), ((0, 777), max(2, S_MIN[net, prec]), True)]
    return out


CASES = [(net, prec, n, S, full) for net in NETS for prec in PRECISIONS for n, S, full in _shapes(net, prec)]
IDS = [f"{net}-{prec}-n{f'{a}cus+' if a else ''}{b}-S{S}" for net, prec, (a, b), S, full in CASES]
# The smallest-S MoCo passes of f32 (S = 2) and bf16x3 (S = 8) are held to the bit-exact invariants and the envelope test, not to the
# 1e-4 bar: there the intervals are a third of the ray or more and one sample carries the ray -- the fp32 oracle itself sits
# 1.0e-4 .. 1.6e-4 (max-rel, depth / opacity) from the same oracle with float64 accumulation, so that bar would measure the
# reference arithmetic.  S = 16 carries their many-rows-per-tile case to the oracle.  The fast mode's bars are relative (to a
# 1e-3 .. 1e-2 distance): its smallest S, 12, is compared.
ORACLE = [(case, i) for case, i in zip(CASES, IDS) if not (case[0] == "moco" and case[3] < 16 and case[1] != "bf16")]


@pytest.fixture(scope="module")
def M():
    import moco_flow_amd
    assert torch.cuda.is_available()
    moco_flow_amd._lib.lib()          # fail loudly if the HIP library is missing
    return moco_flow_amd


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _case(net, S, Mi=0):
    c = dict(RENDER_CASES[NETS[net]])
    c["S"], c["M"] = S, Mi
    return c


def _inputs(net, n):
    from moco_flow_amd import synth
    rays, bg = synth.rays(0, n, chained=(net == "moco"))
    rays = torch.from_numpy(rays)
    return (varied_indices(rays, seed=n) if net == "moco" else rays), torch.from_numpy(bg)


def _render(M, c, rays, bg, precision):
    """The HIP pass over rays (cuda tensors, any row stride) in `precision`, gradient-free."""
    from moco_flow_amd import rendering
    embs, nerfs, kw = build_case(M, c, 0, device="cuda")
    strict = rendering.STRICT_RNG
    try:
        rendering.STRICT_RNG = False
        rendering.set_precision(precision)
        with torch.no_grad():
            return M.render_rays(rays, bg, embs, nerfs, **kw)
    finally:
        rendering.set_precision("f32")
        rendering.STRICT_RNG = strict


_ORACLE = {}     # (net, n, S, arith) -> (idx, result): the fp32 oracle's subset is shared by the f32 and bf16x3 cases


def _oracle(net, c, rays, bg, idx, arith, shift=0.0):
    """The oracle of rays[idx]; shift: added to the sigma of every ray's last sample (the noise hook), before its activation."""
    from oracle import bf16_ref as B
    from oracle import cpu_ref as R
    key = (net, rays.shape[0], c["S"], arith, shift, tuple(idx.tolist()))
    if key not in _ORACLE:
        embs, nerfs, kw = build_case(R if arith == "cpu_ref" else B.Backend(B.BF16), c, 0)
        noise = torch.zeros(len(idx), c["S"])
        noise[:, -1] = shift
        with torch.no_grad():
            _ORACLE[key] = R.render_rays(rays[idx], bg[idx], embs, nerfs, _rng={"noise_coarse": noise}, **kw)
    return _ORACLE[key]


def _subset(n, S, full, arith):
    k, budget = SUBSET[arith]
    return torch.arange(n) if full else subset_rays(n, max(16, min(k, budget // S)), seed=S)


def _check_consensus(got, want, k, bf16):
    """nof_*_disp_* of a whole batch: the rules of test_gpu_parity._check_result (f32, bf16x3) and of
    test_c3_full_size_bf16_vs_oracle (bf16: its mean to 2 %, its length to 2 %)."""
    got = got.cpu().double()          # (a lazy.MaskedVector materialises here)
    want = want.double()
    n_g, n_w = got.shape[0], want.shape[0]
    if bf16:
        assert abs(n_g - n_w) <= max(2, 0.02 * n_w), (k, n_g, n_w)
        assert abs(float(got.mean()) - float(want.mean())) <= 2e-2 * abs(float(want.mean())), k
        return
    assert abs(n_g - n_w) <= max(2, int(0.002 * n_w)), (k, n_g, n_w)
    if n_g == n_w:
        assert relerr(got, want) <= TOL, (k, relerr(got, want))
    else:
        assert abs(float(got.mean()) - float(want.mean())) <= 1e-3 * abs(float(want.mean())), k


@pytest.mark.parametrize("net,prec,n_of,S,full", [c for c, _ in ORACLE], ids=[i for _, i in ORACLE])
def test_pass_vs_oracle_on_a_ray_subset(M, cus, net, prec, n_of, S, full):
    """One launch over all n rays; per-ray outputs at the oracle's subset against cpu_ref (f32, bf16x3: 1e-4 max-rel) or
    bf16_ref (fast bf16: >= 20 dB closer than to cpu_ref, l2-rel <= a tenth of the fp32-oracle distance)."""
    from oracle import bf16_ref as B
    n = n_of[0] * cus + n_of[1]
    if n_of[0] >= 128:
        assert n > 64 * cus and n % 2 == 1
    c = _case(net, S)
    rays, bg = _inputs(net, n)
    got = _render(M, c, rays.cuda(), bg.cuda(), prec)
    keys = ["rgb_coarse", "depth_coarse", "opacity_coarse"]
    for k in keys:
        assert got[k].shape[0] == n and bool(torch.isfinite(got[k]).all()), k
    idx = _subset(n, S, full, "cpu_ref")
    want = _oracle(net, c, rays, bg, idx, "cpu_ref")
    if prec != "bf16":
        errs = {k: relerr(got[k].cpu()[idx], want[k]) for k in keys}
        print(f"{net} {prec} n={n} S={S}: {len(idx)} rays vs cpu_ref, max-rel " + " / ".join(f"{e:.1e}" for e in errs.values()))
        for k, e in errs.items():
            assert e <= TOL, (k, e)
        if full:
            for k in want:
                if k.startswith("nof_"):
                    _check_consensus(got[k], want[k], k, False)
        return
    # fast bf16: a subset of the fp32 oracle's subset (its rows reused), against the oracle of its own arithmetic
    pos = _subset(len(idx), S, full, "bf16_ref")
    idx_b = idx[pos]
    own = _oracle(net, c, rays, bg, idx_b, "bf16_ref")
    # The far-plane hazard: the last sample's interval is 1e10 (rendering.py:158-160), so its alpha is 1 for any sigma > 0 and 0
    # for sigma <= 0.  A ray whose last sigma lies within the bf16 arithmetic's error of zero renders the rest of its transmittance
    # there in one evaluation and not in the other.  Measured: ray 683 of the 777-ray MoCo batch (S = 12, 13, 20: the same far
    # point), last alpha 1 in the kernel, 0 in its oracle, every other sample alike; the f32 and bf16x3 kernels agree with the
    # oracle there.  Rays whose oracle changes its last alpha when that sigma moves by 0.1 leave the bars; at most 5 % of them.
    stable = torch.ones(len(idx_b), dtype=torch.bool)
    if net == "moco":
        for shift in (-0.1, 0.1):
            near = _oracle(net, c, rays, bg, idx_b, "bf16_ref", shift)
            for k in keys:
                d = (near[k] - own[k]).abs()
                stable &= (d.amax(1) if d.dim() == 2 else d) <= 1e-2
    n_unstable = int((~stable).sum())
    assert n_unstable <= max(1, len(idx_b) // 20), n_unstable
    sel = idx_b[stable]
    own = {k: own[k][stable] for k in keys}
    f32 = {k: want[k][pos][stable] for k in keys}
    ps_own, ps_f32 = B.psnr_equiv(got["rgb_coarse"].cpu()[sel], own["rgb_coarse"]), B.psnr_equiv(got["rgb_coarse"].cpu()[sel], f32["rgb_coarse"])
    l2_own = [B.l2rel(got[k].cpu()[sel], own[k]) for k in keys]
    l2_f32 = [B.l2rel(got[k].cpu()[sel], f32[k]) for k in keys]
    print(f"{net} bf16 n={n} S={S}: {len(sel)} rays ({n_unstable} at the far-plane hazard left out), PSNR-equiv to its own oracle {ps_own:.1f} dB "
          f"(fp32 oracle {ps_f32:.1f}); l2-rel " + " / ".join(f"{x:.1e}" for x in l2_own) + " (fp32 oracle "
          + " / ".join(f"{x:.1e}" for x in l2_f32) + ")")
    assert ps_own >= ps_f32 + 20.0 and ps_own >= 55.0, (ps_own, ps_f32)
    for a, b in zip(l2_own, l2_f32):
        assert a <= max(0.1 * b, 1e-5), (l2_own, l2_f32)
    if full:
        whole = _oracle(net, c, rays, bg, idx_b, "bf16_ref")
        for k in whole:
            if k.startswith("nof_"):
                _check_consensus(got[k], whole[k], k, True)


def _split_points(n):
    """Two cuts of 0..n into three uneven non-empty parts."""
    a = max(1, n // 7)
    return a, min(n - 1, a + max(1, (2 * n) // 5))


@pytest.mark.parametrize("net,prec,n_of,S,full", CASES, ids=IDS)
def test_launch_invariants_bit_exact(M, cus, net, prec, n_of, S, full):
    """Over the whole batch, bit for bit: one launch = the concatenation of three launches over an uneven split (what
    tools/ragged_sweep.py checks by hand); a row-strided rays view = its contiguous copy (the pointer and stride(0) go to the
    kernels as they are), for a (N, 12) buffer's leading columns and for rays[::2]."""
    n = n_of[0] * cus + n_of[1]
    c = _case(net, S)
    rays, bg = _inputs(net, n)
    rays, bg = rays.cuda(), bg.cuda()
    keys = ["rgb_coarse", "depth_coarse", "opacity_coarse"]
    ref = _render(M, c, rays, bg, prec)

    def same(out, what):
        for k in keys:
            assert torch.equal(out[k], ref[k]), (what, k, int((out[k] != ref[k]).sum()))

    if n >= 3:
        a, b = _split_points(n)
        parts = [_render(M, c, rays[lo:hi], bg[lo:hi], prec) for lo, hi in ((0, a), (a, b), (b, n))]
        same({k: torch.cat([p[k] for p in parts]) for k in keys}, f"split {a} / {b - a} / {n - b}")
    wide = torch.full((n, 12), float("nan"), device="cuda")
    wide[:, :rays.shape[1]] = rays
    view = wide[:, :rays.shape[1]]
    assert view.stride(0) == 12
    same(_render(M, c, view, bg, prec), "(N, 12) buffer")
    twice = torch.full((2 * n, rays.shape[1]), float("nan"), device="cuda")
    twice[::2] = rays
    assert twice[::2].stride(0) == 2 * rays.shape[1]
    same(_render(M, c, twice[::2], bg, prec), "rays[::2]")


@pytest.mark.parametrize("net", sorted(NETS))
@pytest.mark.parametrize("prec", PRECISIONS)
def test_sample_count_envelope_is_pinned(M, net, prec):
    """The largest S renders, one more is refused on the host with the envelope in the message; for the bf16 MoCo passes the
    smallest S renders and one less is refused as too short for the per-ray bias rows.  (A pass at the limits is compared
    with the oracle by the tests above; here the limits themselves.)"""
    from moco_flow_amd import synth
    s_max, s_min = S_MAX[net, prec], S_MIN[net, prec]
    rays, bg = synth.rays(0, 1, chained=(net == "moco"))
    rays, bg = torch.from_numpy(rays).cuda(), torch.from_numpy(bg).cuda()
    for S in (s_min, s_max):
        out = _render(M, _case(net, S), rays, bg, prec)
        assert bool(torch.isfinite(out["rgb_coarse"]).all()), S
    with pytest.raises(NotImplementedError, match=MSG_TOO_LONG.format(S=s_max + 1, m=s_max)):
        _render(M, _case(net, s_max + 1), rays, bg, prec)
    if s_min > 1:
        with pytest.raises(NotImplementedError, match=MSG_TOO_SHORT.format(S=s_min - 1)):
            _render(M, _case(net, s_min - 1), rays, bg, prec)


TRAIN = [(37, 50), (100, 155)]


def _train(M, c, rays, bg, idx, gt, fwd):
    """HIP training step: forward over `rays`, loss MSE(rgb_coarse[idx], gt) + MSE(rgb_fine[idx], gt), backward.  -> (result,
    the networks (their .grad), captured planes)"""
    from moco_flow_amd import rendering
    embs, nerfs, kw = build_case(M, c, 0, device="cuda")
    nets = list(nerfs) + (list(kw["nof_models"]) if kw["nof_models"] else [])
    cap = {}
    try:
        rendering.set_train_forward_precision(fwd)
        res = M.render_rays(rays.cuda(), bg.cuda(), embs, nerfs, _capture=cap, **kw)
    finally:
        rendering.set_train_forward_precision("f32")
    i, g = idx.cuda(), gt.cuda()
    (((res["rgb_coarse"][i] - g) ** 2).mean() + ((res["rgb_fine"][i] - g) ** 2).mean()).backward()
    return res, nets, cap


@pytest.mark.parametrize("S,Mi", TRAIN, ids=[f"S{s}+{m}" for s, m in TRAIN])
@pytest.mark.parametrize("net", sorted(NETS))
@pytest.mark.parametrize("fwd", ["f32", "bf16x3"])
def test_training_at_odd_shapes(M, cus, fwd, net, S, Mi, wgrad):
    """A training step (coarse S + fine Mi samples, odd totals) over enough rays that the coarse pass owns >= 2 groups per
    workgroup; the loss covers a subset of the rays only (MSE of rgb_*[idx]), so the HIP backward runs over every sample, the
    zero-gradient rays included.  Forward values at the subset against the fp32 oracle (1e-4 max-rel, the fine pass on the HIP
    path's own fine depths); every weight gradient against the same step launched over the subset's rays alone -- the same
    function, so the launch shape may move a gradient by the contractions' summation order only (measured <= 1.5e-6 max-rel);
    with the fp32 training forward, every weight gradient against the float64 oracle of the subset (_check_grads_vs_float64, the
    rule of test_gradients_vs_oracle's MoCo cases).  Not asserted, measured at wgrad f32 (worst max-rel vs the fp32 oracle / its bar):
      * the NeRF's fixed 1e-4 bar against the fp32 oracle (test_gradients_vs_oracle's NeRF route): 1.6e-3 on xyz_encoding_1.weight
        at S 37 + 50, 2.0e-4 at 100 + 155 -- on 128 rays x two NeRFs one ReLU unit flipping between fp32 evaluation orders moves a
        first-layer row by that sample's whole contribution (the helper's 2e-3 floor is there for it);
      * the bf16x3 training forward: 1.3e-2 / 9.3e-3 (NeRF, 37 + 50), 9.1e-3 / 8.9e-3 and 3.6e-3 / 2.0e-3 (MoCo) -- its 1e-5 forward
        moves more ReLU units across than fp32 rounding does (test_train_forward_bf16x3); identical in the subset-only launch."""
    from oracle import cpu_ref as R
    # G S <= the samples a workgroup stages (S_MAX: the same LDS layout with the activation dump) and G <= 64
    n = 2 * cus * min(64, S_MAX[net, fwd] // S) + 37
    c = _case(net, S, Mi)
    rays, bg = _inputs(net, n)
    idx = subset_rays(n, 64 if net == "moco" else 128, seed=S)
    gt = torch.rand(len(idx), 3, generator=torch.Generator().manual_seed(S))
    res, nets, cap = _train(M, c, rays, bg, idx, gt, fwd)
    _, nets1, cap1 = _train(M, c, rays[idx], bg[idx], torch.arange(len(idx)), gt, fwd)
    named = lambda ms: {f"{j}.{k}": p.grad for j, m in enumerate(ms) for k, p in m.named_parameters()}
    grads, alone = named(nets), named(nets1)
    z_fine = cap["z_fine"].cpu()[idx]
    assert torch.equal(z_fine, cap1["z_fine"].cpu())
    embs, nerfs, kw = build_case(R, c, 0)
    with torch.no_grad():
        want = R.render_rays(rays[idx], bg[idx], embs, nerfs, _z_fine_override=z_fine, **kw)
    for k in ("rgb_coarse", "depth_coarse", "opacity_coarse", "rgb_fine", "depth_fine", "opacity_fine"):
        e = relerr(res[k].detach().cpu()[idx], want[k])
        assert e <= TOL, (k, e)
    live = [k for k, g in alone.items() if g is not None and float(g.abs().max()) > 0.0]
    assert len(live) >= 20
    worst = max((relerr(grads[k], alone[k]), k) for k in live)
    print(f"{net} {fwd} forward, wgrad {wgrad}, n={n} S={S}+{Mi}: {len(live)} weight gradients vs the subset-only launch, worst "
          f"max-rel {worst[0]:.1e} ({worst[1]})")
    for k, g in alone.items():
        assert (grads[k] is None) == (g is None), k
    assert worst[0] <= 1e-5, worst
    if fwd == "f32":
        _, g32 = _oracle_grads_subset(c, rays[idx], bg[idx], z_fine, gt, torch.float32)
        _, g64 = _oracle_grads_subset(c, rays[idx], bg[idx], z_fine, gt, torch.float64)
        assert _check_grads_vs_float64(nets, g32, g64, label=f"{net} f32 forward, wgrad {wgrad}, S={S}+{Mi}") >= 20


def _oracle_grads_subset(c, rays, bg, z_fine, gt, dtype):
    """The float64 / fp32 oracle's autograd of the same loss over the subset's rays, the fine pass on the HIP path's fine depths."""
    from oracle import cpu_ref as R
    embs, nerfs, kw = build_case(R, c, 0)
    nets = list(nerfs) + (list(kw["nof_models"]) if kw["nof_models"] else [])
    for m in nets:
        for k in m.p:
            m.p[k] = m.p[k].to(dtype).clone().requires_grad_(True)
    for e in list(embs) + list(kw["nof_embeddings"] or []):
        if e is not None:
            e.freq_bands = e.freq_bands.to(dtype)
    torch.set_default_dtype(dtype)
    try:
        res = R.render_rays(rays.to(dtype), bg.to(dtype), embs, nerfs, _z_fine_override=z_fine.to(dtype), **kw)
        loss = ((res["rgb_coarse"] - gt.to(dtype)) ** 2).mean() + ((res["rgb_fine"] - gt.to(dtype)) ** 2).mean()
    finally:
        torch.set_default_dtype(torch.float32)
    flat = [(i, k) for i, m in enumerate(nets) for k in m.p]
    grads = torch.autograd.grad(loss, [nets[i].p[k] for i, k in flat], allow_unused=True)
    return res, {f"{i}.{k}": g for (i, k), g in zip(flat, grads)}
