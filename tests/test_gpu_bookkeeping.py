"""The small kernels around the hot path, each driven through the C ABI at the shapes and edges where its index bookkeeping
could go wrong, against a CPU reference in float64 or in exact integer arithmetic (run with -m gpu on an MI355X):
mask compaction, the loss partials and their backward seeds, sample_pdf on its OWN cdf (inputs chosen so that nothing is left
to rounding), the 1-nearest-neighbour search on a lattice, the image scatter-back, the NoF's embedded rows and the ray
generator.  Inputs are seeded and generated here; nothing compares a kernel with itself unless its docstring says so."""
import ctypes
import math

import numpy as np
import pytest
import torch

from helpers import pdf_per_wave_floats, relerr

pytestmark = pytest.mark.gpu

THR = np.float32(0.01)                                  # rendering.py:306: the consensus mask is alphas >= 0.01
THR_BELOW = np.nextafter(THR, np.float32(0))


@pytest.fixture(scope="module")
def M():
    import moco_flow_amd
    assert torch.cuda.is_available()
    moco_flow_amd._lib.lib()          # fail loudly if the HIP library is missing
    return moco_flow_amd


@pytest.fixture(scope="module")
def R():
    from oracle import cpu_ref
    return cpu_ref


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stream():
    import moco_flow_amd._lib as L
    return L.current_stream(torch.device("cuda"))


# ------------------------------------------------------------------------------------------------ 1. mf_compact_mask
def _alphas(rng, N, S):
    """Uniform in [0, 0.03) with entries exactly at the threshold (kept: the rule is >=), one float below it (dropped) and
    nan (dropped); rays 3, 10, 17, ... entirely below the threshold (a ray with no masked sample between rays with some),
    ray 1 entirely above."""
    a = (rng.random((N, S)) * 0.03).astype(np.float32)
    flat = a.reshape(-1)
    n = flat.size
    if n:
        idx = rng.permutation(n)
        k, kn = max(1, n // 40), max(1, n // 150)
        flat[idx[:k]] = THR
        flat[idx[k:2 * k]] = THR_BELOW
        flat[idx[2 * k:2 * k + kn]] = np.nan
    a[3::7] = (rng.random(a[3::7].shape) * 0.0099).astype(np.float32)
    if N > 1:
        a[1] = (0.01 + rng.random(S) * 0.02).astype(np.float32)
    return a


COMPACT_SHAPES = [(0, 64), (0, 1), (1, 1), (1, 64), (1, 200), (3, 37), (3, 128), (4, 63), (4, 65), (4, 384), (5, 1), (5, 64), (5, 200),
                  (1023, 1), (1023, 64), (1023, 65), (1024, 37), (1024, 64), (1024, 128), (1024, 200), (1025, 63), (1025, 64),
                  (1025, 65), (2049, 37), (2049, 64), (2049, 200), (2049, 384), (5000, 63), (5000, 64), (5000, 200)]
SENTINEL = -12345.0


def _compact(alphas, va, vb):
    """mf_compact_mask on device tensors (va / vb None: that side's pointers are NULL) -> (out_a, out_b, count).  Outputs
    are N S + 5 sentinels before the call."""
    import moco_flow_amd._lib as L
    N, S = alphas.shape
    oa = None if va is None else torch.full((N * S + 5,), SENTINEL, device="cuda")
    ob = None if vb is None else torch.full((N * S + 5,), SENTINEL, device="cuda")
    count = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    scratch = torch.empty(int(L.lib().mf_compact_scratch_bytes(N)), dtype=torch.uint8, device="cuda")
    L.check(L.lib().mf_compact_mask(L.ptr(alphas), L.ptr(va), L.ptr(vb), N, S, L.ptr(oa), L.ptr(ob), L.ptr(count), L.ptr(scratch),
                                    _stream()), "mf_compact_mask")
    torch.cuda.synchronize()
    return (None if oa is None else oa.cpu()), (None if ob is None else ob.cpu()), int(count.item())


@pytest.mark.parametrize("N,S", COMPACT_SHAPES)
def test_compact_mask_exact_every_shape_class(M, N, S):
    """mf_compact_mask (rendering.py:306-314) against vals[alphas >= 0.01] of torch on the CPU: the count, both outputs bit
    for bit, nothing written past the count, one-sided calls, at every class of N (the scan's 1024-ray blocks and their carry)
    and of S (the ballot loop's tail and running offset)."""
    rng = np.random.default_rng(1000 * N + S)
    a = _alphas(rng, N, S)
    va, vb = rng.standard_normal((N, S)).astype(np.float32), rng.standard_normal((N, S)).astype(np.float32)
    ta, tva, tvb = torch.from_numpy(a), torch.from_numpy(va), torch.from_numpy(vb)
    mask = ta >= 0.01
    assert np.array_equal(mask.numpy(), a >= THR)                    # (torch compares in fp32, like the kernel)
    if N * S >= 1000:                                                # the generator's own edges survived the ray overrides
        assert (a == THR).any() and (a == THR_BELOW).any() and np.isnan(a).any() and mask[2::7].any() and not mask[3::7].any()
    n = int(mask.sum())
    want_a, want_b = (tva[mask], tvb[mask]) if n else (tva.reshape(-1), tvb.reshape(-1))
    want_n = n if n else N * S
    da, dva, dvb = ta.cuda(), tva.cuda(), tvb.cuda()
    oa, ob, count = _compact(da, dva, dvb)
    assert count == want_n
    assert torch.equal(oa[:count], want_a) and torch.equal(ob[:count], want_b)
    assert bool((oa[count:] == SENTINEL).all()) and bool((ob[count:] == SENTINEL).all())
    oa1, none_b, c1 = _compact(da, dva, None)
    none_a, ob1, c2 = _compact(da, None, dvb)
    assert none_a is None and none_b is None and c1 == c2 == want_n
    assert torch.equal(oa1, oa) and torch.equal(ob1, ob)


@pytest.mark.parametrize("N,S", [(37, 64), (1025, 65), (1024, 1), (3, 200), (2049, 63)])
def test_compact_mask_all_false_fallback(M, N, S):
    """No sample reaches the threshold (zeros, nan and values just below it): the mask falls back to all-true
    (rendering.py:307-308) -- every value, in row-major order, count = N S."""
    rng = np.random.default_rng(7 * N + S)
    a = (rng.random((N, S)) * 0.0099).astype(np.float32)
    a.reshape(-1)[::3] = THR_BELOW
    a.reshape(-1)[1::5] = np.nan
    a.reshape(-1)[2::11] = 0.0
    assert not (a >= THR).any()
    va, vb = rng.standard_normal((N, S)).astype(np.float32), rng.standard_normal((N, S)).astype(np.float32)
    oa, ob, count = _compact(_dev(a), _dev(va), _dev(vb))
    assert count == N * S
    assert torch.equal(oa[:count], torch.from_numpy(va).reshape(-1)) and torch.equal(ob[:count], torch.from_numpy(vb).reshape(-1))
    assert bool((oa[count:] == SENTINEL).all()) and bool((ob[count:] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ 2. mf_loss_partials
def _loss_pass(rng, N, S, mask_kind="mixed"):
    """One pass's arrays (numpy fp32): rgb, alphas and two non-negative consensus planes."""
    if mask_kind == "mixed":
        a = _alphas(rng, N, S)
    elif mask_kind == "empty":
        a = (rng.random((N, S)) * 0.0099).astype(np.float32)
        a.reshape(-1)[::3] = THR_BELOW
        a.reshape(-1)[1::7] = np.nan
    else:                                                            # "full"
        a = (0.01 + rng.random((N, S)) * 0.02).astype(np.float32)
        a.reshape(-1)[::3] = THR
    return dict(rgb=rng.random((N, 3)).astype(np.float32), alphas=a, disp_local=rng.random((N, S)).astype(np.float32),
                disp_global=(rng.random((N, S)) * 3).astype(np.float32), S=S)


ALL4 = ("rgb", "alphas", "disp_local", "disp_global")


def _loss_struct(p, keep):
    """mf_loss_pass of a pass dict (its arrays on the device under 'dev'); `keep`: the array names handed over."""
    import moco_flow_amd._lib as L
    s = L.mf_loss_pass()
    for k in ALL4:
        setattr(s, k, L.ptr(p["dev"][k]) if k in keep else None)
    s.n_samples = p["S"]
    return s


def _loss_partials(coarse, fine, target, N, keep_c, keep_f, with_means=True):
    """-> (out12 float64 numpy, means6 fp32 numpy or None, out12 on the device)."""
    import moco_flow_amd._lib as L
    lib = L.lib()
    for p in (coarse, fine):
        if p is not None and "dev" not in p:
            p["dev"] = {k: _dev(p[k]) for k in ALL4}
    sc = _loss_struct(coarse, keep_c)
    sf = _loss_struct(fine, keep_f) if fine is not None else None
    out12 = torch.full((12,), float("nan"), dtype=torch.float64, device="cuda")
    means = torch.full((6,), -3.0, device="cuda") if with_means else None
    scratch = torch.empty(int(lib.mf_loss_partials_scratch_bytes()), dtype=torch.uint8, device="cuda")
    L.check(lib.mf_loss_partials(ctypes.byref(sc), ctypes.byref(sf) if sf is not None else None, L.ptr(target), N, L.ptr(out12),
                                 L.ptr(means), L.ptr(scratch), _stream()), "mf_loss_partials")
    torch.cuda.synchronize()
    return out12.cpu().numpy(), (None if means is None else means.cpu().numpy()), out12


def _loss_reference(passes, keeps, target, N):
    """The header comment of mf_loss_partials in float64: twelve numbers and, per sum, the number of terms it adds.  Sums by
    math.fsum -- the correctly rounded sum of the float64 terms: the reference adds one rounding and no order of its own."""
    want, terms = [0.0] * 12, [0] * 6
    for q, (p, keep) in enumerate(zip(passes, keeps)):
        if p is None:
            continue
        if "rgb" in keep:
            d = p["rgb"].astype(np.float64) - target.astype(np.float64)
            want[2 * q], want[2 * q + 1], terms[q] = math.fsum((d * d).reshape(-1)), float(3 * N), 3 * N
        mask = p["alphas"] >= THR
        cnt = int(mask.sum())
        sel = mask if cnt else np.ones_like(mask)                    # no element set -> all elements (rendering.py:307-308)
        cnt = cnt if cnt else mask.size
        for j, name in ((2, "disp_local"), (4, "disp_global")):
            if name in keep:
                want[2 * j + 2 * q] = math.fsum(p[name].astype(np.float64)[sel])
                want[2 * j + 2 * q + 1], terms[j + q] = float(cnt), cnt
    return want, terms


def _check_loss(got, means, want, terms, tag):
    for k in range(6):
        s, c = got[2 * k], got[2 * k + 1]
        print(f"loss_partials {tag} pair {k}: sum {s!r} want {want[2 * k]!r} count {c} terms {terms[k]}")
        assert c == want[2 * k + 1], (tag, k)                         # counts: exact
        # fp32 inputs accumulated in float64 against a float64 reference: summation order only; every term >= 0, so the
        # bound is n 2^-53 relative, n the number of terms of THIS sum
        assert abs(s - want[2 * k]) <= terms[k] * 2.0 ** -53 * abs(want[2 * k]), (tag, k, s, want[2 * k])
        if terms[k] == 0:
            assert s == 0.0 and c == 0.0, (tag, k)                    # an absent array leaves its pair at exactly (0, 0)
        if means is not None:
            assert means.dtype == np.float32
            if c == 0:
                assert np.isnan(means[k]), (tag, k)
            else:                                                    # (the sum itself was just held to the reference)
                assert means[k] == np.float32(s / c), (tag, k)


def test_loss_partials_joint_stage_size_block_cap_binds(M):
    """(a) N = 1024, S = 128 / 384, everything present: 530 432 elements > 256 blocks x 256 threads x 8, the grid is capped
    and every thread walks its grid-stride loop more than once."""
    rng = np.random.default_rng(11)
    N = 1024
    c, f = _loss_pass(rng, N, 128), _loss_pass(rng, N, 384)
    assert 2 * 3 * N + N * (128 + 384) > 256 * 256 * 8
    target = rng.random((N, 3)).astype(np.float32)
    got, means, _ = _loss_partials(c, f, _dev(target), N, ALL4, ALL4)
    want, terms = _loss_reference((c, f), (ALL4, ALL4), target, N)
    _check_loss(got, means, want, terms, "joint")


@pytest.mark.parametrize("kinds", [("mixed", "mixed"), ("empty", "mixed"), ("mixed", "empty"), ("empty", "full"), ("full", "empty"),
                                   ("empty", "empty")])
@pytest.mark.parametrize("N,Sc,Sf", [(5, 3, 3), (37, 64, 192), (300, 65, 1)])
def test_loss_partials_fallback_is_decided_per_pass(M, N, Sc, Sf, kinds):
    """(b), (c): small shapes, and a pass whose alphas are all below 0.01 beside one whose are not (both ways round): the
    all-true fallback of rendering.py:307-308 belongs to the pass, sum and count alike."""
    rng = np.random.default_rng(N * 100 + Sc + 7 * len(kinds[0]) + len(kinds[1]))
    c, f = _loss_pass(rng, N, Sc, kinds[0]), _loss_pass(rng, N, Sf, kinds[1])
    for p, kind in ((c, kinds[0]), (f, kinds[1])):
        n = int((p["alphas"] >= THR).sum())
        assert (n == 0) == (kind == "empty") and (n == p["alphas"].size) == (kind == "full")
    target = rng.random((N, 3)).astype(np.float32)
    got, means, _ = _loss_partials(c, f, _dev(target), N, ALL4, ALL4)
    want, terms = _loss_reference((c, f), (ALL4, ALL4), target, N)
    _check_loss(got, means, want, terms, f"{N}x{Sc}/{Sf} {kinds}")
    if kinds[0] == "empty":
        assert got[5] == N * Sc and got[9] == N * Sc
    if kinds[1] == "empty":
        assert got[7] == N * Sf and got[11] == N * Sf


@pytest.mark.parametrize("keep_c,keep_f", [
    (("rgb",), ("rgb",)), (("alphas", "disp_local"), ("alphas", "disp_local")), (("alphas", "disp_global"), ("alphas", "disp_global")),
    (("alphas", "disp_local", "disp_global"), ALL4), (ALL4, ("rgb", "alphas")), (ALL4, ()), (ALL4, None),
    (("rgb", "alphas", "disp_global"), ("rgb", "alphas", "disp_local")), (("rgb",), None)])
def test_loss_partials_absent_arrays_leave_exact_zeros(M, keep_c, keep_f):
    """(d): each optional array absent in turn, and fine == NULL: the pair of an absent array is exactly (0, 0), its mean nan,
    and the pairs that remain are held to the reference as before."""
    rng = np.random.default_rng(5)
    N = 41
    c, f = _loss_pass(rng, N, 70), _loss_pass(rng, N, 33)
    target = rng.random((N, 3)).astype(np.float32)
    fine = None if keep_f is None else f
    got, means, _ = _loss_partials(c, fine, _dev(target), N, keep_c, keep_f or ())
    want, terms = _loss_reference((c, fine), (keep_c, keep_f or ()), target, N)
    _check_loss(got, means, want, terms, f"{keep_c} {keep_f}")
    got2, none, _ = _loss_partials(c, fine, _dev(target), N, keep_c, keep_f or (), with_means=False)     # means6 is optional
    assert none is None and np.array_equal(got2, got)


def test_loss_partials_no_rays(M):
    """(e) n_rays = 0: all twelve numbers are 0, all six means nan."""
    rng = np.random.default_rng(2)
    c, f = _loss_pass(rng, 0, 64), _loss_pass(rng, 0, 192)
    # (an empty tensor has no address: hand over a live buffer, as a caller holding a zero-ray view of a larger tensor does)
    live = torch.zeros(8, device="cuda")
    for p in (c, f):
        p["dev"] = {k: live for k in ALL4}
    got, means, _ = _loss_partials(c, f, live, 0, ALL4, ALL4)
    assert np.array_equal(got, np.zeros(12)) and np.isnan(means).all()


# ------------------------------------------------------------------------------------------------ 3. mf_loss_partials_backward
def _grad_pass(rng, N, S, mask_kind, ray_width=9):
    """A pass for the backward: rays, depths and reconstructed points whose x - recon has a sign no fp32 contraction of
    x = o + d z can change (|x - recon| >= 1e-3 against an ulp of 1e-6); rays 2, 7, 12, ... have a direction of exactly 0
    (x == o whatever the contraction) and recon == o on some of their components: the exact-zero branch."""
    p = _loss_pass(rng, N, S, mask_kind)
    rays = rng.standard_normal((N, ray_width)).astype(np.float32)
    rays[2::5, 3:6] = 0.0
    z = (2.0 + 4.0 * rng.random((N, S))).astype(np.float32)
    x = rays[:, None, 0:3].astype(np.float64) + rays[:, None, 3:6].astype(np.float64) * z[:, :, None].astype(np.float64)
    p.update(rays=rays, z=z, x=x)
    for name in ("recon_local", "recon_global"):
        delta = (1e-3 + 1e-2 * rng.random((N, S, 3))) * rng.choice([-1.0, 1.0], size=(N, S, 3))
        rec = (x + delta).astype(np.float32)
        zero = np.zeros((N, S, 3), dtype=bool)
        zero[2::5] = rng.random(zero[2::5].shape) < 0.5
        rec = np.where(zero, np.broadcast_to(rays[:, None, 0:3], rec.shape), rec)
        assert (np.abs(x - rec)[~zero] > 5e-4).all() and (x[zero] == rec[zero]).all() and zero.any()
        p[name] = np.ascontiguousarray(rec.reshape(N * S, 3))
    return p


def _seeds_reference(p, q, target, g12):
    """The header's formulas in float64, rounded where the kernel says it rounds; the all-true fallback decided from the
    mask itself, on the CPU."""
    N, S = p["alphas"].shape
    n_masked = int((p["alphas"] >= THR).sum())
    every = n_masked in (0, N * S)                                   # empty mask -> all elements (rendering.py:307-308)
    out = dict(g_rgb=np.float32(g12[2 * q]) * (np.float32(2) * (p["rgb"] - target)))      # fp32, every operation rounded
    for name, j in (("recon_local", 4), ("recon_global", 8)):
        m = np.ones((N, S), dtype=bool) if every else (p["alphas"] >= THR)
        seed = np.float32(g12[j + 2 * q] / 3.0)
        sign = np.sign(p["x"] - p[name].reshape(N, S, 3)).astype(np.float32)
        out["g_" + name] = np.where(m[:, :, None], -sign * seed, np.float32(0)).astype(np.float32).reshape(N * S, 3)
    return out


GRAD_OUTS = ("g_rgb", "g_recon_local", "g_recon_global")


def _loss_backward(passes, target, N, out12_dev, g12, skip=()):
    """mf_loss_partials_backward with every output prefilled with nan; `skip`: (pass index, output name) pairs left NULL."""
    import moco_flow_amd._lib as L
    structs, outs, keep = [], [], []
    for q, p in enumerate(passes):
        if p is None:
            structs.append(None)
            outs.append(None)
            continue
        S = p["S"]
        d = {k: _dev(p[k]) for k in ("rgb", "alphas", "rays", "z", "recon_local", "recon_global")}
        keep.append(d)
        o = {name: torch.full((N if name == "g_rgb" else N * S, 3), float("nan"), device="cuda") for name in GRAD_OUTS}
        s = L.mf_loss_grad_pass()
        s.rgb, s.alphas, s.n_samples, s.rays, s.ray_stride, s.z_vals = L.ptr(d["rgb"]), L.ptr(d["alphas"]), S, L.ptr(d["rays"]), p["rays"].shape[1], L.ptr(d["z"])
        s.recon_local, s.recon_global = L.ptr(d["recon_local"]), L.ptr(d["recon_global"])
        for name in GRAD_OUTS:
            setattr(s, name, None if (q, name) in skip else L.ptr(o[name]))
        structs.append(s)
        outs.append(o)
    g12_dev = _dev(np.asarray(g12, dtype=np.float64))
    L.check(L.lib().mf_loss_partials_backward(ctypes.byref(structs[0]), ctypes.byref(structs[1]) if structs[1] is not None else None,
                                              L.ptr(target), N, L.ptr(out12_dev), L.ptr(g12_dev), _stream()), "mf_loss_partials_backward")
    torch.cuda.synchronize()
    return [None if o is None else {k: v.cpu() for k, v in o.items()} for o in outs]


def _check_seeds(passes, target, N, g12, skip=()):
    """Forward launch on the pass arrays (its out12 is what the backward reads), then the seeds against the reference."""
    target_dev = _dev(target)
    got12, _, out12_dev = _loss_partials(passes[0], passes[1], target_dev, N, ALL4, ALL4 if passes[1] is not None else ())
    outs = _loss_backward(passes, target_dev, N, out12_dev, g12, skip)
    for q, p in enumerate(passes):
        if p is None:
            continue
        want = _seeds_reference(p, q, target, g12)
        mask = p["alphas"] >= THR
        # the count the backward reads is the forward kernel's: held to the mask here, so kernel and reference cannot move together
        assert got12[4 + 2 * q + 1] == got12[8 + 2 * q + 1] == (int(mask.sum()) if mask.any() else mask.size), q
        for name, w in want.items():
            got, w = outs[q][name], torch.from_numpy(w)
            if (q, name) in skip:
                continue
            assert not bool(torch.isnan(got).any()), (q, name)        # written whole
            assert torch.equal(got, w), (q, name, int((got != w).sum()))
            if name != "g_rgb" and mask.any() and not mask.all():     # mask off -> exactly 0
                off = torch.from_numpy(~mask.reshape(-1))
                assert bool((got[off] == 0).all()) and bool((got[~off] != 0).any()), (q, name)
    return got12


@pytest.mark.parametrize("kinds", [("mixed", "empty"), ("full", "mixed"), ("empty", "full"), ("mixed", None)])
@pytest.mark.parametrize("N,Sc,Sf,ray_width", [(7, 3, 5, 9), (40, 64, 192, 11)])
def test_loss_backward_seeds_exact(M, N, Sc, Sf, ray_width, kinds):
    """The seeds of mf_loss_partials_backward, bit for bit: g_recon = -/+ fp32(g12 / 3) or 0, g_rgb the fp32 expression, zeros
    where the mask is off, every buffer written whole (prefilled with nan), the all-true fallback taken exactly when the
    count of the forward launch on the same arrays says so: once with an empty mask, once with a full one."""
    rng = np.random.default_rng(N + 13 * Sc + len(kinds[0]))
    c = _grad_pass(rng, N, Sc, kinds[0], ray_width)
    f = None if kinds[1] is None else _grad_pass(rng, N, Sf, kinds[1], ray_width)
    target = rng.random((N, 3)).astype(np.float32)
    got12 = _check_seeds((c, f), target, N, rng.standard_normal(12))
    for q, (p, kind) in enumerate(((c, kinds[0]), (f, kinds[1]))):
        if kind in ("empty", "full"):
            assert got12[4 + 2 * q + 1] == N * p["S"] == got12[8 + 2 * q + 1]
        elif kind == "mixed":
            assert 0 < got12[4 + 2 * q + 1] < N * p["S"]


@pytest.mark.parametrize("skip", [((0, "g_rgb"),), ((0, "g_recon_local"),), ((1, "g_recon_global"),), ((0, "g_recon_local"), (0, "g_recon_global")),
                                  ((1, "g_rgb"), (1, "g_recon_local"), (1, "g_recon_global")), ((0, "g_rgb"), (1, "g_recon_local"))])
def test_loss_backward_null_outputs_are_skipped_one_by_one(M, skip):
    """Any output pointer may be NULL: the others are what they are in the full call."""
    rng = np.random.default_rng(31)
    N = 23
    c, f = _grad_pass(rng, N, 37, "mixed"), _grad_pass(rng, N, 65, "mixed")
    target = rng.random((N, 3)).astype(np.float32)
    _check_seeds((c, f), target, N, rng.standard_normal(12), skip)


def test_loss_backward_block_cap_binds(M):
    """N = 8192, S = 128 / 192: 2 670 592 elements > 2048 blocks x 256 threads x 4, the grid is capped and the grid-stride loops
    run more than once; a mixed mask beside an empty one."""
    rng = np.random.default_rng(77)
    N = 8192
    assert 2 * 3 * N + N * (128 + 192) > 2048 * 256 * 4
    c, f = _grad_pass(rng, N, 128, "mixed"), _grad_pass(rng, N, 192, "empty")
    target = rng.random((N, 3)).astype(np.float32)
    _check_seeds((c, f), target, N, rng.standard_normal(12))


def test_loss_backward_no_rays_and_no_outputs(M):
    """n_rays = 0, and a call whose outputs are all NULL, return MF_OK."""
    import moco_flow_amd._lib as L
    s = L.mf_loss_grad_pass()
    buf = torch.zeros(12, dtype=torch.float64, device="cuda")
    assert L.lib().mf_loss_partials_backward(ctypes.byref(s), None, None, 0, L.ptr(buf), L.ptr(buf), _stream()) == 0
    assert L.lib().mf_loss_partials_backward(ctypes.byref(s), None, None, 5, L.ptr(buf), L.ptr(buf), _stream()) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 4. mf_sample_pdf
PDF_EPS = 2.0 ** -10


def _dyadic_rays(rng, N, nw):
    """Integer counts k (N, nw), k >= 1, every row summing to a power of two Q: with eps = 2^-10 and weights
    w = (k - 1) eps, w + eps = k eps, the normaliser Q eps, pdf = k / Q and every partial sum of the cdf are exact in fp32 in
    any order -- searchsorted has one right answer.  Rows 0, 3, 6, ...: a third of the weights 0 (k = 1); rows 1, 4, ...: the
    mass on the first quarter of the bins (many eps-only bins); where nw is a power of two, rows 4, 9, ...: every weight 0,
    the uniform pdf (for any other nw, 1 / nw is not a binary fraction and such a row could not be exact)."""
    Q = 4
    while Q < 4 * nw:
        Q *= 2
    k = np.ones((N, nw), dtype=np.int64)
    uniform = np.zeros(N, dtype=bool)
    for r in range(N):
        if nw & (nw - 1) == 0 and r % 5 == 4:
            uniform[r] = True
            continue
        if r % 3 == 0:
            free = rng.permutation(nw)[nw // 3:]
        elif r % 3 == 1:
            free = np.arange(max(1, nw // 4))
        else:
            free = np.arange(nw)
        k[r] += np.bincount(free[rng.integers(len(free), size=Q - nw)], minlength=nw)
    Qr = np.where(uniform, nw, Q)
    assert (k.sum(1) == Qr).all()
    w = ((k - 1) * PDF_EPS).astype(np.float32)
    cdf = np.concatenate([np.zeros((N, 1)), np.cumsum(k, 1) / Qr[:, None]], 1)           # exact: binary fractions
    assert np.array_equal(cdf.astype(np.float32).astype(np.float64), cdf) and (cdf[:, -1] == 1.0).all()
    return w, cdf, uniform


def _planted_u(rng, cdf, Mi):
    """(N, Mi) draws in [0, 1): every third column exactly ON a cdf value of its ray; 0 and 1.0 planted on rays 1, 5, ... /
    2, 6, ... (first / last column)."""
    N, nb = cdf.shape
    u = rng.random((N, Mi)).astype(np.float32)
    for m in range(0, Mi, 3):
        u[:, m] = cdf[np.arange(N), rng.integers(nb, size=N)]
    u[1::4, 0] = 0.0
    u[2::4, -1] = 1.0
    return u


def _dyadic_depths(rng, N, S):
    """Ascending coarse depths on the grid 2 + j / 64: the mid-points 0.5 (z_i + z_i+1) are exact in fp32 too."""
    return (2.0 + np.cumsum(rng.integers(1, 5, size=(N, S)), 1) / 64.0).astype(np.float32)


def _sample_pdf(bins, z_coarse, w, w_stride, N, nb, Mi, u, u_stride, cdf_in=None, eps=PDF_EPS, w_offset=0):
    """mf_sample_pdf_eps on device tensors -> (z_new, inds) on the CPU."""
    import moco_flow_amd._lib as L
    inds = torch.full((N, Mi), -1, dtype=torch.int32, device="cuda")
    out = torch.full((N, Mi), float("nan"), device="cuda")
    wp = None if w is None else w.data_ptr() + 4 * w_offset
    L.check(L.lib().mf_sample_pdf_eps(L.ptr(bins), L.ptr(z_coarse), wp, w_stride, N, nb, Mi, L.ptr(u), u_stride, L.ptr(cdf_in),
                                      L.ptr(out), L.ptr(inds), None, float(eps), _stream()), "mf_sample_pdf_eps")
    torch.cuda.synchronize()
    return out.cpu(), inds.cpu()


def _check_pdf(R, got, bins, w, u, Mi, cdf, tag):
    """Against the float64 oracle: its cdf is the exact one; every index equal, the u = 1.0 column included and no element
    left out; samples within 1e-6 max-rel."""
    z_new, inds = got
    want = R.sample_pdf_full(torch.from_numpy(bins).double(), torch.from_numpy(w).double(), Mi, eps=PDF_EPS, u=torch.from_numpy(u).double())
    assert np.array_equal(want["cdf"].numpy(), cdf), tag
    bad = int((inds.long() != want["inds"]).sum())
    err = relerr(z_new, want["samples"])
    print(f"sample_pdf {tag}: {bad} of {inds.numel()} indices differ, samples max-rel {err:.3e}")
    assert bad == 0, (tag, bad)
    assert err <= 1e-6, (tag, err)


PDF_BINS = (2, 3, 5, 63, 64, 65, 66, 129, 255)
PDF_M = (1, 63, 64, 65, 200)


@pytest.mark.parametrize("nb", PDF_BINS)
def test_sample_pdf_own_cdf_exact_indices(M, R, nb):
    """mf_sample_pdf_eps on its OWN pdf / normaliser / cdf (the k0 block loop and its kmax trip count at n_bins > 64, one
    weight at n_bins = 2, n_bins not a multiple of 4), inputs with nothing left to rounding: indices torch.equal to the
    float64 oracle's for every draw -- u on a cdf value, 0 and 1.0 included --, samples within 1e-6.  Explicit bins; bins as
    the mid-points of z_coarse; the weights embedded in a wider matrix (w_stride > n_bins - 1); one shared u row (u_stride 0)."""
    rng = np.random.default_rng(nb)
    N, nw = 40, nb - 1
    w, cdf, uniform = _dyadic_rays(rng, N, nw)
    assert uniform.any() == (nw & (nw - 1) == 0) and ((w == 0).sum(1) >= nw // 3)[0::3].all()
    bins = np.sort(2 + 4 * rng.random((N, nb)), -1).astype(np.float32)
    z = _dyadic_depths(rng, N, nb + 1)
    mid = 0.5 * (z[:, :-1].astype(np.float64) + z[:, 1:].astype(np.float64))
    assert np.array_equal(mid.astype(np.float32).astype(np.float64), mid)
    mid = mid.astype(np.float32)
    wide = np.full((N, nw + 7), 1e3, dtype=np.float32)               # (a read outside the ray's nb - 1 weights would show)
    wide[:, 3:3 + nw] = w
    dbins, dz, dw, dwide = _dev(bins), _dev(z), _dev(w), _dev(wide)
    for Mi in PDF_M:
        u = _planted_u(rng, cdf, Mi)
        du = _dev(u)
        _check_pdf(R, _sample_pdf(dbins, None, dw, nw, N, nb, Mi, du, Mi), bins, w, u, Mi, cdf, f"nb={nb} M={Mi} bins")
        _check_pdf(R, _sample_pdf(None, dz, dw, nw, N, nb, Mi, du, Mi), mid, w, u, Mi, cdf, f"nb={nb} M={Mi} z_coarse")
        _check_pdf(R, _sample_pdf(dbins, None, dwide, nw + 7, N, nb, Mi, du, Mi, w_offset=3), bins, w, u, Mi, cdf, f"nb={nb} M={Mi} w_stride")
        # one shared row: multiples of 1 / 64 are cdf values of many rays at once (every cdf value is a multiple of 1 / Q)
        row = rng.random(Mi).astype(np.float32)
        row[::3] = rng.integers(0, 65, size=len(row[::3])) / 64.0
        row[0] = 0.0 if Mi % 2 else 1.0
        shared = np.ascontiguousarray(np.broadcast_to(row, (N, Mi)))
        _check_pdf(R, _sample_pdf(dbins, None, dw, nw, N, nb, Mi, _dev(row), 0), bins, w, shared, Mi, cdf, f"nb={nb} M={Mi} u_stride=0")


def test_sample_pdf_largest_accepted_shape(M, R):
    """The last n_bins + M the LDS limit lets through (4 waves x 4096 floats = 64 KiB exactly) is not refused for size and
    computes the oracle's indices (tests/test_host_cpu.py holds the first refused one, one draw more, on the host)."""
    nb, Mi = 64, 1
    while pdf_per_wave_floats(nb, Mi + 1) * 16 <= 64 * 1024:
        Mi += 1
    assert pdf_per_wave_floats(nb, Mi) == 4096 and pdf_per_wave_floats(nb, Mi + 1) > 4096
    rng = np.random.default_rng(3)
    N, nw = 6, nb - 1
    w, cdf, _ = _dyadic_rays(rng, N, nw)
    bins = np.sort(2 + 4 * rng.random((N, nb)), -1).astype(np.float32)
    u = _planted_u(rng, cdf, Mi)
    _check_pdf(R, _sample_pdf(_dev(bins), None, _dev(w), nw, N, nb, Mi, _dev(u), Mi), bins, w, u, Mi, cdf, f"nb={nb} M={Mi} largest")


def test_sample_pdf_given_cdf_zero_width_interval(M, R):
    """cdf_in with intervals narrower than eps under planted draws (1 / 4096 < 2^-10), a draw on the last cdf value, and draws
    on a run of equal cdf values: `denom < eps -> 1` (rendering.py:41-42).  The cdf handed in is the float64 oracle's own for
    dyadic weights (exact in fp32), so the oracle's samples -- the same branch -- are the reference."""
    rng = np.random.default_rng(9)
    N, Q = 12, 4096
    k = np.tile(np.array([2047, 1, 1023, 1, 1, 1022, 1], dtype=np.int64), (N, 1))
    for r in range(N):
        k[r] = k[r][rng.permutation(7)]
    nw, nb, Mi = 7, 8, 9
    w = ((k - 1) * PDF_EPS).astype(np.float32)
    cdf = np.concatenate([np.zeros((N, 1)), np.cumsum(k, 1) / Q], 1)
    bins = np.sort(2 + 4 * rng.random((N, nb)), -1).astype(np.float32)
    u = rng.random((N, Mi)).astype(np.float32)
    narrow = np.argmax(k == 1, axis=1)                                # a 1 / 4096 interval of every ray
    u[:, 0] = cdf[np.arange(N), narrow] + 2.0 ** -13                  # inside it
    u[:, 1] = cdf[np.arange(N), narrow]                               # on its left edge
    u[:, 2] = 1.0                                                     # the last cdf value: below == above, denom == 0
    u[:, 3] = 0.0
    want = R.sample_pdf_full(torch.from_numpy(bins).double(), torch.from_numpy(w).double(), Mi, eps=PDF_EPS, u=torch.from_numpy(u).double())
    assert np.array_equal(want["cdf"].numpy(), cdf)
    denom = torch.gather(want["cdf"], 1, want["above"]) - torch.gather(want["cdf"], 1, want["below"])
    assert bool((denom[:, :3] < PDF_EPS).all()) and bool((denom[:, 2] == 0).all())    # these draws DO take the branch
    z_new, inds = _sample_pdf(_dev(bins), None, None, nw, N, nb, Mi, _dev(u), Mi, cdf_in=_dev(cdf.astype(np.float32)))
    assert torch.equal(inds.long(), want["inds"])
    assert relerr(z_new, want["samples"]) <= 1e-6
    # what the branch decides: inside the narrow interval the sample moves by 2^-13 of the bin, not by half of it
    dbl = torch.from_numpy(bins).double()
    b0, b1 = torch.gather(dbl, 1, want["below"][:, :1])[:, 0], torch.gather(dbl, 1, want["above"][:, :1])[:, 0]
    assert relerr(z_new[:, 0], b0 + 2.0 ** -13 * (b1 - b0)) <= 1e-6
    # a run of equal cdf values (a cdf no pdf with eps > 0 produces): searchsorted(right=True) steps over the whole run;
    # reference: rendering.py:30-45 restated in float64
    cdf2 = np.tile(np.array([0, 0.25, 0.5, 0.5, 0.5, 0.75, 1.0, 1.0], dtype=np.float32), (N, 1))
    u2 = np.tile(np.array([0.5, 0.25, 0.0, 1.0, 0.625, 0.4999999], dtype=np.float32), (N, 1))
    z2, i2 = _sample_pdf(_dev(bins), None, None, nw, N, nb, 6, _dev(u2), 6, cdf_in=_dev(cdf2))
    want_i = np.stack([np.searchsorted(cdf2[r].astype(np.float64), u2[r].astype(np.float64), side="right") for r in range(N)])
    assert np.array_equal(i2.numpy(), want_i) and want_i[0].tolist() == [5, 2, 1, 8, 5, 2]
    below, above = np.maximum(want_i - 1, 0), np.minimum(want_i, nw)
    rows = np.arange(N)[:, None]
    c0, c1, b0, b1 = (a.astype(np.float64)[rows, i] for a, i in ((cdf2, below), (cdf2, above), (bins, below), (bins, above)))
    den = c1 - c0
    den[den < PDF_EPS] = 1
    assert relerr(z2, b0 + (u2 - c0) / den * (b1 - b0)) <= 1e-6


@pytest.mark.parametrize("S", [3, 4, 5, 65, 129, 200])
def test_sample_pdf_merge_argument_plumbing(M, S):
    """mf_sample_pdf_merge(z_coarse, weights) against the general entry with bins = mid-points, weights[:, 1:-1]: the same
    z_new and indices bit for bit -- KERNEL AGAINST KERNEL, a check of the argument plumbing only (the arithmetic is held to
    the oracle above) -- and z_out = torch.sort of the union, as test_resample_merge_is_torch_sort_of_the_union has it."""
    import moco_flow_amd._lib as L
    rng = np.random.default_rng(S)
    N = 33
    z = _dyadic_depths(rng, N, S)
    w = rng.random((N, S)).astype(np.float32)
    w[:, S // 3: S // 2] = 0.0
    w[::5] = 0.0                                                     # eps-only pdf: uniform
    dz, dw = _dev(z), _dev(w)
    dmid = _dev((0.5 * (z[:, :-1].astype(np.float64) + z[:, 1:])).astype(np.float32))
    dinner = dw[:, 1:-1].contiguous()
    for Mi in (1, 64, 200):
        u = rng.random((N, Mi)).astype(np.float32)
        u[1::4, 0], u[2::4, -1] = 0.0, 1.0
        du = _dev(u)
        z_out = torch.full((N, S + Mi), float("nan"), device="cuda")
        inds = torch.full((N, Mi), -1, dtype=torch.int32, device="cuda")
        z_new = torch.full((N, Mi), float("nan"), device="cuda")
        L.check(L.lib().mf_sample_pdf_merge(L.ptr(dz), L.ptr(dw), N, S, Mi, L.ptr(du), L.ptr(z_out), L.ptr(inds), L.ptr(z_new), _stream()),
                "mf_sample_pdf_merge")
        torch.cuda.synchronize()
        want_new, want_inds = _sample_pdf(dmid, None, dinner, S - 2, N, S - 1, Mi, du, Mi, eps=1e-5)
        assert torch.equal(z_new.cpu(), want_new) and torch.equal(inds.cpu(), want_inds), (S, Mi)
        assert torch.equal(z_out.cpu(), torch.sort(torch.cat([torch.from_numpy(z), want_new], -1), -1)[0]), (S, Mi)


# ------------------------------------------------------------------------------------------------ 5. mf_knn1
def _lattice(rng, n):
    """n integer points with coordinates in [-480, 480] (units of 1/8): half of them on the coarse sub-lattice of multiples
    of 64, so that duplicates and exact ties are frequent."""
    p = rng.integers(-480, 481, size=(n, 3))
    coarse = rng.random(n) < 0.5
    p[coarse] = rng.integers(-7, 8, size=(int(coarse.sum()), 3)) * 64
    return p.astype(np.int64)


def _knn_reference(ref, qry):
    """int64 squared distances, argmin with first-minimum-wins -> (indices, squared distances in units of 1/64)."""
    Q = len(qry)
    want_i, want_d2 = np.empty(Q, dtype=np.int64), np.empty(Q, dtype=np.int64)
    for lo in range(0, Q, 256):
        d2 = sum((qry[lo:lo + 256, None, c] - ref[None, :, c]) ** 2 for c in range(3))
        want_i[lo:lo + 256] = np.argmin(d2, axis=1)
        want_d2[lo:lo + 256] = d2.min(axis=1)
    return want_i, want_d2


@pytest.mark.parametrize("Q", [1, 255, 256, 257, 5000])
@pytest.mark.parametrize("V", [1, 2, 1023, 1024, 1025, 2049, 6890])
def test_knn1_exact_on_a_lattice(M, V, Q):
    """mf_knn1 on lattice points k / 8, |k| <= 512: every difference, square and fma of the kernel is exact in fp32, squared
    distances are integers / 64, so the int64 argmin with first-minimum-wins is THE answer for every query -- across the
    1024-point LDS tiles (a duplicate at 5 and 1024 + 5, a tie between 1023 and 1024, the last index as the only nearest
    neighbour) and the 256-query blocks."""
    import moco_flow_amd._lib as L
    rng = np.random.default_rng(V * 10 + Q)
    ref, qry = _lattice(rng, V), _lattice(rng, Q)
    plants = []                                                      # (query point, the index it must get), outside the cloud's box
    if V >= 1030:
        ref[5] = (509, -511, 505)
        ref[1024 + 5] = ref[5]
        plants.append((ref[5].copy(), 5))
    if V >= 1025:
        ref[1023], ref[1024] = (500, 500, 496), (500, 500, 504)
        plants.append((np.array([500, 500, 500]), 1023))
    if V - 1 == 1024:
        plants.append((np.array([500, 500, 506]), V - 1))
    else:
        ref[V - 1] = (-500, -500, -500)
        plants.append((np.array([-501, -500, -499]), V - 1))
    plants = plants[Q % len(plants):] + plants[:Q % len(plants)]      # (Q = 1 has room for one: a different one per V)
    for j, (pt, _) in enumerate(plants):
        if j < Q:
            qry[j] = pt
        if Q > 2 * len(plants):
            qry[Q - 1 - j] = pt
    want_i, want_d2 = _knn_reference(ref, qry)
    for j, (_, idx) in enumerate(plants):
        if j < Q:
            assert want_i[j] == idx, (j, idx)                         # the plants are what they claim to be
    assert int(want_d2.max()) < 2 ** 24                               # exact in fp32
    dref, dq = _dev((ref / 8.0).astype(np.float32)), _dev((qry / 8.0).astype(np.float32))
    dist = torch.full((Q,), float("nan"), device="cuda")
    ind = torch.full((Q,), -1, dtype=torch.int64, device="cuda")
    L.check(L.lib().mf_knn1(L.ptr(dref), V, L.ptr(dq), Q, L.ptr(dist), L.ptr(ind), _stream()), "mf_knn1")
    torch.cuda.synchronize()
    assert torch.equal(ind.cpu(), torch.from_numpy(want_i)), (V, Q, int((ind.cpu() != torch.from_numpy(want_i)).sum()))
    want_d = np.sqrt(want_d2 / 64.0).astype(np.float32)
    got_d = dist.cpu().numpy()
    assert (np.abs(got_d.astype(np.float64) - want_d.astype(np.float64)) <= np.spacing(want_d).astype(np.float64)).all()   # sqrtf: 1 ulp
    assert (got_d[want_d2 == 0] == 0).all()


def test_knn1_wrapper_on_the_lattice(M):
    """The module the trainers call (knn_cuda.KNN(k=1, transpose_mode=True)) on the same kind of input: (1, Q, 1) shapes,
    int64 indices, the planted tie across the tile boundary."""
    from moco_flow_amd.knn import KNN
    rng = np.random.default_rng(4)
    ref, qry = _lattice(rng, 2049), _lattice(rng, 300)
    ref[1023], ref[1024] = (500, 500, 496), (500, 500, 504)
    qry[7] = (500, 500, 500)
    d, i = KNN(k=1, transpose_mode=True)(_dev((ref / 8.0).astype(np.float32))[None], _dev((qry / 8.0).astype(np.float32))[None])
    want_i, _ = _knn_reference(ref, qry)
    assert i.shape == (1, 300, 1) and i.dtype == torch.int64 and int(i[0, 7, 0]) == 1023
    assert torch.equal(i[0, :, 0].cpu(), torch.from_numpy(want_i))


# ------------------------------------------------------------------------------------------------ 6. compose, embed rows, rays
@pytest.mark.parametrize("B", [1, 255, 256, 257, 4099])
def test_image_compose_pixel_classes(M, B):
    """mf_image_compose direct, against the numpy restatement of trainer/trainer_moco_flow.py:252-263:
      not rendered -> background colour, depth 10;          rendered, opacity > 0 -> the ray's colour and depth;
      rendered, opacity 0 (or -0) -> background, depth 8;   rendered, opacity negative or nan -> black, depth 8
    (`foreground_mask > 0` and `== 0` are both false there).  With a mask + rank, then without a mask and rank == NULL."""
    import moco_flow_amd._lib as L
    rng = np.random.default_rng(B)
    OFF, POS, ZERO, NEGZERO, NEG, NAN = range(6)
    for shift in range(6):
        for masked in (True, False):
            cls = (np.arange(B) * 5 // 3 + shift) % 6
            if not masked:
                cls = np.where(cls == OFF, POS, cls)
            msk = (cls != OFF).astype(np.uint8)
            rank = np.where(msk != 0, np.cumsum(msk) - 1, 0).astype(np.int64)
            Mr = max(int(msk.sum()), 1)
            vals = {POS: 0.05 + rng.random(B), ZERO: np.zeros(B), NEGZERO: -np.zeros(B), NEG: -0.05 - rng.random(B), NAN: np.full(B, np.nan)}
            opacity = np.full(Mr, 0.5, dtype=np.float32)
            for c, v in vals.items():
                sel = cls == c
                opacity[rank[sel]] = v[sel].astype(np.float32)
            rgb, depth = rng.random((Mr, 3)).astype(np.float32), (2 + rng.random(Mr)).astype(np.float32)
            bg = (2 + rng.random((B, 3))).astype(np.float32)
            want_img, want_d = np.zeros((B, 3), dtype=np.float32), np.full(B, 8, dtype=np.float32)
            want_d[cls == OFF] = 10
            back = (cls == OFF) | (cls == ZERO) | (cls == NEGZERO)
            want_img[back] = bg[back]
            want_img[cls == POS], want_d[cls == POS] = rgb[rank[cls == POS]], depth[rank[cls == POS]]
            img, dout = torch.full((B, 3), float("nan"), device="cuda"), torch.full((B,), float("nan"), device="cuda")
            dm, dr = (_dev(msk), _dev(rank)) if masked else (None, None)
            keep = [_dev(opacity), _dev(rgb), _dev(depth), _dev(bg)]
            L.check(L.lib().mf_image_compose(L.ptr(dm), L.ptr(dr), B, *[L.ptr(t) for t in keep], L.ptr(img), L.ptr(dout), _stream()),
                    "mf_image_compose")
            torch.cuda.synchronize()
            assert np.array_equal(img.cpu().numpy(), want_img), (B, shift, masked)
            assert np.array_equal(dout.cpu().numpy(), want_d), (B, shift, masked)


NOF_WEIGHTS = {0: [], 3: [1.0, 0.4, 0.0], 5: [1.0, 0.4, 0.0, 1.0, 1.0]}


@pytest.mark.parametrize("n_freqs", [0, 3, 5])
@pytest.mark.parametrize("S", [1, 7, 64])
@pytest.mark.parametrize("P", [1, 3, 4, 5, 1001])
def test_nof_embed_rows_direct(M, P, S, n_freqs):
    """mf_nof_embed_rows into a nan-filled (P, 80) buffer, against float64:
    [x | w_k sin(f_k x) | w_k cos(f_k x) ... | 0 to column 33 | ind_emb[row // S] | 0 to column 80].  sin / cos within the 2e-6
    max-rel the embedding is held to elsewhere (|x| <= 1.5); the copied columns bit for bit; muted (k >= n_freqs) and padding
    columns exactly 0, not stale: the weight-gradient launches read all 80."""
    import moco_flow_amd._lib as L
    rng = np.random.default_rng(P * 100 + S * 10 + n_freqs)
    pts = rng.uniform(-1.5, 1.5, size=(P, 3)).astype(np.float32)
    n_rays = (P + S - 1) // S
    e = L.mf_embedding()
    e.in_channels, e.n_freqs = 3, n_freqs
    for k, wk in enumerate(NOF_WEIGHTS[n_freqs]):
        e.freq[k], e.weight[k] = 2.0 ** k, wk
    for ind_width in (0, 5, 33):
        ind = rng.standard_normal((n_rays, max(ind_width, 1))).astype(np.float32)
        want = np.zeros((P, 80))
        want[:, 0:3] = pts
        for k, wk in enumerate(NOF_WEIGHTS[n_freqs]):
            arg = 2.0 ** k * pts.astype(np.float64)
            want[:, 3 + 6 * k:6 + 6 * k] = float(np.float32(wk)) * np.sin(arg)
            want[:, 6 + 6 * k:9 + 6 * k] = float(np.float32(wk)) * np.cos(arg)
        if ind_width:
            want[:, 33:33 + ind_width] = ind[np.arange(P) // S, :ind_width]
        out = torch.full((P, 80), float("nan"), device="cuda")
        dpts, dind = _dev(pts), (_dev(ind) if ind_width else None)
        L.check(L.lib().mf_nof_embed_rows(ctypes.byref(e), L.ptr(dpts), L.ptr(dind), ind_width, S, P, L.ptr(out), _stream()), "mf_nof_embed_rows")
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        tag = (P, S, n_freqs, ind_width)
        assert not np.isnan(got).any(), tag
        assert np.array_equal(got[:, 0:3], pts), tag
        assert np.array_equal(got[:, 33:33 + ind_width], want[:, 33:33 + ind_width].astype(np.float32)), tag
        if n_freqs:
            assert relerr(got[:, 3:3 + 6 * n_freqs], want[:, 3:3 + 6 * n_freqs]) <= 2e-6, tag
            assert (got[:, 15:21] == 0).all(), tag                    # the frequency whose weight is 0
        assert (got[:, 3 + 6 * n_freqs:33] == 0).all() and (got[:, 33 + ind_width:80] == 0).all(), tag


def _oracle_rays64(R, H, W, focal, cx, cy, c2w, near, far, idx):
    torch.set_default_dtype(torch.float64)
    try:
        return R.make_rays(H, W, [float(focal)], (float(cx), float(cy)), None if c2w is None else c2w.astype(np.float64),
                           float(near), float(far), float(idx))
    finally:
        torch.set_default_dtype(torch.float32)


@pytest.mark.parametrize("H,W", [(1, 1), (1, 257), (257, 1), (37, 53)])
def test_make_rays_shapes_and_off_centre(M, R, H, W):
    """mf_make_rays against oracle/cpu_ref.py::make_rays evaluated in float64, at H W = 1, one over a block, a non-square
    image, an off-centre principal point, with and without c2w: directions within 1e-6, the near / far / idx columns and
    the origin (c2w[:, 3]) bit for bit."""
    import moco_flow_amd._lib as L
    rng = np.random.default_rng(H * 1000 + W)
    focal, cx, cy = np.float32(61.7), np.float32(0.31 * W + 1.25), np.float32(0.77 * H - 0.5)
    near, far, idx = np.float32(1.37), np.float32(5.11), np.float32(17.0)
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    c2w = np.concatenate([q, rng.standard_normal((3, 1)) * 2], 1).astype(np.float32)
    for mat in (c2w, None):
        want = _oracle_rays64(R, H, W, focal, cx, cy, mat, near, far, idx)
        assert want.dtype == torch.float64 and want.shape == (H * W, 9)
        out = torch.full((H * W, 9), float("nan"), device="cuda")
        arr = None if mat is None else (ctypes.c_float * 12)(*mat.reshape(-1).tolist())
        L.check(L.lib().mf_make_rays(H, W, float(focal), float(cx), float(cy), arr, float(near), float(far), float(idx), L.ptr(out),
                                     _stream()), "mf_make_rays")
        torch.cuda.synchronize()
        got = out.cpu()
        assert relerr(got, want) <= 1e-6 and relerr(got[:, 3:6], want[:, 3:6]) <= 1e-6, (H, W, mat is None)
        tail = torch.tensor([float(near), float(far), float(idx)], dtype=torch.float32)
        assert torch.equal(got[:, 6:9], want[:, 6:9].float()) and torch.equal(got[:, 6:9], tail.expand(H * W, 3))
        origin = torch.zeros(3) if mat is None else torch.from_numpy(mat[:, 3])
        assert torch.equal(got[:, 0:3], origin.expand(H * W, 3)), (H, W, mat is None)


def test_make_rays_wrapper(M, R):
    """camera.make_rays -- the function the trainers call -- at an off-centre, non-square shape."""
    from moco_flow_amd import camera
    c2w = np.array([[0.0, -1.0, 0.0, 0.5], [1.0, 0.0, 0.0, -2.0], [0.0, 0.0, 1.0, 3.0]], dtype=np.float32)
    rays = camera.make_rays(37, 53, 61.7, (17.25, 28.0), c2w, 1.37, 5.11, 4.0)
    want = _oracle_rays64(R, 37, 53, np.float32(61.7), 17.25, 28.0, c2w, np.float32(1.37), np.float32(5.11), 4.0)
    assert rays.shape == (37 * 53, 9) and relerr(rays, want) <= 1e-6 and torch.equal(rays[:, 6:9].cpu(), want[:, 6:9].float())
