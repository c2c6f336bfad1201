"""The fused point queries and the module-level forwards past the first trip of their persistent loops (-m gpu).

Every per-point kernel runs `for (tile = blockIdx.x; tile < ntiles; tile += gridDim.x)` with at most one workgroup per CU
(persistent_grid, mf_host.hpp).  Here every variant of query_sigma -- points_kernel_bf16<NOF, PERPT, X3> (mf_render_bf16.hip:
fast, no NoF / scalar index / per-point indices; bf16x3, no NoF / scalar index) and points_kernel<NOF> (mf_forward.hip) --
and NeRF.forward / NoF.forward (nerf_forward_kernel<DUMP>, nof_forward_kernel<8 | 16>, with and without the activation
dump) is launched at (#CUs + 1) tiles + 1 point: workgroups 0 and 1 take a second trip, the second one over a ragged tile of
one point, and the single LDS bias entry of a scalar index is reused across trips.  Per-point image indices are
IND_VALUES[i % 5] (tests/points_oracle.py): neighbouring lanes differ, every tile holds all five, so a lane that read
another point's bias rows, or a bias table written one entry off, computes different numbers.

The oracle (tests/points_oracle.py) evaluates subset(): the first tile, the two second-trip tiles, 256 seeded points between.
  (a) the fast mode against the oracle OF ITS ARITHMETIC (oracle/bf16_ref.BF16), in units of that oracle's own floor -- the same
      oracle with fp32 instead of float64 accumulation, at the same points: within 3 floors (the kernel's MFMA association order is
      a third order next to those two, and a ReLU flip is a discrete event), at least twice as far from a deliberately wrong oracle
      (lo products of the NoF's xyz block dropped; the NeRF's hidden operands split) and closer than to the fp32 oracle;
  (b) f32 and bf16x3 to the 1e-4 max-rel contract; bf16x3 no farther from BF16X3 than from F32 (1 dB) and >= 20 dB closer than
      to the oracle with unsplit hidden activations.  query_sigma(precision="bf16x3") with an index tensor runs the fp32 kernel;
  (c) a per-point launch = the five scalar-index launches on the points of each value, bit for bit;
  (d) prefixes, uneven splits and repeats of the large launch, bit for bit;
  (e) a NaN / inf point gives a NaN sigma in "bf16" and "bf16x3"  and moves no other point;
  (f) the module forwards at the same shape against cpu_ref, with (d), with and without the dump.
tests/test_points_oracle_cpu.py holds the preconditions (floor sizes, wrong oracles >= 10 floors away) without a GPU.

Measured on the MI355X (256 CUs; fast: 65 793 points, 769 compared; others: 32 897 points, 513 compared):
  (a) l2-rel of the fast kernel to BF16 [= floors; the floor; the fp32 oracle in floors; the wrong oracle in floors]
      no NoF       canonical-space sigma  3.32e-4 [1.16; 2.87e-4; 25.7; 24.4]
      scalar index canonical point        8.65e-7 [0.89; 9.74e-7; 96.8; 125.5]   sigma through the NoF 1.13e-3 [1.15; 9.83e-4; 19.3; 23.9]
      per point    canonical point        1.75e-6 [0.64; 2.73e-6; 35.6; 42.5]    sigma through the NoF 1.38e-3 [1.42; 9.70e-4; 18.4; 23.4]
      -- the point kernel sits at its floor as the render kernels do: no arithmetic of its own to model.
  (b) max-rel to cpu_ref, f32: sigma 1.0e-6 (no NoF) / 1.4e-5 (scalar) / 1.7e-5 (per point), canonical point 1.2e-7 / 7.7e-8;
      bf16x3: sigma 2.5e-5 (no NoF) / 2.2e-5 (scalar), canonical point 1.5e-7; with an index tensor the f32 figures (that kernel).
      bf16x3 PSNR-equiv to BF16X3 / F32 / unsplit hidden activations: canonical-space sigma 92.5 / 88.0 / 37.3 dB, sigma through
      the NoF 89.2 / 87.0 / 37.2 dB, canonical point 149.5 / 149.2 dB.
  (f) max-rel to cpu_ref 1.0e-6 (NeRF(dir)), 9.4e-7 (NeRF(ind) sigma), 1.5e-7 (quat NoF; displacement 1.9e-6), 7.6e-8 (bare NoF();
      displacement 1.4e-6); every dump forward bit-equal to its no-grad forward.
"""
import functools
from dataclasses import replace

import pytest
import torch

import points_oracle as P
from helpers import TOL, relerr

pytestmark = pytest.mark.gpu

VARIANTS = ("none", "nof_scalar", "nof_tensor")
IND_SCALAR = P.IND_VALUES[0]


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


@pytest.fixture(scope="module")
def B():
    from oracle import bf16_ref
    return bf16_ref


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def second_trip(prec):
    return P.second_trip(P.TILE[prec], cus())


def sizes(prec):
    t = P.TILE[prec]
    return (1, t - 1, t, t + 1, second_trip(prec))


def _split_points(n):
    """Two cuts of 0..n into three uneven non-empty parts."""
    a = max(1, n // 7)
    return a, min(n - 1, a + max(1, (2 * n) // 5))


def _load(module, sd):
    module.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return module.cuda()


@functools.lru_cache(maxsize=None)
def _models():
    import moco_flow_amd as M
    sd_n, sd_f = P.states()
    return dict(nerf=_load(M.NeRF(8, 256, 63, [4], "ind", 5), sd_n), nof=_load(M.NoF(4, 128, 33, [2], "ind", 33, True), sd_f),
                ex=M.Embedding(3, 10), nof_embs=[M.Embedding(3, 5), M.Embedding(1, 16)])


@functools.lru_cache(maxsize=None)
def _inputs(prec):
    """(xyz, ind) of the large launch of `prec`, on the host; the smaller launches are prefixes."""
    return P.inputs(second_trip(prec))


def _launch(prec, variant, xyz, ind):
    """query_sigma over host tensors xyz (n, 3) / ind (n,) -> {output name: device tensor}.  variant: "none" (canonical
    space), "nof_scalar" (IND_SCALAR for every point; ind ignored), "nof_tensor" (ind per point)."""
    import moco_flow_amd as M
    m = _models()
    with torch.no_grad():
        if variant == "none":
            return {"sigma_canonical": M.query_sigma(xyz.cuda(), m["nerf"], m["ex"], precision=prec)}
        sig, canon = M.query_sigma(xyz.cuda(), m["nerf"], m["ex"], bw_nof=m["nof"], nof_embeddings=m["nof_embs"],
                                   ind=IND_SCALAR if variant == "nof_scalar" else ind.cuda(), return_canonical=True, precision=prec)
    return {"canon": canon, "sigma_nof": sig}


def _rows(t, idx):
    """The rows of a launch's output the oracle evaluated."""
    return t.cpu()[idx]


_ORACLE = {}      # (arith, prec, variant is scalar) -> {output name: tensor} on subset(): shared by (a) and (b)


def _oracle(arith, prec, variant):
    scalar = variant == "nof_scalar"
    key = (arith, prec, scalar)
    if key not in _ORACLE:
        xyz, ind = _inputs(prec)
        idx = _subset(prec)
        sd_n, sd_f = P.states()
        canon, s_nof, s_can = P.point_query(arith, sd_n, sd_f, xyz[idx], torch.full((len(idx),), IND_SCALAR) if scalar else ind[idx])
        _ORACLE[key] = {"canon": canon, "sigma_nof": s_nof, "sigma_canonical": s_can}
    return _ORACLE[key]


def _subset(prec):
    return P.subset(second_trip(prec), P.TILE[prec], seed=P.TILE[prec])


# ---------------------------------------------------------------- (a) the fast mode against the oracle of its arithmetic
@pytest.mark.parametrize("variant", VARIANTS)
def test_fast_point_query_vs_the_oracle_of_its_arithmetic(B, variant):
    """query_sigma(precision="bf16") at the second-trip size against points_oracle.point_query(BF16) on subset(); the floor of
    each output comes from the oracle alone at the same points (the module docstring has the bars and the measured figures)."""
    xyz, ind = _inputs("bf16")
    idx = _subset("bf16")
    got = _launch("bf16", variant, xyz, ind)
    own, acc32, f32 = (_oracle(a, "bf16", variant) for a in (B.BF16, replace(B.BF16, acc="f32"), B.F32))
    wrong = {"canon": replace(B.BF16, nof_xyz="plain"), "sigma_nof": replace(B.BF16, nof_xyz="plain"),
             "sigma_canonical": replace(B.BF16, nerf_hidden="split")}
    fails = []
    for k, out in got.items():
        assert out.shape[0] == xyz.shape[0] and bool(torch.isfinite(out).all()), k
        g = _rows(out, idx)
        floor = B.l2rel(acc32[k], own[k])
        d_own, d_f32, d_wrong = B.l2rel(g, own[k]), B.l2rel(g, f32[k]), B.l2rel(g, _oracle(wrong[k], "bf16", variant)[k])
        print(f"fast {variant} {k}: {len(idx)} of {xyz.shape[0]} points, l2-rel to its own oracle {d_own:.2e} = {d_own / floor:.2f} floors "
              f"(floor {floor:.2e}); to the fp32 oracle {d_f32:.2e} = {d_f32 / floor:.1f}; to the wrong oracle {d_wrong:.2e} = {d_wrong / floor:.1f}")
        if not d_own <= 3.0 * floor:
            fails.append((k, "farther than 3 floors", d_own, floor))
        if not d_wrong >= 2.0 * d_own:
            fails.append((k, "the wrong oracle is not twice as far", d_wrong, d_own))
        if not d_own < d_f32:
            fails.append((k, "closer to the fp32 oracle", d_own, d_f32))
    assert not fails, fails


# ---------------------------------------------------------------- (b) f32 and bf16x3
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_point_query_fp32_contract(B, prec, variant):
    """1e-4 max-rel against cpu_ref on subset() of the second-trip launch; bf16x3 also against the oracle of its arithmetic.
    (bf16x3 with an index tensor: query_sigma runs the fp32 kernel -- the case is kept, held to the contract alone.)"""
    xyz, ind = _inputs(prec)
    idx = _subset(prec)
    got = _launch(prec, variant, xyz, ind)
    f32 = _oracle(B.F32, prec, variant)
    x3 = prec == "bf16x3" and variant != "nof_tensor"
    for k, out in got.items():
        assert out.shape[0] == xyz.shape[0]
        g = _rows(out, idx)
        e = relerr(g, f32[k])
        line = f"{prec} {variant} {k}: {len(idx)} of {xyz.shape[0]} points, max-rel to cpu_ref {e:.2e}"
        if x3:
            ps_own, ps_f32 = B.psnr_equiv(g, _oracle(B.BF16X3, prec, variant)[k]), B.psnr_equiv(g, f32[k])
            line += f"; PSNR-equiv to BF16X3 {ps_own:.1f} dB, to F32 {ps_f32:.1f} dB"
            if k != "canon":          # (the NeRF's hook: the canonical point is in front of it)
                ps_wrong = B.psnr_equiv(g, _oracle(replace(B.BF16X3, nerf_hidden="wsplit"), prec, variant)[k])
                line += f", hidden activations unsplit {ps_wrong:.1f} dB"
        print(line)
        assert e <= TOL, (k, e)
        if x3:
            assert ps_own >= ps_f32 - 1.0, (k, ps_own, ps_f32)
            if k != "canon":
                assert ps_wrong <= ps_own - 20.0, (k, ps_wrong, ps_own)


# ---------------------------------------------------------------- (c) per-point indices, bit for bit
@pytest.mark.parametrize("prec", ["bf16", "f32"])
def test_per_point_indices_equal_the_scalar_launches(M, prec):
    """On the points of each of the five index values, the per-point launch = the launch with that value as the scalar index."""
    xyz, ind = _inputs(prec)
    per_point = _launch(prec, "nof_tensor", xyz, ind)
    m = _models()
    seen = 0
    for v in P.IND_VALUES:
        with torch.no_grad():
            sig, canon = M.query_sigma(xyz.cuda(), m["nerf"], m["ex"], bw_nof=m["nof"], nof_embeddings=m["nof_embs"], ind=v,
                                       return_canonical=True, precision=prec)
        sel = (ind == v).cuda()
        seen += int(sel.sum())
        for k, out in (("sigma_nof", sig), ("canon", canon)):
            diff = int((out[sel] != per_point[k][sel]).sum())
            assert torch.equal(out[sel], per_point[k][sel]), (prec, v, k, diff)
        other = ~sel                  # (the bar can fail: with another point's index the flow differs)
        assert not torch.equal(canon[other], per_point["canon"][other])
    assert seen == xyz.shape[0]


# ---------------------------------------------------------------- (d) launch invariants, bit for bit
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("prec", ["f32", "bf16x3", "bf16"])
def test_point_query_launch_invariants_bit_exact(prec, variant):
    """Launches of 1, TILE - 1, TILE, TILE + 1 points = the prefix of the second-trip launch; three launches over an uneven
    split, concatenated, = that launch; so is its repeat.  One case is another kernel by the API's own rule: an index tensor
    of ONE element is the scalar index (query_sigma), so under "bf16x3" the 1-point launch with ind[:1] runs the bf16x3 kernel
    where the larger per-point launches run the fp32 one -- it is held to the scalar-index bf16x3 launch's first row."""
    xyz, ind = _inputs(prec)
    n = xyz.shape[0]
    ref = _launch(prec, variant, xyz, ind)

    def same(out, lo, hi, what, ref=ref):
        for k in ref:
            assert out[k].shape[0] == hi - lo, (what, k)
            assert torch.equal(out[k], ref[k][lo:hi]), (what, k, int((out[k] != ref[k][lo:hi]).sum()))

    for b in sizes(prec)[:-1]:
        if b == 1 and (prec, variant) == ("bf16x3", "nof_tensor"):
            assert float(ind[0]) == IND_SCALAR
            same(_launch(prec, variant, xyz[:b], ind[:b]), 0, b, "prefix 1 (one-element index tensor = scalar index)",
                 ref=_launch(prec, "nof_scalar", xyz, ind))
            continue
        same(_launch(prec, variant, xyz[:b], ind[:b]), 0, b, f"prefix {b}")
    a, b = _split_points(n)
    for lo, hi in ((0, a), (a, b), (b, n)):
        same(_launch(prec, variant, xyz[lo:hi], ind[lo:hi]), lo, hi, f"split {lo}:{hi}")
    same(_launch(prec, variant, xyz, ind), 0, n, "repeat")


# ---------------------------------------------------------------- (e) the NaN rule
def _poison(xyz, prec):
    """xyz with one NaN and one +inf point in the first tile and in the tile workgroup 0 takes on its second trip; -> (xyz, rows)."""
    bad = xyz.clone()
    second = cus() * P.TILE[prec]
    rows = [3, 70, second + 5, second + 101]
    for r, (col, v) in zip(rows, ((1, float("nan")), (2, float("inf")), (0, float("inf")), (2, float("nan")))):
        bad[r, col] = v
    return bad, rows


NAN_CASES = [("bf16", "none"), ("bf16", "nof_scalar"), ("bf16", "nof_tensor"), ("bf16x3", "none"), ("bf16x3", "nof_scalar")]


@pytest.mark.parametrize("prec,variant", NAN_CASES, ids=[f"{p}-{v}" for p, v in NAN_CASES])
def test_nan_or_inf_point_gives_nan_sigma_and_moves_no_other(prec, variant):
    """INTEGRATION.md, "bf16" / "bf16x3": "a NaN / inf ray or canonical point renders NaN" -- for points: the nanprop line of
    points_kernel_bf16.  ("f32": not documented, not asserted.)"""
    xyz, ind = _inputs(prec)
    clean = _launch(prec, variant, xyz, ind)
    bad_xyz, rows = _poison(xyz, prec)
    assert len(rows) == 4 and rows[-1] < xyz.shape[0] and bool(torch.isfinite(xyz).all())
    bad = _launch(prec, variant, bad_xyz, ind)
    sk = "sigma_canonical" if variant == "none" else "sigma_nof"
    assert bool(torch.isnan(bad[sk].cpu()[rows]).all()), bad[sk].cpu()[rows]
    keep = torch.ones(xyz.shape[0], dtype=torch.bool)
    keep[rows] = False
    keep = keep.cuda()
    for k in clean:
        assert torch.equal(bad[k][keep], clean[k][keep]), (k, int((bad[k][keep] != clean[k][keep]).sum()))


# ---------------------------------------------------------------- (f) the module forwards
FORWARDS = ("nerf_dir", "nerf_ind_sigma", "nof_quat", "nof_bare")


@functools.lru_cache(maxsize=None)
def _forward_case(name):
    """Module, oracle container, the embedded input rows of the large launch (host) and the call's keyword arguments."""
    import moco_flow_amd as M
    from moco_flow_amd import synth
    from oracle import cpu_ref as R
    n = second_trip("f32")
    g = torch.Generator().manual_seed(2000 + FORWARDS.index(name))
    xyz = torch.rand(n, 3, generator=g) * 3 - 1.5
    _, ind = P.inputs(n)
    sd_n, sd_f = P.states()
    if name == "nerf_dir":
        sd = synth.nerf_state(43, extra_feat_type="dir", extra_feat_dim=27, regime="dense", tag="fwd")
        dirs = torch.randn(n, 3, generator=g)
        dirs = dirs / dirs.norm(dim=1, keepdim=True)
        inp = torch.cat([R._embed_padded(R.Embedding(3, 10), xyz, 63), R.Embedding(3, 4)(dirs)], -1)
        return dict(mod=_load(M.NeRF(8, 256, 63, [4], "dir", 27), sd), ref=R.NeRF(8, 256, 63, [4], "dir", 27, state=sd), args=(inp,), kw={})
    if name == "nerf_ind_sigma":
        inp = R._embed_padded(R.Embedding(3, 10), xyz, 63)
        return dict(mod=_load(M.NeRF(8, 256, 63, [4], "ind", 5), sd_n), ref=R.NeRF(8, 256, 63, [4], "ind", 5, state=sd_n), args=(inp,),
                    kw=dict(sigma_only=True))
    if name == "nof_quat":
        inp = torch.cat([R._embed_padded(R.Embedding(3, 5), xyz, 33), R._embed_padded(R.Embedding(1, 16), ind[:, None], 33)], -1)
        return dict(mod=_load(M.NoF(4, 128, 33, [2], "ind", 33, True), sd_f), ref=R.NoF(4, 128, 33, [2], "ind", 33, True, state=sd_f),
                    args=(inp, xyz), kw={})
    sd = synth.nof_state(44, D=8, W=256, in_channels_xyz=33, skips=(4,), extra_feat_dim=0, use_quat=False, tag="fwd")
    inp = R._embed_padded(R.Embedding(3, 5), xyz, 33)        # the bare NoF() default: W = 256 (NK = 16), no index block
    return dict(mod=_load(M.NoF(), sd), ref=R.NoF(state=sd), args=(inp, xyz), kw={})


def _forward(c, lo, hi, grad=False):
    """The module call over rows lo:hi of the case's inputs; grad: with autograd on (parameters requiring grad: the dump kernels)."""
    args = [a[lo:hi].cuda() for a in c["args"]]
    with torch.set_grad_enabled(grad):
        out = c["mod"](*args, **c["kw"])
    assert out.requires_grad == grad
    return out.detach()


@pytest.mark.parametrize("name", FORWARDS)
def test_module_forward_past_the_first_trip(name):
    """NeRF.forward / NoF.forward at (#CUs + 1) x 128 + 1 rows against cpu_ref on subset(), 1e-4 max-rel; the same call with
    parameters requiring grad (mf_nerf_forward_dump / mf_nof_forward_dump) to the same bar.  The bare NoF() has no gradient
    path at its width (tests/test_gpu_shapes.py pins the NotImplementedError): no dump leg.  No backward at this size."""
    c = _forward_case(name)
    n = c["args"][0].shape[0]
    idx = P.subset(n, P.TILE["f32"], seed=FORWARDS.index(name))
    with torch.no_grad():
        want = c["ref"](*[a[idx] for a in c["args"]], **c["kw"])
    got = _forward(c, 0, n)
    assert got.shape == (n, want.shape[1]) and n == second_trip("f32")
    legs = [("no grad", got)]
    if name != "nof_bare":
        assert all(p.requires_grad for p in c["mod"].parameters())
        dumped = _forward(c, 0, n, grad=True)
        print(f"{name}: dump forward bit-equal to the no-grad forward: {torch.equal(dumped, got)}")
        legs.append(("dump", dumped))
    for leg, out in legs:
        g = _rows(out, idx)
        errs = [relerr(g, want)]
        if name.startswith("nof"):       # the flow's displacement: next to |xyz| ~ 1.5 the output alone hides the network
            errs.append(relerr(g - c["args"][1][idx], want - c["args"][1][idx]))
        if name == "nerf_dir":           # rgb in (0, 1) next to sigma of several units
            errs.append(relerr(g[:, :3], want[:, :3]))
        print(f"{name} [{leg}]: {len(idx)} of {n} rows, max-rel to cpu_ref " + " / ".join(f"{e:.2e}" for e in errs))
        assert max(errs) <= TOL, (leg, errs)


@pytest.mark.parametrize("grad", [False, True], ids=["nograd", "dump"])
@pytest.mark.parametrize("name", FORWARDS)
def test_module_forward_launch_invariants_bit_exact(name, grad):
    if grad and name == "nof_bare":
        with pytest.raises(NotImplementedError):          # (as pinned by tests/test_gpu_shapes.py: nothing to launch)
            _forward(_forward_case(name), 0, 1, grad=True)
        return
    c = _forward_case(name)
    n = c["args"][0].shape[0]
    ref = _forward(c, 0, n, grad)

    def same(lo, hi, what):
        out = _forward(c, lo, hi, grad)
        assert out.shape[0] == hi - lo, what
        assert torch.equal(out, ref[lo:hi]), (what, int((out != ref[lo:hi]).sum()))

    for b in sizes("f32")[:-1]:
        same(0, b, f"prefix {b}")
    a, b = _split_points(n)
    for lo, hi in ((0, a), (a, b), (b, n)):
        same(lo, hi, f"split {lo}:{hi}")
    same(0, n, "repeat")
