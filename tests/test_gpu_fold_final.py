"""fp32 inference passes over the folded stream (-m gpu): xyz_encoding_final pre-multiplied into extra_encoding by the packer
(mf_nerf_pack_fold, MF_F_FOLDED_FINAL, rendering.FOLD_FINAL).

What is held here: the fp32 contract against the oracle at the shapes where the panel program can go wrong; everything the fold
cannot touch (sigma and what follows from it) bit for bit against the unfolded pass; the fold's own arithmetic against the oracle
in float64 with the unfolded pass as the yardstick; the cache rules of the sixth PackedWeights; the training path untouched."""
import ctypes as C

import pytest
import torch

from cases import RENDER_CASES
from helpers import TOL, build_case, case_inputs, load_golden, relerr, subset_rays
from streams_util import HOLD_MS, hold, poison

pytestmark = pytest.mark.gpu

KEYS = ("rgb_coarse", "depth_coarse", "opacity_coarse")
S_MAX_F32 = 1356        # the largest S one group of the fp32 NeRF pass stages (tests/test_gpu_launch_shapes.py, S_MAX)


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


@pytest.fixture(autouse=True)
def _switches():
    from moco_flow_amd import rendering
    old = (rendering.FOLD_FINAL, rendering.STRICT_RNG, rendering.PRECISION)
    rendering.FOLD_FINAL, rendering.STRICT_RNG = True, False
    rendering.set_precision("f32")
    yield
    rendering.FOLD_FINAL, rendering.STRICT_RNG = old[0], old[1]
    rendering.set_precision(old[2])


def _seed(name):
    return int(load_golden(name)["meta_seed"])


def _render(M, model, rays, bg, fold=True, capture=None, **over):
    """render_rays without gradients, FOLD_FINAL = fold; the pass must have taken the stream the switch asks for."""
    from moco_flow_amd import rendering
    embs, nerfs, kw = model
    rendering.FOLD_FINAL = fold
    try:
        with torch.no_grad():
            out = M.render_rays(rays, bg, embs, nerfs, _capture=capture, **dict(kw, **over))
    finally:
        rendering.FOLD_FINAL = True
    assert (nerfs[0]._packed_fold.buf is not None) or not fold
    return out


def _oracle(R, c, seed, rays, bg, dtype=torch.float32, edit=None):
    """The CPU oracle at `dtype` (float64: the same function without arithmetic noise, as _oracle_grads of
    tests/test_gpu_parity.py evaluates it).  edit(nerf.p): changes to the weights before the conversion."""
    embs, nerfs, kw = build_case(R, c, seed)
    nets = list(nerfs) + (list(kw["nof_models"]) if kw["nof_models"] else [])
    if edit is not None:
        edit(nerfs[0].p)
    for m in nets:
        for k in m.p:
            m.p[k] = m.p[k].to(dtype)
    for e in list(embs) + list(kw["nof_embeddings"] or []):
        if e is not None:
            e.freq_bands = e.freq_bands.to(dtype)
    torch.set_default_dtype(dtype)
    try:
        with torch.no_grad():
            return R.render_rays(rays.to(dtype), bg.to(dtype) if bg is not None else None, embs, nerfs, **kw)
    finally:
        torch.set_default_dtype(torch.float32)


def _big_n():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return 2 * cus * min(64, S_MAX_F32 // 64) + 37


# (case, n rays or None = the fixture's): extra block dir / ind / none; half a tile (four waves without a sample); 3.5 tiles;
# S = 40; every workgroup owns >= 2 groups, so the stream wraps from the last folded panel to layer 0 across a composite
# phase; the bw -> NeRF -> fw stream jumps of a local chain; softplus
ORACLE_CASES = [("r_nerf_dir_dense", None), ("r_nerf_ind_dense", None), ("r_nerf_none_dense", None), ("r_nerf_dir_dense", 1),
                ("r_nerf_dir_dense", 7), ("r_nerf_dir_S40", None), ("r_nerf_dir_dense", "big"), ("r_moco_local", 48),
                ("r_nerf_dir_softplus", None)]


@pytest.mark.parametrize("name,n", ORACLE_CASES, ids=[f"{c}-n{n}" for c, n in ORACLE_CASES])
def test_folded_pass_vs_oracle(M, R, name, n):
    """rgb / depth / opacity of the folded fp32 pass within the project's contract (helpers.TOL, 1e-4 max-rel) of cpu_ref; the
    largest batch at a subset of its rays (per-ray outputs do not depend on the batch around them)."""
    c = dict(RENDER_CASES[name])
    seed = _seed(name)
    n = _big_n() if n == "big" else n
    rays, bg = case_inputs(c, seed, n=n)
    got = _render(M, build_case(M, c, seed, device="cuda"), rays.cuda(), bg.cuda() if bg is not None else None)
    idx = subset_rays(rays.shape[0], 256, seed=1)
    want = _oracle(R, c, seed, rays[idx], bg[idx] if bg is not None else None)
    errs = {k: relerr(got[k].cpu()[idx], want[k]) for k in KEYS}
    print(f"\n{name} n={rays.shape[0]}: folded pass vs cpu_ref, max-rel " + " / ".join(f"{e:.1e}" for e in errs.values()))
    for k in KEYS:
        assert got[k].shape[0] == rays.shape[0] and bool(torch.isfinite(got[k]).all()), k
        assert errs[k] <= TOL, (k, errs[k])


@pytest.mark.parametrize("name", ["r_nerf_dir_dense", "r_moco_local", "r_nerf_dir_S40"])
def test_fold_on_equals_fold_off_where_sigma_decides(M, name):
    """sigma never sees the folded layers: depth, opacity and the weights / alphas planes are bit-identical with the switch
    on and off; rgb differs only by the rounding of the folded weights."""
    c = dict(RENDER_CASES[name])
    seed = _seed(name)
    rays, bg = case_inputs(c, seed, device="cuda")
    model = build_case(M, c, seed, device="cuda")
    cap_on, cap_off = {}, {}
    on = _render(M, model, rays, bg, True, cap_on)
    off = _render(M, model, rays, bg, False, cap_off)
    assert model[1][0]._packed.buf is not None and model[1][0]._packed_fold.buf is not None      # one stream each
    for k in ("depth_coarse", "opacity_coarse"):
        assert torch.equal(on[k], off[k]), k
    for k in ("weights_coarse", "alphas_coarse"):
        assert cap_on[k] is not None and torch.equal(cap_on[k], cap_off[k]), k
    assert relerr(on["rgb_coarse"], off["rgb_coarse"]) <= 1e-5


def test_sigma_only_coarse_pass_is_bit_identical(M):
    """test_time with N_importance > 0: the coarse pass evaluates sigma only, over the folded stream's trunk panels -- the same
    bytes.  Every output of it, and with it the fine pass's depths, is bit-identical to the unfolded run; an inference-only
    model packs the folded stream alone."""
    name = "r_nerf_dir_fine_test"
    c = dict(RENDER_CASES[name])
    seed = _seed(name)
    rays, bg = case_inputs(c, seed, device="cuda")
    m_on, m_off = build_case(M, c, seed, device="cuda"), build_case(M, c, seed, device="cuda")
    cap_on, cap_off = {}, {}
    on = _render(M, m_on, rays, bg, True, cap_on)
    off = _render(M, m_off, rays, bg, False, cap_off)
    assert all(m._packed.buf is None and m._packed_fold.buf is not None for m in m_on[1])
    assert all(m._packed.buf is not None and m._packed_fold.buf is None for m in m_off[1])
    assert set(on) == set(off) and "rgb_coarse" not in on
    assert torch.equal(on["opacity_coarse"], off["opacity_coarse"])
    for k in ("weights_coarse", "alphas_coarse", "z_fine", "weights_fine", "alphas_fine"):
        assert torch.equal(cap_on[k], cap_off[k]), k
    for k in ("depth_fine", "opacity_fine"):
        assert torch.equal(on[k], off[k]), k
    assert relerr(on["rgb_fine"], off["rgb_fine"]) <= 1e-5


@pytest.mark.parametrize("bias_scale", [1.0, 8.0], ids=["dense", "final-bias-x8"])
def test_fold_arithmetic_vs_float64_oracle(M, R, bias_scale):
    """The sharp one for W' = W_e[:, :W] W_f and b' = b_e + W_e[:, :W] b_f: rgb against the oracle evaluated in float64.  The
    yardstick is the unfolded pass's max-rel to it (the parent's behaviour); the folded pass must stay within 3 x that -- a max
    over 3072 values of two different fp32 roundings of one function fluctuates by about 2 x.  The second draw scales
    xyz_encoding_final.bias by 8, so that a dropped W_e b_f term cannot hide.
    MEASURED on an MI355X (1024 rays x 64 of r_nerf_dir_dense): dense draw: unfolded 6.18e-06, folded 6.18e-06 (1.00 x); final
    bias x 8: unfolded 5.54e-06, folded 5.54e-06 (1.00 x) -- at this batch the distance is set by the fp32 sample positions in
    front of sin(512 x), which both passes share.  The build that drops W_e b_f (-DMF_FOLD_BREAK_BIAS) fails both draws:
    2.1e-02 and 1.7e-01."""
    name = "r_nerf_dir_dense"
    c = dict(RENDER_CASES[name])
    seed = _seed(name)
    rays, bg = case_inputs(c, seed, n=1024)
    model = build_case(M, c, seed, device="cuda")
    with torch.no_grad():
        model[1][0].xyz_encoding_final.bias.mul_(bias_scale)

    def edit(p):
        p["xyz_encoding_final.bias"] = p["xyz_encoding_final.bias"] * bias_scale

    want = _oracle(R, c, seed, rays, bg, torch.float64, edit)["rgb_coarse"]
    off = relerr(_render(M, model, rays.cuda(), bg.cuda(), False)["rgb_coarse"], want)
    on = relerr(_render(M, model, rays.cuda(), bg.cuda(), True)["rgb_coarse"], want)
    print(f"\nfinal bias x {bias_scale:g}: rgb max-rel to the float64 oracle: unfolded {off:.2e}, folded {on:.2e} ({on / off:.2f} x)")
    assert 0.0 < off <= TOL
    assert on <= 3.0 * off, (on, off)


def _fresh_like(M, c, seed, model):
    """A freshly constructed model carrying `model`'s weights."""
    fresh = build_case(M, c, seed, device="cuda")
    for a, b in zip(fresh[1], model[1]):
        a.load_state_dict({k: v.detach().clone() for k, v in b.state_dict().items()})
    return fresh


def _oracle_like(R, c, seed, model, rays, bg):
    sd = {k: v.detach().cpu() for k, v in model[1][0].state_dict().items()}

    def edit(p):
        for k in p:
            p[k] = sd[k].clone()

    return _oracle(R, c, seed, rays.cpu(), bg.cpu(), torch.float32, edit)


def test_folded_cache_follows_the_weights(M, R):
    """The folded stream is re-packed when xyz_encoding_final.weight or extra_encoding's bias alone changes in place (the
    version counter), and after a param.data edit plus invalidate_packed(): each render equals a freshly constructed model
    carrying those weights, bit for bit, and holds the contract against the oracle of those weights."""
    name = "r_nerf_dir_dense"
    c = dict(RENDER_CASES[name])
    seed = _seed(name)
    rays, bg = case_inputs(c, seed, device="cuda")
    model = build_case(M, c, seed, device="cuda")
    nerf = model[1][0]
    first = _render(M, model, rays, bg)

    def bump_final():
        with torch.no_grad():
            nerf.xyz_encoding_final.weight.mul_(1.25)

    def bump_extra_bias():
        with torch.no_grad():
            nerf.extra_encoding[0].bias.mul_(-3.0)

    def edit_data():
        nerf.xyz_encoding_final.bias.data.add_(0.5)
        nerf.invalidate_packed()

    last = first
    for what, change in (("final.weight", bump_final), ("extra.bias", bump_extra_bias), ("data + invalidate", edit_data)):
        change()
        got = _render(M, model, rays, bg)
        assert not torch.equal(got["rgb_coarse"], last["rgb_coarse"]), what
        fresh = _render(M, _fresh_like(M, c, seed, model), rays, bg)
        want = _oracle_like(R, c, seed, model, rays, bg)
        for k in KEYS:
            assert torch.equal(got[k], fresh[k]), (what, k)
            assert relerr(got[k], want[k]) <= TOL, (what, k, relerr(got[k], want[k]))
        last = got


def _train_step(M, model, rays, bg, gt):
    embs, nerfs, kw = model
    for m in nerfs:
        m.zero_grad(set_to_none=True)
    res = M.render_rays(rays, bg, embs, nerfs, **kw)
    ((res["rgb_coarse"] - gt) ** 2).mean().backward()
    return [res[k].detach().clone() for k in KEYS] + [p.grad.clone() for m in nerfs for p in m.parameters()]


def test_inference_interleaved_with_training(M):
    """Inference, one training step, inference: the two inference results are bit-identical, and the step's forward values
    and every gradient equal the same step with FOLD_FINAL off -- the training forward reads the unfolded stream either way."""
    from moco_flow_amd import rendering
    name = "r_nerf_dir_dense"
    c = dict(RENDER_CASES[name])
    seed = _seed(name)
    rays, bg = case_inputs(c, seed, device="cuda")
    gt = torch.rand(rays.shape[0], 3, generator=torch.Generator().manual_seed(1)).cuda()
    model, twin = build_case(M, c, seed, device="cuda"), build_case(M, c, seed, device="cuda")
    before = _render(M, model, rays, bg)
    step = _train_step(M, model, rays, bg, gt)
    after = _render(M, model, rays, bg)
    for k in KEYS:
        assert torch.equal(before[k], after[k]), k
    rendering.FOLD_FINAL = False
    try:
        step_off = _train_step(M, twin, rays, bg, gt)
    finally:
        rendering.FOLD_FINAL = True
    assert len(step) == len(step_off) and len(step) > 3 + 20
    for i, (a, b) in enumerate(zip(step, step_off)):
        assert torch.equal(a, b), i


def test_first_folded_call_on_a_side_stream(M):
    """The fold kernel and the pack run on the stream that builds the cache.  The first folded call of a fresh model is made on
    a side stream behind a hold, over memory last filled with 0xFF there; an immediate call on the default stream must wait for
    that build: both equal the serial result."""
    name = "r_nerf_dir_dense"
    c = dict(RENDER_CASES[name])
    seed = _seed(name)
    rays, bg = case_inputs(c, seed, device="cuda")
    serial = build_case(M, c, seed, device="cuda")
    want = _render(M, serial, rays, bg)
    torch.cuda.synchronize()
    nbytes = serial[1][0]._packed_fold.buf.numel()
    cold = build_case(M, c, seed, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        poison([nbytes])
        hold(side, HOLD_MS)
        a = _render(M, cold, rays, bg)
        built = torch.cuda.Event()
        built.record(side)
    b = _render(M, cold, rays, bg)
    delayed = built.query() is False
    torch.cuda.synchronize()
    assert delayed, "the build was not delayed: nothing shown"
    for k in KEYS:
        assert torch.equal(a[k], want[k]), ("side stream", k)
        assert torch.equal(b[k], want[k]), ("default stream", k, bool(torch.isnan(b[k]).any()))


def test_largest_shape_is_deterministic_across_repacks(M):
    """Three runs of the largest shape with a re-pack in between: bit-identical (the fold sums in a fixed order, no atomics)."""
    name = "r_nerf_dir_dense"
    c = dict(RENDER_CASES[name])
    seed = _seed(name)
    rays, bg = case_inputs(c, seed, n=_big_n(), device="cuda")
    model = build_case(M, c, seed, device="cuda")
    runs = []
    for _ in range(3):
        runs.append(_render(M, model, rays, bg))
        model[1][0].invalidate_packed()
        assert model[1][0]._packed_fold.buf is None
    for r in runs[1:]:
        for k in KEYS:
            assert torch.equal(r[k], runs[0][k]), k


def test_flag_refusals_launch_nothing(M):
    """MF_F_FOLDED_FINAL with bf16 / bf16x3: MF_E_UNSUPPORTED; with a dump pointer: MF_E_INVALID -- before anything is launched
    (the outputs keep their fill).  The same arguments in fp32 without a dump render."""
    L = M._lib
    name = "r_nerf_dir_dense"
    c = dict(RENDER_CASES[name])
    seed = _seed(name)
    rays, bg = case_inputs(c, seed, device="cuda")
    embs, nerfs, kw = build_case(M, c, seed, device="cuda")
    N, S = rays.shape[0], 64
    z_steps = torch.linspace(0, 1, S, device="cuda")
    desc, buf = nerfs[0].packed_fold()
    outs = {k: torch.full(shape, 7.0, device="cuda") for k, shape in (("rgb", (N, 3)), ("depth", (N,)), ("opacity", (N,)))}
    acts = torch.full((N * S, 9 * 256 + 128), 7.0, device="cuda")

    def call(precision, dump):
        a = L.mf_render_args()
        a.rays, a.ray_stride, a.n_rays = L.ptr(rays), rays.stride(0), N
        a.background, a.n_samples, a.z_steps = L.ptr(bg), S, L.ptr(z_steps)
        a.activation, a.flags, a.precision = L.MF_ACT_RELU, L.MF_F_FOLDED_FINAL, precision
        a.nerf, a.nerf_packed = C.pointer(desc), buf.data_ptr()
        a.emb_xyz, a.emb_extra = embs[0].descriptor(), embs[2].descriptor()
        a.rgb, a.depth, a.opacity = (outs[k].data_ptr() for k in ("rgb", "depth", "opacity"))
        if dump:
            a.dump_acts, a.dump_stride = acts.data_ptr(), acts.shape[1]
        rc = L.lib().mf_render_pass(C.byref(a), L.current_stream(rays.device))
        torch.cuda.synchronize()
        return rc

    untouched = lambda: all(bool((t == 7.0).all()) for t in list(outs.values()) + [acts])
    assert call(L.MF_PREC_BF16, False) == -3 and b"MF_F_FOLDED_FINAL" in L.lib().mf_last_error() and untouched()
    assert call(L.MF_PREC_BF16X3, False) == -3 and untouched()
    assert call(L.MF_PREC_F32, True) == -1 and b"dump" in L.lib().mf_last_error() and untouched()
    assert call(L.MF_PREC_F32, False) == 0
    want = _render(M, (embs, nerfs, kw), rays, bg)
    assert torch.equal(outs["rgb"], want["rgb_coarse"]) and torch.equal(outs["opacity"], want["opacity_coarse"])
    assert bool((acts == 7.0).all())
