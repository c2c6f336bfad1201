"""The folded fp32 inference kernels' per-ray bias (-m gpu): extra_encoding's extra block -- the encoding of the ray's direction or
image index, the same for every sample of a ray -- is added to b' once per ray of a group (a table of G rows in LDS) and each
lane starts the layer's accumulators from its own ray's row, instead of multiplying the block per sample.

What can go wrong is the ROW a lane reads (tile and group edges, partial groups, a workgroup's second and third group) and the
table itself (columns, order, a stale stream after a weight change).  Everything sigma decides is held bit for bit to the
unfolded pass (MF_FOLD_FINAL=0, the in-tree stand-in for the behaviour before the fold), rgb to 1e-5 of it and to the oracle."""
import pytest
import torch

from cases import RENDER_CASES
from helpers import TOL, build_case, case_inputs, relerr, subset_rays, varied_indices

pytestmark = pytest.mark.gpu

KEYS = ("rgb_coarse", "depth_coarse", "opacity_coarse")
PLANES = ("weights_coarse", "alphas_coarse")
SEED = 0
# (n_rays, S): a tile holds samples of four rays, one of them split, and the last group is partial; a ray spans two tiles; 700
# groups of 6 rays, so that every workgroup takes a second and a third group
SHAPES = [(37, 40), (5, 192), (4200, 64)]


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


def _case(name, S, **over):
    c = dict(RENDER_CASES[name])
    c["S"] = S
    c.update(over)
    return c


def _rays(c, n):
    """synth's rays: every ray its own random unit direction; ray 1 gets a zero component, ray 2 an axis."""
    rays, bg = case_inputs(c, SEED, n=n)
    rays[1, 3:6] = torch.tensor([0.0, 0.6, 0.8])
    rays[2, 3:6] = torch.tensor([0.0, 0.0, 1.0])
    assert len({tuple(r) for r in rays[:, 3:6].tolist()}) == n
    return rays, bg


def _render(M, model, rays, bg, fold, **over):
    """(result, captured planes) of render_rays without gradients, FOLD_FINAL = fold."""
    from moco_flow_amd import rendering
    embs, nerfs, kw = model
    cap = {}
    rendering.FOLD_FINAL = fold
    try:
        with torch.no_grad():
            out = M.render_rays(rays, bg, embs, nerfs, _capture=cap, **dict(kw, **over))
    finally:
        rendering.FOLD_FINAL = True
    assert (nerfs[0]._packed_fold.buf is not None) or not fold          # the pass took the stream the switch asks for
    return out, cap


def _oracle(R, c, rays, bg, dtype=torch.float32, edit=None):
    """oracle.cpu_ref at `dtype` (tests/test_gpu_fold_final.py: float64 = the same function without arithmetic noise)."""
    embs, nerfs, kw = build_case(R, c, SEED)
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


def _same_but_rgb(on, cap_on, off, cap_off, label, keys=("depth_coarse", "opacity_coarse"), planes=PLANES):
    """sigma is read in front of extra_encoding: depth, opacity and the sample planes bit-identical, rgb by one accumulation order."""
    for k in keys:
        assert torch.equal(on[k], off[k]), (label, k)
    for k in planes:
        assert cap_on[k] is not None and torch.equal(cap_on[k], cap_off[k]), (label, k)


def _scale_extra_block(model, scale):
    nerf = model[1][0]
    with torch.no_grad():
        nerf.extra_encoding[0].weight[:, nerf.W:].mul_(scale)


_PAIR = {}     # (n, S, scale) -> the folded and the unfolded NeRF(dir) pass over _rays, shared by tests 1 and 2


def _dir_pair(M, n, S, scale):
    if (n, S, scale) not in _PAIR:
        c = _case("r_nerf_dir_dense", S)
        rays, bg = _rays(c, n)
        model = build_case(M, c, SEED, device="cuda")
        if scale != 1.0:
            _scale_extra_block(model, scale)
        on = _render(M, model, rays.cuda(), bg.cuda(), True)
        off = _render(M, model, rays.cuda(), bg.cuda(), False)
        _PAIR[n, S, scale] = (c, rays, bg, on, off)
    return _PAIR[n, S, scale]


def _group_edge_subset(n):
    """Oracle rays of a large batch: subset_rays' draw (first, last, between) plus the rays around the first group edges."""
    if n <= 256:
        return torch.arange(n)
    return torch.unique(torch.cat([subset_rays(n, 224, seed=1), torch.arange(32)]))


@pytest.mark.parametrize("n,S", SHAPES, ids=[f"n{n}-S{S}" for n, S in SHAPES])
def test_row_selection_across_tile_and_group_edges(M, R, n, S):
    """1. NeRF(dir/27), every ray its own direction: against the unfolded pass depth, opacity, weights and alphas bit for bit and
    rgb within 1e-5; against cpu_ref every output within helpers.TOL."""
    c, rays, bg, (on, cap_on), (off, cap_off) = _dir_pair(M, n, S, 1.0)
    _same_but_rgb(on, cap_on, off, cap_off, (n, S))
    e = relerr(on["rgb_coarse"], off["rgb_coarse"])
    print(f"\nn={n} S={S}: rgb, per-ray bias vs unfolded pass, max-rel {e:.2e}")
    assert e <= 1e-5, e
    idx = _group_edge_subset(n)
    want = _oracle(R, c, rays[idx], bg[idx])
    for k in KEYS:
        assert bool(torch.isfinite(on[k]).all()), k
        assert relerr(on[k].cpu()[idx], want[k]) <= TOL, (k, relerr(on[k].cpu()[idx], want[k]))


@pytest.mark.parametrize("n,S", SHAPES, ids=[f"n{n}-S{S}" for n, S in SHAPES])
def test_extra_block_x8_vs_float64_oracle(M, R, n, S):
    """2. W_e[:, W:] x 8, so that the extra block dominates extra_encoding's pre-activation and a wrong row cannot hide: rgb
    against the oracle in float64.  The yardstick is the unfolded pass's max-rel on the same inputs; the per-ray bias pass must
    stay within 3 x that (a max over two fp32 roundings of one function fluctuates by about 2 x).  Test 1's identities hold too.
    MEASURED on an MI355X, unfolded / per-ray bias: (37, 40) 2.45e-05 / 2.45e-05; (5, 192) 8.51e-07 / 8.51e-07; (4200, 64)
    2.74e-05 / 2.74e-05 (1.00 x each).  The build whose lanes all read the group's first row (-DMF_RAYBIAS_BREAK_ROW) fails this
    test and test 1 at every shape (rgb 8.1e-02 .. 3.1e-01 from the unfolded pass)."""
    c, rays, bg, (on, cap_on), (off, cap_off) = _dir_pair(M, n, S, 8.0)
    _same_but_rgb(on, cap_on, off, cap_off, (n, S, "x8"))
    assert relerr(on["rgb_coarse"], off["rgb_coarse"]) <= 1e-5
    idx = _group_edge_subset(n)

    def edit(p):
        w = p["extra_encoding.0.weight"].clone()
        w[:, 256:] *= 8.0
        p["extra_encoding.0.weight"] = w

    want = _oracle(R, c, rays[idx], bg[idx], torch.float64, edit)["rgb_coarse"]
    e_off = relerr(off["rgb_coarse"].cpu()[idx], want)
    e_on = relerr(on["rgb_coarse"].cpu()[idx], want)
    print(f"\nn={n} S={S}, extra block x 8: rgb max-rel to the float64 oracle: unfolded {e_off:.2e}, per-ray bias {e_on:.2e} "
          f"({e_on / e_off:.2f} x)")
    assert 0.0 < e_off <= TOL
    assert e_on <= 3.0 * e_off, (e_on, e_off)


@pytest.mark.parametrize("name", ["r_moco_local", "r_nerf_none_dense"])
def test_image_index_block_and_no_extra_block(M, R, name):
    """3. NeRF(ind/5) behind the NoF chains with a distinct image index per ray (the MoCo folded kernel), and a NeRF without an
    extra block (no table: every lane reads b'), at (37, 40): the assertions of test 1."""
    n, S = 37, 40
    c = _case(name, S)
    rays, bg = case_inputs(c, SEED, n=n)
    if c.get("nof", "none") != "none":
        rays = varied_indices(rays, seed=n)
        assert len(set(rays[:, 8].tolist())) == n
    model = build_case(M, c, SEED, device="cuda")
    on, cap_on = _render(M, model, rays.cuda(), bg.cuda(), True)
    off, cap_off = _render(M, model, rays.cuda(), bg.cuda(), False)
    _same_but_rgb(on, cap_on, off, cap_off, name)
    assert relerr(on["rgb_coarse"], off["rgb_coarse"]) <= 1e-5
    want = _oracle(R, c, rays, bg)
    for k in KEYS:
        assert relerr(on[k], want[k]) <= TOL, (k, relerr(on[k], want[k]))


def test_sigma_only_coarse_then_fine_pass(M):
    """4. test_time with 64 + 128 samples on 64 rays: the coarse pass is sigma-only (no table), the fine pass stages explicit
    depths.  Sample planes and opacities bit-identical to the unfolded run."""
    c = _case("r_nerf_dir_fine_test", 64)
    rays, bg = _rays(c, 64)
    m_on, m_off = build_case(M, c, SEED, device="cuda"), build_case(M, c, SEED, device="cuda")
    on, cap_on = _render(M, m_on, rays.cuda(), bg.cuda(), True)
    off, cap_off = _render(M, m_off, rays.cuda(), bg.cuda(), False)
    assert set(on) == set(off) and "rgb_coarse" not in on
    _same_but_rgb(on, cap_on, off, cap_off, "fine", keys=("opacity_coarse", "depth_fine", "opacity_fine"),
                  planes=("weights_coarse", "alphas_coarse", "z_fine", "weights_fine", "alphas_fine"))
    assert relerr(on["rgb_fine"], off["rgb_fine"]) <= 1e-5


def _noise(n, S):
    return 0.5 * torch.randn(n, S, generator=torch.Generator().manual_seed(3))


OPTIONS = {
    "bg-none": dict(bg=False),
    "disp-on": dict(over=dict(use_disp=True)),
    "disp-off": dict(over=dict(use_disp=False)),
    "z-vals": dict(over=dict(perturb=1.0), rng=lambda n, S: {"perturb_rand": torch.rand(n, S, generator=torch.Generator().manual_seed(2))}),
    "stride-10": dict(stride=10),
    "stride-20": dict(stride=20),
    "noise": dict(rng=lambda n, S: {"noise_coarse": _noise(n, S)}),
}


@pytest.mark.parametrize("opt", sorted(OPTIONS))
def test_optional_inputs_of_the_ray_rows(M, opt):
    """5. What a pass reads per ray beside the row's first nine columns, at (37, 40): no background, depths in disparity or not,
    explicit depths (the stratified jitter's), rows of 10 and of 20 floats (the entry point takes no row shorter than 9: the
    index column is the ninth), noise on sigma.  Bit-identical to the unfolded pass in everything but rgb."""
    n, S = 37, 40
    o = OPTIONS[opt]
    c = _case("r_nerf_dir_dense", S)
    rays, bg = _rays(c, n)
    rays, bg = rays.cuda(), (bg.cuda() if o.get("bg", True) else None)
    if "stride" in o:
        wide = torch.full((n, o["stride"]), float("nan"), device="cuda")
        wide[:, :9] = rays
        rays = wide[:, :10] if o["stride"] > 10 else torch.cat([rays, torch.full((n, 1), 0.5, device="cuda")], 1)
        assert rays.stride(0) == o["stride"]
    over = dict(o.get("over", {}))
    if "rng" in o:
        over["_rng"] = {k: v.cuda() for k, v in o["rng"](n, S).items()}
    model = build_case(M, c, SEED, device="cuda")
    on, cap_on = _render(M, model, rays, bg, True, **over)
    off, cap_off = _render(M, model, rays, bg, False, **over)
    _same_but_rgb(on, cap_on, off, cap_off, opt)
    assert bool(torch.isfinite(on["rgb_coarse"]).all())
    assert relerr(on["rgb_coarse"], off["rgb_coarse"]) <= 1e-5


def test_rows_shorter_than_nine_floats_are_refused(M):
    c = _case("r_nerf_dir_dense", 40)
    rays, bg = _rays(c, 37)
    with pytest.raises(RuntimeError, match="rays must be"):
        _render(M, build_case(M, c, SEED, device="cuda"), rays[:, :8].contiguous().cuda(), bg.cuda(), True)


def test_table_follows_the_extra_block_weights(M, R):
    """6. After an in-place change of extra_encoding's weight (an optimizer step's version bump) the next call is re-packed: rgb
    moves, equals a freshly constructed model carrying those weights bit for bit, and holds the contract against their oracle."""
    n, S = 37, 40
    c = _case("r_nerf_dir_dense", S)
    rays, bg = _rays(c, n)
    model = build_case(M, c, SEED, device="cuda")
    nerf = model[1][0]
    first, _ = _render(M, model, rays.cuda(), bg.cuda(), True)
    _scale_extra_block(model, -2.5)
    got, _ = _render(M, model, rays.cuda(), bg.cuda(), True)
    assert not torch.equal(got["rgb_coarse"], first["rgb_coarse"])
    for k in ("depth_coarse", "opacity_coarse"):
        assert torch.equal(got[k], first[k]), k
    fresh_model = build_case(M, c, SEED, device="cuda")
    fresh_model[1][0].load_state_dict({k: v.detach().clone() for k, v in nerf.state_dict().items()})
    fresh, _ = _render(M, fresh_model, rays.cuda(), bg.cuda(), True)
    sd = {k: v.detach().cpu() for k, v in nerf.state_dict().items()}

    def edit(p):
        for k in p:
            p[k] = sd[k].clone()

    want = _oracle(R, c, rays, bg, torch.float32, edit)
    for k in KEYS:
        assert torch.equal(got[k], fresh[k]), k
        assert relerr(got[k], want[k]) <= TOL, (k, relerr(got[k], want[k]))
