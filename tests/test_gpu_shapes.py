"""GPU parity at the sizes and shapes the reference actually runs (-m gpu):
* BASELINE config C2 at full size (4096 rays x 64 samples, canonical NeRF dir/27, fp32) against the oracle;
* the reference's own training shapes -- the joint MoCo stage (configs/people_snapshot/male-3-casual/c2f.yaml:34-41,
  105-109: S = 128, M = 128, NeRF(ind/5), quaternion NoFs, local + global chains, perturb = 1.0) and stage 1
  (init_nerf.yaml:29-36: S = 128, M = 128, NeRF(dir/27), xyz N_freqs = 0, softplus, perturb = 1.0) -- on a ray slice
  the oracle finishes in seconds, in TRAINING mode (gradients recorded: the dumping kernels are the ones checked);
* the child-process legs (tests/preflight.py, started by conftest.py before this process touched the GPU): the 1-rank RCCL
  group (tests/rccl_child.py) and bench.py's real two-rank worker path.
Bars: 1e-4 max-rel (north_star) unless a comment says why not."""
import json
import os

import numpy as np
import pytest
import torch

from cases import RENDER_CASES
from helpers import build_case, relerr

pytestmark = pytest.mark.gpu

TOL = 1e-4


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


def test_c2_full_size_fp32_vs_oracle(M, R):
    """BASELINE config C2 (the headline workload of bench.py, its weight draw and its ray generator): every per-ray
    output of the one fused launch against the oracle at 4096 x 64, 1e-4 max-rel."""
    from moco_flow_amd import synth
    c = dict(RENDER_CASES["r_nerf_dir_dense"])
    tags = dict(coarse="nerf")
    rays_np, bg_np = synth.rays(0, 4096)
    rays, bg = torch.from_numpy(rays_np), torch.from_numpy(bg_np)
    embs_o, nerfs_o, kw_o = build_case(R, c, 0, tags=tags)
    embs, nerfs, kw = build_case(M, c, 0, device="cuda", tags=tags)
    cap = {}
    with torch.no_grad():
        res = M.render_rays(rays.cuda(), bg.cuda(), embs, nerfs, _capture=cap, **kw)
        cap_o = {}
        want = R.render_rays(rays, bg, embs_o, nerfs_o, _capture=cap_o, **kw_o)
    assert sorted(res) == sorted(want) == ["depth_coarse", "opacity_coarse", "rgb_coarse"]
    for k in want:
        assert res[k].shape == want[k].shape
        e = relerr(res[k], want[k])
        print(f"C2 full size {k}: max-rel {e:.2e}")
        assert e <= TOL, (k, e)
    for k in ("weights_coarse", "alphas_coarse"):
        assert relerr(cap[k], cap_o[k]) <= TOL, k
    # not a degenerate batch: a good share of the per-sample opacities lies strictly inside (0, 1)
    al = cap_o["alphas_coarse"]
    assert float(((al > 0.01) & (al < 0.99)).float().mean()) > 0.1


def _draws(n, S, Mi, seed=11):
    gen = torch.Generator().manual_seed(seed)
    return dict(perturb_rand=torch.rand(n, S, generator=gen), u=torch.rand(n, Mi, generator=gen))


def _with_grads(nets):
    for m in nets:
        for k in m.p:
            m.p[k] = m.p[k].clone().requires_grad_(True)


C2F = dict(n=256, S=128, M=128, extra="ind", regime="dense", nof="global")
STAGE1 = dict(n=256, S=128, M=128, extra="dir", regime="dense", act="softplus", xyz_freqs=0)


def test_c2f_training_shape_vs_oracle(M, R, wgrad):
    """Joint MoCo stage shape (c2f.yaml: 128 coarse + 128 importance samples, two NeRF(ind), bw / fw quaternion NoFs,
    local + global chains, perturb = 1.0) on 256 of its 1024 rays, in training mode: the values come from the DUMPING
    forward (`render_kernel<true, true>`), both passes.  The stratified jitter and the stochastic resample take
    injected draws; the fine pass is compared on the HIP path's own fine depths (rendering.py:323 detaches them)."""
    from moco_flow_amd import synth
    c = dict(C2F)
    n, S, Mi = c["n"], c["S"], c["M"]
    rays_np, bg_np = synth.rays(11, n, chained=True)
    rays, bg = torch.from_numpy(rays_np), torch.from_numpy(bg_np)
    rng = _draws(n, S, Mi)
    embs_o, nerfs_o, kw_o = build_case(R, c, 11)
    embs, nerfs, kw = build_case(M, c, 11, device="cuda")
    for k_ in (kw, kw_o):
        k_.update(perturb=1.0, noise_std=0.0)
    cap = {}
    res = M.render_rays(rays.cuda(), bg.cuda(), embs, nerfs, _rng={k: v.cuda() for k, v in rng.items()}, _capture=cap, **kw)
    assert res["rgb_fine"].requires_grad and res["nof_global_disp_fine"].requires_grad     # training graph attached
    assert cap["z_fine"].shape == (n, S + Mi)
    cap_o = {}
    with torch.no_grad():
        want = R.render_rays(rays, bg, embs_o, nerfs_o, _rng=rng, _z_fine_override=cap["z_fine"].cpu(), _capture=cap_o, **kw_o)
    assert list(res.keys()) == list(want.keys())
    assert relerr(cap["z_coarse"], cap_o["z_coarse"]) <= 1e-6
    # seed 11: neither pass is degenerate (mean opacity 0.46 coarse / 0.33 fine, masks neither empty nor full)
    assert 0.1 < float(want["opacity_coarse"].mean()) < 0.9 and 0.1 < float(want["opacity_fine"].mean()) < 0.9
    worst = 0.0
    for k, v in want.items():
        got = res[k].detach()
        if k.startswith("nof_"):
            # alpha >= 0.01 can flip for an alpha within an ulp of 0.01: lengths agree to a couple of entries
            assert abs(got.shape[0] - v.shape[0]) <= max(2, int(0.002 * v.shape[0])), (k, got.shape, v.shape)
            if got.shape[0] == v.shape[0]:
                e = relerr(got, v)
            else:
                e = abs(float(got.mean()) - float(v.mean())) / abs(float(v.mean()))
        else:
            assert got.shape == v.shape, k
            e = relerr(got, v)
        print(f"c2f shape (training forward) {k}: max-rel {e:.2e}")
        worst = max(worst, e)
        assert e <= TOL, (k, e)
    # the step is trainable end to end at this shape: every parameter of the five networks receives a finite gradient
    loss = M.get_loss(dict(type="MSE"))(res, torch.rand(n, 3, device="cuda"))
    for key in ("nof_local_disp", "nof_global_disp"):
        loss = loss + 0.2 * (res[key + "_coarse"].mean() + res[key + "_fine"].mean())
    loss.backward()
    for m in list(nerfs) + list(kw["nof_models"]):
        for name, p in m.named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name


def _oracle_stage1(R, c, seed, rays, bg, rng, gt, z_fine, dtype):
    """Oracle forward + autograd of the reference's loss at `dtype` (float64: the arithmetic-noise-free truth)."""
    embs_o, nerfs_o, kw_o = build_case(R, c, seed)
    kw_o.update(perturb=1.0, noise_std=0.0)
    for m in nerfs_o:
        for k in m.p:
            m.p[k] = m.p[k].to(dtype).clone().requires_grad_(True)
    for e in embs_o:
        if e is not None:
            e.freq_bands = e.freq_bands.to(dtype)
    torch.set_default_dtype(dtype)          # the oracle allocates its pads / ones with the default dtype
    try:
        want = R.render_rays(rays.to(dtype), bg.to(dtype), embs_o, nerfs_o, _rng={k: v.to(dtype) for k, v in rng.items()},
                             _z_fine_override=z_fine.to(dtype), **kw_o)
    finally:
        torch.set_default_dtype(torch.float32)
    loss = ((want["rgb_coarse"] - gt.to(dtype)) ** 2).mean() + ((want["rgb_fine"] - gt.to(dtype)) ** 2).mean()
    flat = [(i, k) for i, m in enumerate(nerfs_o) for k in m.p]
    grads = torch.autograd.grad(loss, [nerfs_o[i].p[k] for i, k in flat], allow_unused=True)
    return want, dict(zip(flat, grads))


def test_stage1_training_shape_vs_oracle(M, R, wgrad):
    """Stage 1 shape (init_nerf.yaml: 128 + 128 samples, NeRF(dir/27) with the xyz encoding at N_freqs = 0 zero-padded
    to 63 columns, softplus densities, perturb = 1.0) on 128 of its 5120 rays: training-mode forward 1e-4 against the
    oracle, and the END-TO-END gradients of the reference's loss (MSE coarse + fine, models/losses.py:4-14).
    Gradient bars.  A weight gradient here is a heavily cancelling sum over 49 152 samples behind eight ReLUs, and the
    REFERENCE's own fp32 arithmetic is only good to ~1e-4 on it: oracle fp32 vs float64 autograd differ by up to 4.3e-4
    max-rel / 1.3e-4 l2-rel per tensor at this shape (measured in the build container) -- single borderline samples
    whose ReLU mask flips between two fp32 evaluation orders move a row of dW by their whole contribution, so the
    max-rel figure is a discrete event, not rounding noise.  The truth is therefore the oracle in float64, and every
    HIP tensor must be within 3x the fp32 oracle's own l2 distance to it (floor 1e-4), with max-rel <= 2e-3 as the
    guard against a wrong element.  (What pins each backward kernel at 1e-4 is test_*_backward_vs_oracle*: the same
    function at the same points, masks included.)"""
    from moco_flow_amd import synth
    c = dict(STAGE1)
    n, S, Mi = 128, c["S"], c["M"]
    rays_np, bg_np = synth.rays(4, n)
    rays, bg = torch.from_numpy(rays_np), torch.from_numpy(bg_np)
    gt = torch.rand(n, 3, generator=torch.Generator().manual_seed(1))
    rng = _draws(n, S, Mi)
    embs, nerfs, kw = build_case(M, c, 4, device="cuda")
    assert embs[0].N_freqs == 0 and embs[0].out_channels == 3
    kw.update(perturb=1.0, noise_std=0.0)
    cap = {}
    res = M.render_rays(rays.cuda(), bg.cuda(), embs, nerfs, _rng={k: v.cuda() for k, v in rng.items()}, _capture=cap, **kw)
    M.get_loss(dict(type="MSE"))(res, gt.cuda()).backward()
    z_fine = cap["z_fine"].cpu()
    want, g32 = _oracle_stage1(R, c, 4, rays, bg, rng, gt, z_fine, torch.float32)
    _, g64 = _oracle_stage1(R, c, 4, rays, bg, rng, gt, z_fine, torch.float64)
    for k, v in want.items():
        e = relerr(res[k].detach(), v.detach())
        print(f"stage-1 shape (training forward) {k}: max-rel {e:.2e}")
        assert e <= TOL, (k, e)
    def l2rel(a, b):
        a, b = a.detach().cpu().double(), b.detach().double()
        return float((a - b).norm() / b.norm().clamp_min(1e-30))

    checked, worst, floor, worst_max = 0, (0.0, ""), (0.0, ""), (0.0, "")
    for key, g in g64.items():
        i, k = key
        p = dict(nerfs[i].named_parameters())[k]
        if g is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        noise = l2rel(g32[key], g)                      # the reference arithmetic's own error on this tensor
        e, emax = l2rel(p.grad, g), relerr(p.grad, g)
        worst, floor = max(worst, (e, f"{i}.{k}")), max(floor, (noise, f"{i}.{k}"))
        worst_max = max(worst_max, (emax, f"{i}.{k}"))
        assert e <= max(TOL, 3 * noise), (i, k, e, noise)
        assert emax <= 2e-3, (i, k, emax)
        checked += 1
    print(f"stage-1 shape: end-to-end gradients vs the float64 oracle, worst l2-rel {worst[0]:.2e} at {worst[1]}, worst max-rel "
          f"{worst_max[0]:.2e} at {worst_max[1]} (fp32 oracle's own worst l2-rel {floor[0]:.2e} at {floor[1]}; {checked} tensors)")
    assert checked == 2 * 24


def _preflight_log(preflight, name):
    assert preflight, "conftest.py did not start tests/preflight.py (MF_NO_PREFLIGHT set?)"
    log = open(os.path.join(preflight["dir"], name + ".log")).read()
    print(log[-3000:])
    assert preflight["status"].get(name) == 0, (preflight["status"], log[-3000:])
    return log


def test_rccl_one_rank_child(preflight):
    """BASELINE config C4's collective leg on one GPU (trainer/base.py:104-106): tests/rccl_child.py -- a 1-rank "nccl"
    (RCCL) process group, 50 MoCo bf16 steps whose loss partials go through OverlappedLossReducer's real all-reduce Work
    objects under torch's sync-debug "error" mode -- was run by tests/preflight.py before this process touched the GPU."""
    log = _preflight_log(preflight, "rccl")
    line = [ln for ln in log.splitlines() if ln.startswith("{")][-1]
    out = json.loads(line)
    assert out["ok"] and out["backend"] == "nccl" and out["world"] == 1
    assert out["steps"] == 50 and out["mismatching_steps"] == 0
    assert all("Done" not in t for t in out["work_types"]), out["work_types"]
    # round 5, the training half of SURVEY 8(e): ten joint steps' flat gradient (four buckets, 5.3 MB) through
    # dist.GradReducer's ncclAllReduce from the post-accumulate hooks, bit-identical to the un-reduced gradients
    assert out["grad_steps"] == 10 and out["grad_buckets"] == 4 and out["grad_mismatching_tensors"] == 0
    assert out["grad_collectives"] == 11 * 4 and out["grad_flat_bytes"] > 5_000_000


def test_bench_two_ranks_real_worker_path(preflight):
    """`python bench.py --gpus 2 --steps 3 --warmup 1 --full` -- bench.py's REAL world > 1 worker path (self-spawned ranks, 127.0.0.1
    rendezvous, the sharded main line WITH its loss all-reduce, C2 / C4 / C5 legs, MAX-over-ranks timing, one compact JSON
    line from rank 0 + the detail on stderr) -- with both ranks on GPU 0 and gloo as the backend (MF_BENCH_SHARE_GPU /
    MF_BENCH_BACKEND: what one GPU can execute; RCCL itself is the other child's subject)."""
    log = _preflight_log(preflight, "bench2")
    lines = [ln for ln in log.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines
    assert len(lines[0].encode()) <= 1800
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["warmup"] == 1 and d["scaling"] == "weak"
    assert d["config"]["global_rays"] == 8192 and d["config"]["rays_per_gpu"] == 4096 and d["config"]["sharding"] == "rays2"
    # round 6: the N > 1 main line is the workload north_star describes -- the rank's 4096 x 64 fp32 batch + the all-reduce of
    # its loss partials inside the step -- and the ranks the all-reduce reached are on the line
    assert d["config"]["loss_allreduce"] is True and d["config"]["main_has_collective"] is True and d["dtype"] == "f32"
    assert d["rccl_ranks_seen"] == 2
    assert np.isfinite(d["value"]) and d["value"] > 0 and np.isfinite(d["ms_per_step"])
    assert 0 < d["roofline"]["frac"] < 1 and d["roofline"]["bound"] == "mfma"
    assert set(d["legs"]) == {"C2", "C4", "C5"} and d["leg_fields"][0] == "ms"
    assert all(np.isfinite(v[0]) and v[0] > 0 for v in d["legs"].values())
    assert np.isfinite(d["train_dp_ms"]["local"]) and d["train_dp_ms"]["allreduce"] > 0
    det = [ln for ln in log.splitlines() if ln.startswith("bench_detail {")]
    assert len(det) == 1
    full = json.loads(det[0][len("bench_detail "):])
    assert full["configs"]["C2"]["config"]["loss_allreduce"] is False           # the headline without its collective: a leg
    for name in ("C4", "C5"):
        leg = full["configs"][name]
        assert leg["config"]["loss_allreduce"] is True and leg["config"]["sharding"] == "rays2", name
        assert np.isfinite(leg["value"]) and leg["value"] > 0 and 0 < leg["roofline"]["frac"] < 1, name
    # round 5: the data-parallel TRAINING leg -- the joint step per rank with the global loss (dist.global_partials) and the
    # four per-network gradient buckets all-reduced from the backward's hooks (dist.GradReducer); both ranks ran it
    dp = full["train_joint_dp"]
    assert dp["world"] == 2 and dp["buckets"] == 4 and dp["flat_gradient_bytes"] > 5_000_000
    assert np.isfinite(dp["ms_per_step_local"]) and np.isfinite(dp["ms_per_step_allreduce"]) and dp["ms_per_step_allreduce"] > 0


def test_bench_json_line_is_last_on_stdout_under_rccl(preflight):
    """Round 6: RCCL prints a five-line version banner through C stdio to STDOUT when its first communicator comes up; in a pipe that
    text sits in libc's buffer until exit and used to land BEHIND the JSON line (visible in rccl_child's log) -- a driver parsing the
    last stdout line of an N > 1 run would have read "Librccl path : ...".  bench.py now flushes libc's streams once the communicator
    exists and prints only after the group is down.  Checked on the real thing: bench.py under a 1-rank "nccl" group
    (MF_BENCH_FORCE_DIST), stdout alone in a file."""
    assert preflight, "conftest.py did not start tests/preflight.py (MF_NO_PREFLIGHT set?)"
    assert preflight["status"].get("bench1d") == 0, (preflight["status"], open(os.path.join(preflight["dir"], "bench1d.log")).read()[-3000:])
    out = open(os.path.join(preflight["dir"], "bench1d.out")).read()
    lines = [ln for ln in out.splitlines() if ln.strip()]
    print(out[-2500:])
    d = json.loads(lines[-1])                                  # the LAST non-empty stdout line is the compact object
    assert len(lines[-1].encode()) <= 1800 and d["n_gpus"] == 1 and d["rccl_ranks_seen"] == 1 and d["value"] > 0
    assert any("RCCL version" in ln for ln in lines[:-1]), "expected RCCL's banner in front of the JSON line (did the runtime stop printing it?)"


def test_bench_dump_outputs_are_the_c2_render(preflight, M, R):
    """`bench.py --dump-outputs DIR` (the same tests/preflight.py run as above): DIR holds what the last timed C2 step returned --
    one float32 .npy per key of the result dict -- and that is the C2 batch (seeded rays, the "nerf" weight draw) rendered
    here by the same library, and within 1e-4 max-rel of the oracle."""
    from moco_flow_amd import synth
    assert preflight and preflight["status"].get("bench1d") == 0, preflight.get("status")
    d = os.path.join(preflight["dir"], "dump")
    got = {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}
    assert sorted(got) == ["depth_coarse", "opacity_coarse", "rgb_coarse"], sorted(got)
    c = dict(RENDER_CASES["r_nerf_dir_dense"])
    tags = dict(coarse="nerf")
    rays_np, bg_np = synth.rays(0, 4096)
    embs, nerfs, kw = build_case(M, c, 0, device="cuda", tags=tags)
    embs_o, nerfs_o, kw_o = build_case(R, c, 0, tags=tags)
    with torch.no_grad():
        res = M.render_rays(torch.from_numpy(rays_np).cuda(), torch.from_numpy(bg_np).cuda(), embs, nerfs, **kw)
        want = R.render_rays(torch.from_numpy(rays_np), torch.from_numpy(bg_np), embs_o, nerfs_o, **kw_o)
    for k, a in got.items():
        assert a.dtype == np.float32 and a.shape == tuple(res[k].shape), (k, a.dtype, a.shape)
        same, e = relerr(a, res[k]), relerr(a, want[k])
        print(f"bench dump {k}: max-rel {same:.2e} vs this process' render, {e:.2e} vs the oracle")
        assert same <= 1e-6 and e <= TOL, (k, same, e)


def test_lazy_consensus_vectors(M):
    """The consensus vectors as lazy.MaskedVector (moco_flow_amd/lazy.py): what the unchanged trainer does with them --
    torch.mean(res["nof_local_disp_coarse"]) (trainer_moco_flow.py:317-328) -- involves no compaction and NO host
    synchronisation (torch's sync-debug mode set to "error" around render + means); the means equal those of the
    materialised tensors; materialising gives exactly the eager path's tensors; and in training both routes
    back-propagate the same gradients."""
    from moco_flow_amd import rendering, synth
    from moco_flow_amd.lazy import MaskedVector
    c = dict(RENDER_CASES["r_moco_global_fine"])
    embs, nerfs, kw = build_case(M, c, 5, device="cuda")
    rays_np, bg_np = synth.rays(5, 192, chained=True)
    rays, bg = torch.from_numpy(rays_np).cuda(), torch.from_numpy(bg_np).cuda()
    keys = [f"nof_{a}_disp_{b}" for b in ("coarse", "fine") for a in ("local", "global")]
    strict = rendering.STRICT_RNG
    try:
        rendering.STRICT_RNG = False
        for prec in ("f32", "bf16"):
            rendering.set_precision(prec)
            with torch.no_grad():
                M.render_rays(rays, bg, embs, nerfs, **kw)                    # warm-up: packing, module load, allocator
                torch.cuda.synchronize()
                torch.cuda.set_sync_debug_mode("error")
                try:
                    res = M.render_rays(rays, bg, embs, nerfs, **kw)
                    # the unchanged trainer: forward() concatenates its ray chunks' result dicts -- `torch.cat(v, 0)`,
                    # trainer_moco_flow.py:199-223 -- before _shared_step takes the means (:317-328), adding in place
                    wrapped = {k: torch.cat([res[k]], 0) for k in keys}
                    means = {k: torch.mean(wrapped[k]) for k in keys}
                    acc = torch.mean(wrapped[keys[0]])
                    acc += torch.mean(wrapped[keys[2]])
                    sums = {k: res[k].sum() for k in keys}
                    again = torch.mean(wrapped[keys[0]])
                finally:
                    torch.cuda.set_sync_debug_mode("default")
                assert all(isinstance(res[k], MaskedVector) and isinstance(wrapped[k], MaskedVector) for k in keys)
                assert float(again) == float(means[keys[0]])             # the in-place += did not reach the cached mean
                assert float(acc) == pytest.approx(float(means[keys[0]]) + float(means[keys[2]]), rel=1e-6)
                # two ray chunks through the same wrapper: the mean of the concatenation
                h = rays.shape[0] // 2
                parts = [M.render_rays(rays[:h], bg[:h], embs, nerfs, **kw), M.render_rays(rays[h:], bg[h:], embs, nerfs, **kw)]
                for k in keys:
                    cat = torch.cat([q[k] for q in parts], 0)
                    assert isinstance(cat, MaskedVector)
                    whole = res[k].materialize()
                    assert float(torch.mean(cat)) == pytest.approx(float(whole.mean()), rel=2e-6), k
                    assert torch.equal(cat.materialize(), whole), k
                rendering.LAZY_CONSENSUS = False
                eager = M.render_rays(rays, bg, embs, nerfs, **kw)
                rendering.LAZY_CONSENSUS = True
            for k in keys:
                assert torch.is_tensor(eager[k]) and torch.equal(res[k].materialize(), eager[k]), k
                assert res[k].shape == eager[k].shape and len(res[k]) == eager[k].shape[0]
                assert abs(float(means[k]) - float(eager[k].mean())) <= 1e-5 * abs(float(eager[k].mean())), k
                assert abs(float(sums[k]) - float(eager[k].sum())) <= 1e-5 * abs(float(eager[k].sum())), k
            for k in res:                                                    # the per-ray outputs are untouched
                if k not in keys:
                    assert torch.equal(res[k], eager[k]), k
    finally:
        rendering.set_precision("f32")
        rendering.STRICT_RNG, rendering.LAZY_CONSENSUS = strict, True
    # training: loss through the lazy means vs through the materialised vectors
    nets = list(nerfs) + list(kw["nof_models"])
    gt = torch.rand(192, 3, device="cuda")

    def grads(materialise):
        for m in nets:
            m.zero_grad(set_to_none=True)
        res = M.render_rays(rays, bg, embs, nerfs, **kw)
        loss = M.get_loss(dict(type="MSE"))(res, gt)
        for k in keys:
            v = res[k].materialize() if materialise else res[k]
            loss = loss + 0.2 * torch.mean(v)
        loss.backward()
        return float(loss), [p.grad.clone() for m in nets for p in m.parameters()]

    la, ga = grads(False)
    lb, gb = grads(True)
    assert la == pytest.approx(lb, rel=1e-6)
    for x, y in zip(ga, gb):
        assert relerr(x, y) <= 1e-5
    # the eager opt-out in TRAINING with the global chain (c2f.yaml's configuration; ADVICE r3: KeyError 'global')
    try:
        rendering.LAZY_CONSENSUS = False
        lc, gc = grads(False)
    finally:
        rendering.LAZY_CONSENSUS = True
    assert lc == pytest.approx(lb, rel=1e-6)
    for x, y in zip(gc, gb):
        assert relerr(x, y) <= 1e-5


def l2rel(a, b):
    a, b = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _twin_state(m):
    return {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}


def test_reference_constructor_defaults(M, R):
    """The envelope is the reference's constructors, not only its three YAMLs: `NeRF()` -- D = 8, W = 256,
    in_channels_xyz = 33, skips = [4], no extra block (models/nerf.py:6-12) -- renders in every arithmetic and back-propagates;
    `NoF(D=4, W=128)` with the remaining defaults -- in_channels_xyz = 33, skips = [4] (none inside D = 4), extra_feat_dim = 0,
    flow head (models/nof.py:7-15) -- evaluates as a module; a NoF with narrower input blocks (21 + 17 columns: 3 xyz and 8
    index frequencies) runs the MoCo chains; an embedding wider than its block raises like the reference's padding does."""
    from moco_flow_amd import rendering, synth
    from test_gpu_parity import _check_grads_vs_float64, _oracle_grads  # noqa: F401  (same yardstick as the gradient tests)
    torch.manual_seed(3)
    n, S = 96, 64
    rays_np, bg_np = synth.rays(3, n)
    rays, bg = torch.from_numpy(rays_np), torch.from_numpy(bg_np)
    nerf = M.NeRF()
    assert (nerf.D, nerf.W, nerf.in_channels_xyz, nerf.skips, nerf.extra_feat_type, nerf.extra_feat_dim) == (8, 256, 33, [4], "none", 0)
    # the "dense" weight regime of the fixtures (mid-range opacities, so that the composite is exercised) at these widths
    nerf.load_state_dict({k: torch.from_numpy(v) for k, v in synth.nerf_state(3, in_channels_xyz=33, extra_feat_type="none",
                                                                                extra_feat_dim=0, regime="dense", tag="ctor").items()})
    nerf = nerf.cuda()
    sd = _twin_state(nerf)
    embs, oembs = [M.Embedding(3, 5), None, None], [R.Embedding(3, 5), None, None]
    onerf = R.NeRF(state=sd)
    kw = dict(N_samples=S, noise_std=0)
    cap_o = {}
    with torch.no_grad():
        want = R.render_rays(rays, bg, oembs, [onerf], _capture=cap_o, **kw)
    al = cap_o["alphas_coarse"]                             # not a degenerate batch: per-sample opacities inside (0, 1)
    assert float(((al > 0.01) & (al < 0.99)).float().mean()) > 0.1
    for prec, bar in (("f32", TOL), ("bf16x3", TOL), ("bf16", None)):
        try:
            rendering.set_precision(prec)
            with torch.no_grad():
                got = M.render_rays(rays.cuda(), bg.cuda(), embs, [nerf], **kw)
        finally:
            rendering.set_precision("f32")
        for k in want:
            e = relerr(got[k], want[k]) if bar is not None else l2rel(got[k], want[k])
            print(f"NeRF() defaults [{prec}] {k}: {'max-rel' if bar is not None else 'l2-rel'} {e:.2e}")
            assert e <= (bar if bar is not None else 1e-2), (prec, k, e)         # (fast bf16: a structural screen)
    # training step through the HIP backward: float64 oracle as truth, per-tensor noise floors (test_gpu_parity's yardstick)
    gt = torch.rand(n, 3, generator=torch.Generator().manual_seed(0))
    res = M.render_rays(rays.cuda(), bg.cuda(), embs, [nerf], **kw)
    (((res["rgb_coarse"] - gt.cuda()) ** 2).mean() + 0.1 * res["depth_coarse"].mean()).backward()

    def oracle_grads(dtype):
        o = R.NeRF(state=sd)
        for k in o.p:
            o.p[k] = o.p[k].to(dtype).clone().requires_grad_(True)
        e = R.Embedding(3, 5)
        e.freq_bands = e.freq_bands.to(dtype)
        torch.set_default_dtype(dtype)
        try:
            r = R.render_rays(rays.to(dtype), bg.to(dtype), [e, None, None], [o], **kw)
            loss = ((r["rgb_coarse"] - gt.to(dtype)) ** 2).mean() + 0.1 * r["depth_coarse"].mean()
        finally:
            torch.set_default_dtype(torch.float32)
        names = list(o.p)
        return {f"0.{k}": g for k, g in zip(names, torch.autograd.grad(loss, [o.p[k] for k in names]))}

    # (no fixed fp32 bar at this size: one ReLU unit of 6144 samples changing side between the two fp32 evaluation orders moves
    #  a first-layer row by 1.6e-4 -- measured -- where the fp32 oracle itself sits 7e-5 from the float64 truth)
    assert _check_grads_vs_float64([nerf], oracle_grads(torch.float32), oracle_grads(torch.float64), label="NeRF() defaults") == 24
    # module-level calls on pre-embedded rows (trainer_moco_flow.py:146-157)
    x = torch.randn(1000, 33)
    with torch.no_grad():
        assert relerr(nerf(x.cuda()), onerf(x)) <= TOL and relerr(nerf(x.cuda(), sigma_only=True), onerf(x, sigma_only=True)) <= TOL

    nof = M.NoF(D=4, W=128)
    assert (nof.in_channels_xyz, nof.skips, nof.extra_feat_type, nof.extra_feat_dim, nof.use_quat) == (33, [4], "ind", 0, False)
    nof = nof.cuda()
    onof = R.NoF(4, 128, 33, [4], "ind", 0, False, state=_twin_state(nof))
    pts = torch.randn(1000, 3)
    inp = R.Embedding(3, 5)(pts)
    with torch.no_grad():
        e = relerr(nof(inp.cuda(), pts.cuda()), onof(inp, pts))
    print(f"NoF(D=4, W=128) defaults, module call: max-rel {e:.2e}")
    assert e <= TOL

    # the reference's BARE constructor default (models/nof.py:7-15): D = 8, W = 256, skips = [4], 33 input columns, flow head -- the
    # module-level forward (nof_forward_kernel<16>, round 5); the fused passes and the HIP backward stay at W = 128 and say so
    nof0 = M.NoF()
    assert (nof0.D, nof0.W, nof0.in_channels_xyz, nof0.skips, nof0.extra_feat_type, nof0.extra_feat_dim, nof0.use_quat) == (8, 256, 33, [4], "ind", 0, False)
    nof0 = nof0.cuda()
    onof0 = R.NoF(state=_twin_state(nof0))
    with torch.no_grad():
        e = relerr(nof0(inp.cuda(), pts.cuda()), onof0(inp, pts))
    print(f"NoF() bare defaults (D=8, W=256), module call: max-rel {e:.2e}")
    assert e <= TOL
    with pytest.raises((NotImplementedError, RuntimeError)):                    # a render pass with it: refused loudly
        M.render_rays(rays.cuda(), bg.cuda(), embs, [nerf], nof_embeddings=[M.Embedding(3, 5), M.Embedding(1, 16)], nof_models=[nof0], **kw)
    with pytest.raises(NotImplementedError):                                    # gradients of the module call: not built at this width
        nof0(inp.cuda(), pts.cuda())

    # narrower NoF input blocks through the consensus chains, every arithmetic
    nofs = [M.NoF(4, 128, 21, [2], "ind", 17, True).cuda() for _ in range(2)]
    with torch.no_grad():
        for m in nofs:
            m.nof_encoding_final.weight.mul_(0.25)
    onofs = [R.NoF(4, 128, 21, [2], "ind", 17, True, state=_twin_state(m)) for m in nofs]
    rays10 = torch.from_numpy(synth.rays(3, n, chained=True)[0])
    kw2 = dict(N_samples=S, noise_std=0, chain_local=True, chain_global=True)
    with torch.no_grad():
        want = R.render_rays(rays10, bg, oembs, [onerf], nof_embeddings=[R.Embedding(3, 3), R.Embedding(1, 8)], nof_models=onofs, **kw2)
    for prec, bar in (("f32", TOL), ("bf16x3", TOL), ("bf16", None)):
        try:
            rendering.set_precision(prec)
            with torch.no_grad():
                got = M.render_rays(rays10.cuda(), bg.cuda(), embs, [nerf], nof_embeddings=[M.Embedding(3, 3), M.Embedding(1, 8)],
                                    nof_models=nofs, **kw2)
        finally:
            rendering.set_precision("f32")
        assert list(got) == list(want)
        for k in want:
            if k.startswith("nof_"):
                e = abs(float(torch.mean(got[k])) - float(want[k].mean())) / abs(float(want[k].mean()))
            else:
                e = relerr(got[k], want[k]) if bar is not None else l2rel(got[k], want[k])
            print(f"NoF(21 + 17 columns) chains [{prec}] {k}: {e:.2e}")
            assert e <= (bar if bar is not None else 1e-1), (prec, k, e)
    # wider than the block: the reference's zero-padding assignment fails (rendering.py:127-129), so does this
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="wider"):
            M.render_rays(rays.cuda(), bg.cuda(), [M.Embedding(3, 10), None, None], [nerf], **kw)
        with pytest.raises(RuntimeError, match="NoF takes"):
            M.render_rays(rays10.cuda(), bg.cuda(), embs, [nerf], nof_embeddings=[M.Embedding(3, 3), M.Embedding(1, 16)], nof_models=nofs, **kw2)
    # (the NoF BACKWARD is built for 33 + 33 input columns: training through narrower blocks raises, no eager fallback)
    with pytest.raises(NotImplementedError, match="NoF backward"):
        M.render_rays(rays10.cuda(), bg.cuda(), embs, [nerf], nof_embeddings=[M.Embedding(3, 3), M.Embedding(1, 8)], nof_models=nofs, **kw2)
