"""Streams and threads (-m gpu): every op gives its serial result when it runs on a side stream, behind a delayed producer, or
from two threads.  The reference of every comparison is the SAME op run on the default stream and synchronised -- the existing
suite holds those serial results to the oracles -- so every comparison is torch.equal, bit for bit; there is no tolerance here.

  (1) streams_util.hold(stream, ms): a spin kernel of a calibrated length (torch.cuda._sleep) in front of a producer.  A test that
      relies on it records an event behind the producer and, once the consumer has been ENQUEUED, asserts that the event is not
      done: a test whose producer had already finished fails with "producer was not delayed", it never passes vacuously.
  (2) hidden caches (packing.PackedWeights x 5 per network, rendering._LINSPACE, SMPL._model): built on stream A behind a hold,
      consumed on stream B; A and B wait for the default stream and never for each other.  The cold cache's memory is a block
      that was filled with 0xFF on A just before, so a consumer that is not ordered behind the build reads NaN.  Then the weights
      are bumped and the pattern runs again with A and B swapped (the re-pack an optimizer step causes).
  (3) every public op on a held stream B: its input is NaN until a copy ON B behind the hold fills it, and the memory its outputs
      get was last written by a 0xFF fill on B behind the hold: a launch or a temporary on another stream reads NaN, or is
      overwritten.  With gradients: forward and .backward() under B (the engine runs the backward nodes on the forward's stream).
  (4) two threads, a stream each, over shared and over distinct modules; mf_last_error per thread.

The serial run comes first and its modules stay alive: every code object is loaded before a held run, and the allocator cannot
hand a cold cache a freed block that still holds the right bytes.

Two streams may share a hardware queue, and the device then runs one behind the other whatever the program says: an unordered
consumer would look ordered.  The fixture takes streams that were seen to run concurrently with each other and with the default
stream (streams_util.independent_streams), and every held test also asserts that a marker on the consumer's stream (in section
3: on the default stream) completed while the producer was still held.

MEASURED on an MI355X: torch.cuda._sleep counts 2.36e6 ticks per ms (two runs: 2.366e6, 2.359e6), so the 50 ms hold is
1.18e8 ticks; a host read behind it returned after 49.1 ms.  The slowest consumer to enqueue is the training step, 3.1 - 4.4 ms
(its first trip); render_rays takes 0.16 - 0.21 ms, query_sigma 0.06 - 0.14 ms, every other op under 2.4 ms: the hold is more
than ten times the slowest.  The file runs in under 4 s.
On the parent's packing.py / rendering.py / smpl.py the held consumers of section 2 return NaN: query_sigma in all three
precisions, the training step in both arithmetics, render_rays in f32 and bf16x3, sample_pdf(det=True) (the depth steps alone)
and SMPL.forward.  (render_rays in bf16 passed in that run, which was made before the tests insisted on streams that run
concurrently; it has not been repeated.)
"""
import threading
import time

import pytest
import torch

from cases import RENDER_CASES
from helpers import build_case, case_inputs, load_golden
from streams_util import HOLD_MS, first_done, held, hold, independent_streams, poison

pytestmark = pytest.mark.gpu

CASE = "r_moco_global"          # NeRF(ind) + both NoFs, local and global chains: every forward and backward pack of a pair
N_RAYS = 37                     # odd, under one 64-ray tile
N_PTS = 130                     # two 64-point tiles and a tail
PRECISIONS = ("f32", "bf16", "bf16x3")
IND = 0.31


@pytest.fixture(scope="module")
def M():
    import moco_flow_amd
    assert torch.cuda.is_available()
    moco_flow_amd._lib.lib()          # fail loudly if the HIP library is missing
    return moco_flow_amd


@pytest.fixture()
def AB():
    """Two side streams that wait for the default stream and never for each other, and that the device runs concurrently
    with each other and with the default stream (streams_util.independent_streams); drained when the test ends."""
    a, b = independent_streams()
    yield a, b
    a.synchronize()
    b.synchronize()


def _seed():
    return int(load_golden(CASE)["meta_seed"])


def _models(M, seed):
    """(nerf_embs, nerfs, kw) of CASE: fresh modules, cold caches, the synthetic weights of `seed`.  Every test draws its own
    weights: a block that an earlier test's cache freed, and that the allocator hands out again, then holds the wrong bytes."""
    return build_case(M, dict(RENDER_CASES[CASE]), seed, device="cuda")


def _nets(nerfs, kw):
    return list(nerfs) + list(kw["nof_models"])


def _rays(offset=0, n=N_RAYS):
    rays, bg = case_inputs(RENDER_CASES[CASE], _seed() + offset, n=n)
    return rays.cuda(), bg.cuda()


def _points(n=N_PTS, seed=5):
    return (torch.rand(n, 3, generator=torch.Generator().manual_seed(seed)) - 0.5).cuda()


def _tensors(res):
    """The tensors of a result dict in key order; a lazy consensus vector is reduced where it stands (its launch belongs to
    the op and goes to the current stream)."""
    return tuple(v if torch.is_tensor(v) else v.mean() for _, v in sorted(res.items()) if v is not None)


def _render(M, rays, bg, model):
    embs, nerfs, kw = model
    with torch.no_grad():
        return _tensors(M.render_rays(rays, bg, embs, nerfs, **kw))


def _sigma(M, xyz, model, precision):
    embs, nerfs, kw = model
    return (M.query_sigma(xyz, nerfs[0], embs[0], bw_nof=kw["nof_models"][0], nof_embeddings=kw["nof_embeddings"], ind=IND,
                          precision=precision),)


def _train_step(M, rays, bg, gt, model):
    """One step on CASE: render, MSE plus the consensus means, backward -> (rgb, every parameter gradient)."""
    embs, nerfs, kw = model
    nets = _nets(nerfs, kw)
    for m in nets:
        m.zero_grad(set_to_none=True)
    res = M.render_rays(rays, bg, embs, nerfs, **kw)
    loss = ((res["rgb_coarse"] - gt) ** 2).mean()
    for k in sorted(res):
        if k.startswith("nof_"):
            loss = loss + 0.25 * res[k].mean()
    loss.backward()
    grads = tuple(p.grad for m in nets for p in m.parameters())
    assert all(g is not None for g in grads) and len(grads) >= 24
    return (res["rgb_coarse"].detach(),) + grads


def _cache_bytes(model, names):
    """Byte sizes of the packed buffers the serial run left in `names` of every network of `model`."""
    embs, nerfs, kw = model
    out = [getattr(m, n).buf.numel() for m in _nets(nerfs, kw) for n in names if getattr(m, n).buf is not None]
    assert out, names
    return out


def _bump(*models):
    """What an optimizer step does to the cache keys: every parameter edited in place on the default stream."""
    with torch.no_grad():
        for embs, nerfs, kw in models:
            for m in _nets(nerfs, kw):
                for p in m.parameters():
                    p.add_(1e-3)


def _same(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, i)
        assert torch.equal(g, w), f"{what}: output {i} differs from the serial run (NaN in it: {bool(torch.isnan(g.float()).any())})"


def _no_linspace(S):
    """Remove rendering._LINSPACE's entries of S samples -> what was removed (the caller puts it back)."""
    from moco_flow_amd import rendering
    return {k: rendering._LINSPACE.pop(k) for k in [k for k in rendering._LINSPACE if k[0] == S]}


# ------------------------------------------------------------------------------------------------ (2) hidden caches
@pytest.mark.parametrize("precision", PRECISIONS)
def test_forward_packs_and_linspace_built_on_another_stream(M, AB, precision):
    """render_rays on B while the same call, outputs discarded, builds the NeRF's and both NoFs' forward packs and the
    (64, device) depth steps on A behind a hold; then the weights change and A and B swap (every step of a training run
    re-packs).  37 rays of r_moco_global."""
    from moco_flow_amd import rendering
    a, b = AB
    name = {"f32": "_packed", "bf16": "_packed_bf16", "bf16x3": "_packed_x3"}[precision]
    seed = 100 + PRECISIONS.index(precision)
    serial, cold = _models(M, seed), _models(M, seed)
    rays, bg = _rays()
    old = rendering.PRECISION
    M.set_precision(precision)
    try:
        for trip, (pa, pb) in enumerate(((a, b), (b, a))):
            want = _render(M, rays, bg, serial)
            torch.cuda.synchronize()
            sizes = _cache_bytes(serial, (name,)) + [64 * 4]
            saved = _no_linspace(64)
            try:
                got = held(pa, pb, lambda: _render(M, rays, bg, cold), lambda: _render(M, rays, bg, cold), sizes,
                           f"render_rays {precision} trip {trip}")
            finally:
                rendering._LINSPACE.update(saved)
            _same(got, want, f"render_rays {precision}, packs and depth steps built on the other stream (trip {trip})")
            _bump(serial, cold)
    finally:
        M.set_precision(old)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_query_sigma_with_packs_built_on_another_stream(M, AB, precision):
    """query_sigma on 130 points through the backward NoF on B; the producer on A is the explicit pack of the two networks."""
    a, b = AB
    name = {"f32": "_packed", "bf16": "_packed_bf16", "bf16x3": "_packed_x3"}[precision]
    prec = M._lib.PRECISIONS[precision]
    seed = 110 + PRECISIONS.index(precision)
    serial, cold = _models(M, seed), _models(M, seed)
    xyz = _points()
    for trip, (pa, pb) in enumerate(((a, b), (b, a))):
        want = _sigma(M, xyz, serial, precision)
        torch.cuda.synchronize()

        def build():
            cold[1][0].packed(prec)
            cold[2]["nof_models"][0].packed(prec)

        got = held(pa, pb, build, lambda: _sigma(M, xyz, cold, precision), _cache_bytes(serial, (name,)),
                   f"query_sigma {precision} trip {trip}")
        _same(got, want, f"query_sigma {precision}, packs built on the other stream (trip {trip})")
        _bump(serial, cold)


def test_depth_steps_built_on_another_stream(M, AB):
    """rendering._LINSPACE on its own: sample_pdf(det=True) reads the (9, device) table and no packed weights (in render_rays
    the packs' ordering also covers the table: a consumer waits for everything its producer's stream was given so far)."""
    from moco_flow_amd import rendering
    a, b = AB
    g = torch.Generator().manual_seed(3)
    bins = torch.sort(torch.rand(37, 16, generator=g) * 4 + 2, dim=1).values.cuda()
    w = torch.rand(37, 15, generator=g).cuda()
    want = (M.sample_pdf(bins, w, 9, det=True),)
    torch.cuda.synchronize()
    saved = _no_linspace(9)
    try:
        got = held(a, b, lambda: rendering._linspace01(9, bins.device), lambda: (M.sample_pdf(bins, w, 9, det=True),), [9 * 4],
                   "sample_pdf(det=True)")
    finally:
        rendering._LINSPACE.update(saved)
    _same(got, want, "sample_pdf(det=True), depth steps built on the other stream")


def test_backward_packs_built_on_another_stream(M, AB, wgrad):
    """One training step (render_rays + MSE + consensus means, backward) on B; on A, behind a hold, only the packs are built
    -- packed(), packed_bwd(), packed_bwd3() of the three networks, no gradient touched.  Every parameter gradient equals the
    serial step's (test_training_gradients_are_reproducible holds the step bit-identical run to run); `wgrad`: the backward's
    matrix work in exact fp32 and as three bf16 products, so both _packed_bwd and _packed_bwd3 are read."""
    a, b = AB
    seed = 120 + ("f32", "bf16x3").index(wgrad)
    serial, cold = _models(M, seed), _models(M, seed)
    rays, bg = _rays()
    gt = torch.rand(N_RAYS, 3, generator=torch.Generator().manual_seed(1)).cuda()
    for trip, (pa, pb) in enumerate(((a, b), (b, a))):
        want = tuple(t.clone() for t in _train_step(M, rays, bg, gt, serial))
        torch.cuda.synchronize()

        def build():
            for m in _nets(cold[1], cold[2]):
                m.packed()
                m.packed_bwd()
                m.packed_bwd3()

        got = held(pa, pb, build, lambda: _train_step(M, rays, bg, gt, cold),
                   _cache_bytes(serial, ("_packed", "_packed_bwd", "_packed_bwd3")), f"training step {wgrad} trip {trip}")
        _same(got, want, f"training step ({wgrad}), packs built on the other stream (trip {trip})")
        _bump(serial, cold)


def _smpl_pair():
    """Two SMPL modules over the smallest model of tests/smpl_oracle.py (one vertex), shapedirs widened to 12 columns: the
    kernels read the first ten, so the cached copy of that slice is a copy kernel (with ten columns, and the module on the
    device, every cached tensor IS the module's buffer and nothing runs).  `parent` stays on the host: _model reads it, and
    a device read there would wait for the hold and let the producer finish before the consumer is enqueued."""
    import numpy as np
    import smpl_oracle as O
    from moco_flow_amd import smpl as S
    model = O.model(1)
    wide = np.concatenate([model["shapedirs"], np.full((1, 3, 2), 7.0, dtype=np.float32)], axis=2)
    out = []
    for _ in range(2):
        m = S.SMPL(model=dict(model, shapedirs=wide)).cuda()
        m.register_buffer("parent", m.parent.cpu())
        out.append(m)
    return out


def test_smpl_model_copies_made_on_another_stream(M, AB):
    """SMPL.forward of one pose on B while the model's device copies were made on A behind a hold."""
    from moco_flow_amd import synth
    a, b = AB
    serial, cold = _smpl_pair()
    pose, betas = (torch.from_numpy(t).cuda() for t in synth.smpl_pose(5, batch=1, scale=0.6))
    want = (serial(pose, betas),)
    torch.cuda.synchronize()
    assert serial._packed[2]["sd"].data_ptr() != serial.shapedirs.data_ptr()          # a copy, not the buffer
    nbytes = serial._packed[2]["sd"].numel() * 4
    got = held(a, b, lambda: cold._model(pose.device), lambda: (cold(pose, betas),), [nbytes], "SMPL.forward")
    _same(got, want, "SMPL.forward, model copies made on the other stream")


# ------------------------------------------------------------------------------------------------ (3) ops on the current stream
def _op_embedding(M, model):
    e = model[0][0]
    return [_points(300)], lambda x: (e(x), e.rows(x, 2, 64))


def _op_nerf_module(M, model):
    nerf = model[1][0]
    x0 = torch.randn(300, nerf.in_channels_xyz + nerf.extra_feat_dim, generator=torch.Generator().manual_seed(2)).cuda()
    return [x0], lambda x: (nerf(x), nerf(x[:, :nerf.in_channels_xyz], sigma_only=True))


def _op_nof_module(M, model):
    nof = model[2]["nof_models"][0]
    exyz, eind = model[2]["nof_embeddings"]
    ind = torch.full((300, 1), IND, device="cuda")
    return [_points(300)], lambda x: (nof(torch.cat([exyz(x), eind(ind)], -1), x),)


def _op_render(M, model):
    rays, bg = _rays()
    return [rays, bg], lambda r, g: _render(M, r, g, model)


def _op_point_queries(M, model):
    embs, nerfs, kw = model
    q = dict(bw_nof=kw["nof_models"][0], nof_embeddings=kw["nof_embeddings"], ind=IND)
    return [_points()], lambda x: _sigma(M, x, model, "f32") + M.query_radiance(x, nerfs[0], embs, return_canonical=True, **q)


def _op_sample_pdf(M, model):
    g = torch.Generator().manual_seed(3)
    z = torch.sort(torch.rand(37, 16, generator=g) * 4 + 2, dim=1).values.cuda()
    w = torch.rand(37, 16, generator=g).cuda()
    mid = 0.5 * (z[:, :-1] + z[:, 1:])
    return [w], lambda w_: (M.sample_pdf(mid, w_[:, 1:-1], 9, det=True), M.resample_merge(z, w_, 9, det=True))


def _op_camera(M, model):
    import numpy as np
    from moco_flow_amd import camera, image
    from moco_flow_amd.knn import KNN
    H, W = 11, 13
    c2w = np.array([[1, 0, 0, 0.1], [0, 1, 0, -0.2], [0, 0, 1, 3.0], [0, 0, 0, 1]], dtype=np.float64)
    K = np.array([[20.0, 0, W / 2], [0, 20.0, H / 2], [0, 0, 1]])
    aabb = np.array([[x, y, z] for x in (-0.4, 0.4) for y in (-0.5, 0.5) for z in (-0.3, 0.3)], dtype=np.float32)
    g = torch.Generator().manual_seed(4)
    mask = (torch.rand(H * W, generator=g) < 0.6).cuda()
    n = int(mask.sum())
    opacity, depth, bgd = torch.rand(n, generator=g).cuda(), torch.rand(n, generator=g).cuda(), torch.rand(H * W, 3, generator=g).cuda()
    ref = torch.rand(1, 50, 3, generator=g).cuda()
    knn = KNN(k=1, transpose_mode=True)

    def fn(rgb, query):
        return (camera.make_rays(H, W, 20.0, (W / 2, H / 2), c2w, 2.0, 6.0, 0.25), camera.valid_rays_mask(aabb, c2w, K, (H, W)),
                *knn(ref, query), *image.compose_image(mask, opacity, rgb, depth, bgd))

    return [torch.rand(n, 3, generator=g).cuda(), torch.rand(1, 143, 3, generator=g).cuda()], fn


def _op_metrics(M, model):
    g = torch.Generator().manual_seed(6)
    gt = torch.rand(1, 3, 17, 19, generator=g).cuda()
    return [torch.rand(1, 3, 17, 19, generator=g).cuda()], \
        lambda p: (M.metrics.ssim(p, gt), M.metrics.ssim(p, gt, reduction='none'), M.metrics.mse(p, gt), M.metrics.psnr(p, gt))


def _op_vis(M, model):
    H, W = 9, 23
    g = torch.Generator().manual_seed(7)
    rgb = torch.rand(H * W, 3, generator=g).cuda()
    return [torch.rand(H, W, generator=g).cuda() * 5], \
        lambda d: (M.visualize_depth(d), M.visualize_depth(d, 1.0, 4.0), *M.frame_sheet([rgb, d, (d, 0.5, 4.5)], H, W, planar=True))


def _op_marching_cubes(M, model):
    ax = torch.linspace(-1, 1, 9)
    x, y, z = torch.meshgrid(ax, ax * 1.1, ax * 0.9, indexing="ij")
    return [(x * x + y * y + z * z).sqrt().cuda()], lambda v: M.marching_cubes(v, 0.7)


def _op_frame_rays(M, model):
    import numpy as np
    H, W = 11, 13
    c2w = np.array([[1, 0, 0, 0.1], [0, 1, 0, -0.2], [0, 0, 1, 3.0]], dtype=np.float64)
    g = torch.Generator().manual_seed(8)
    mask = (torch.rand(H * W, generator=g) < 0.6).to(torch.uint8).cuda()
    perm = torch.randperm(int(mask.sum()), generator=g).cuda()
    bgd = torch.rand(3, generator=g).cuda()

    def fn(msk, img):
        fr = M.FrameRays(H, W, 20.0, (W / 2, H / 2), c2w, 2.0, 6.0, 0.25, rays_msk=msk)
        return (fr.val_inds,) + fr.sample(37, image=img, background=bgd, perm=perm, chain_idx=-0.5)

    return [mask, torch.rand(H * W, 3, generator=g).cuda()], fn


def _supervision_case(M, model):
    import smpl_oracle as O
    from moco_flow_amd import smpl as S, synth
    smpl = S.SMPL(model=O.model(257)).cuda()
    pose, betas = (torch.from_numpy(t).cuda() for t in synth.smpl_pose(5, batch=2, scale=0.6))
    g = torch.Generator().manual_seed(9)
    n = 150
    draws = (torch.rand(n, 3, generator=g).cuda(), torch.randint(257, (n,), generator=g).cuda(), torch.randn(n, 3, generator=g).cuda())
    embs, nerfs, kw = model

    def losses(p, u):
        corr = M.correspondence(smpl, p[:1], betas[:1], p[1:], betas[1:], n, thickness=0.2, draws=(u,) + draws[1:])
        out = M.point_losses(corr, IND, kw["nof_models"][0], kw["nof_models"][1], kw["nof_embeddings"], nerfs=(nerfs[0],),
                             nerf_embedding_xyz=embs[0], deltas=(1 / 64,))
        return corr, out

    return smpl, pose, betas, draws, losses


def _op_supervision(M, model):
    smpl, pose, betas, draws, losses = _supervision_case(M, model)

    def fn(p, u):
        with torch.no_grad():
            corr, out = losses(p, u)
        return (smpl(p, betas), corr.pairs, corr.inside, corr.dist, corr.ind) + tuple(out[k] for k in sorted(out))

    return [pose, draws[0]], fn


def _param_grads(nets):
    return tuple(p.grad for m in nets for p in m.parameters() if p.grad is not None)


def _zero(nets):
    for m in nets:
        m.zero_grad(set_to_none=True)


def _op_embedding_grad(M, model):
    e = model[0][0]
    w = torch.randn(300, e.out_channels, generator=torch.Generator().manual_seed(10)).cuda()

    def fn(x):
        leaf = x.detach().requires_grad_(True)
        out = e(leaf)
        (out * w).sum().backward()
        return out.detach(), leaf.grad

    return [_points(300)], fn


def _op_nerf_module_grad(M, model):
    nerf = model[1][0]
    x0 = torch.randn(256, nerf.in_channels_xyz + nerf.extra_feat_dim, generator=torch.Generator().manual_seed(2)).cuda()
    w = torch.randn(256, 4, generator=torch.Generator().manual_seed(11)).cuda()

    def fn(x):
        _zero([nerf])
        out = nerf(x)
        (out * w).sum().backward()
        return (out.detach(),) + _param_grads([nerf])

    return [x0], fn


def _op_nof_points_grad(M, model):
    from moco_flow_amd import autograd as A
    nof, embs = model[2]["nof_models"][0], model[2]["nof_embeddings"]
    ind = torch.full((37, 1), IND, device="cuda")
    w = torch.randn(37, 4, 3, generator=torch.Generator().manual_seed(12)).cuda()

    def fn(x):
        _zero([nof])
        leaf = x.detach().view(37, 4, 3).requires_grad_(True)
        out = A.nof_points(leaf, ind, embs, nof)
        (out * w).sum().backward()
        return (out.detach(), leaf.grad) + _param_grads([nof])

    return [_points(148)], fn


def _op_point_losses_grad(M, model):
    smpl, pose, betas, draws, losses = _supervision_case(M, model)
    nets = _nets(model[1], model[2])

    def fn(p, u):
        _zero(nets)
        corr, out = losses(p, u)
        sum(out.values()).backward()
        return tuple(out[k].detach() for k in sorted(out)) + _param_grads(nets)

    return [pose, draws[0]], fn


def _op_train_step(M, model):
    rays, bg = _rays()
    gt = torch.rand(N_RAYS, 3, generator=torch.Generator().manual_seed(1)).cuda()
    return [rays, bg], lambda r, g: _train_step(M, r, g, gt, model)


# name -> (builder, whether the op itself reads the device on the host part way through)
OPS = {"embedding": (_op_embedding, False), "nerf_module": (_op_nerf_module, False), "nof_module": (_op_nof_module, False),
       "render_rays": (_op_render, False), "point_queries": (_op_point_queries, False), "sample_pdf": (_op_sample_pdf, False),
       "camera_knn_compose": (_op_camera, False), "metrics": (_op_metrics, False), "vis": (_op_vis, False),
       "marching_cubes": (_op_marching_cubes, True), "frame_rays": (_op_frame_rays, True), "supervision_smpl": (_op_supervision, False),
       "grad_embedding": (_op_embedding_grad, False), "grad_nerf_module": (_op_nerf_module_grad, False),
       "grad_nof_points": (_op_nof_points_grad, False), "grad_point_losses": (_op_point_losses_grad, False),
       "grad_train_step": (_op_train_step, False)}


@pytest.fixture(scope="module")
def shared_model(M):
    return _models(M, _seed())


@pytest.mark.parametrize("name", list(OPS))
def test_op_runs_on_the_current_stream(M, AB, shared_model, name):
    """The op on B behind a hold.  Its inputs hold NaN (0 for a byte mask) until `x.copy_(x0)` ON B, behind the hold, fills
    them; the blocks its outputs take were filled with 0xFF on B behind the hold.  A launch or a temporary of the op on any
    other stream runs before both and reads NaN or is overwritten.  grad_*: forward and .backward() both under B, outputs
    and gradients compared.  marching_cubes and FrameRays read a count on the host part way (which waits for the hold): for
    them the hold is known to cover the launches in front of that read only, and is asserted there."""
    _, b = AB
    build, reads_host = OPS[name]
    x0s, fn = build(M, shared_model)
    if not name.startswith("grad_"):
        fn = torch.no_grad()(fn)                # the gradient-free kernels; grad_*: the training paths of the same calls
    want = tuple(t.clone() for t in fn(*x0s))
    torch.cuda.synchronize()
    xs = [torch.full_like(x, float("nan")) if x.is_floating_point() else torch.zeros_like(x) for x in x0s]
    torch.cuda.synchronize()
    b.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(b):
        hold(b, HOLD_MS)
        for x, x0 in zip(xs, x0s):
            x.copy_(x0)
        filled, marker = torch.cuda.Event(), torch.cuda.Event()
        filled.record(b)
        marker.record(torch.cuda.default_stream())          # where a launch that ignores the current stream would go
        poison([t.numel() * t.element_size() for t in want])
        assert first_done(marker, filled), "producer was not delayed: the default stream did not run while B was held"
        t0 = time.perf_counter()
        got = fn(*xs)
        enqueue = time.perf_counter() - t0
        delayed = filled.query() is False
    b.synchronize()
    print(f"\n{name}: enqueued in {enqueue * 1e3:.2f} ms")
    assert delayed or reads_host, "producer was not delayed"
    _same(got, want, f"{name} on a side stream")


# ------------------------------------------------------------------------------------------------ (4) threads
def _run_threads(M, models, inputs, streams):
    """Two threads, thread i under streams[i] over models[i]: 3 iterations of (render f32, render bf16x3, query_sigma).
    set_precision is process-wide, so the threads move through the precisions in step: both set the same value, meet at a
    barrier, render, meet again."""
    from moco_flow_amd import rendering
    barrier = threading.Barrier(2)
    results, errors = [[], []], [None, None]

    def work(i):
        try:
            rays, bg, xyz = inputs[i]
            with torch.cuda.stream(streams[i]), torch.no_grad():
                barrier.wait(timeout=60)
                for _ in range(3):
                    for precision in ("f32", "bf16x3"):
                        M.set_precision(precision)
                        barrier.wait(timeout=60)
                        results[i].append(_render(M, rays, bg, models[i]))
                        barrier.wait(timeout=60)
                    results[i].append(_sigma(M, xyz, models[i], "f32"))
        except BaseException as e:          # re-raised in the test's thread
            errors[i] = e
            barrier.abort()

    old = rendering.PRECISION
    try:
        cur = torch.cuda.current_stream()
        for s in streams:
            s.wait_stream(cur)
        threads = [threading.Thread(target=work, args=(i,), daemon=True) for i in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=120)
        assert not any(t.is_alive() for t in threads), "a thread did not finish within 120 s"
        for e in errors:
            if e is not None and not isinstance(e, threading.BrokenBarrierError):
                raise e
        for e in errors:
            if e is not None:
                raise e
        for s in streams:
            s.synchronize()
    finally:
        M.set_precision(old)
    return results


@pytest.mark.parametrize("shared", [True, False], ids=["shared_modules", "distinct_modules"])
def test_two_threads_on_their_own_streams(M, AB, shared):
    """Two Python threads, a stream each, start from a barrier over one shared pair of fresh, cold-cache modules (then over
    distinct ones): each renders its own 37 rays in f32 and bf16x3 and queries sigma, three times over; every result equals
    the serial one.

    This cannot force a race: it is a check against cross-talk between threads and against crashes.  The deterministic tests
    of the ordering are the ones above (sections 2 and 3)."""
    from moco_flow_amd import rendering
    seed = 130 + int(shared)
    serial = _models(M, seed)
    inputs = [_rays(offset=i) + (_points(seed=20 + i),) for i in range(2)]
    want = []
    old = rendering.PRECISION
    try:
        for rays, bg, xyz in inputs:
            per = []
            for precision in ("f32", "bf16x3"):
                M.set_precision(precision)
                per.append(_render(M, rays, bg, serial))
            per.append(_sigma(M, xyz, serial, "f32"))
            want.append(per)
    finally:
        M.set_precision(old)
    torch.cuda.synchronize()
    cold = _models(M, seed)
    models = [cold, cold] if shared else [cold, _models(M, seed)]
    results = _run_threads(M, models, inputs, AB)
    for i in range(2):
        assert len(results[i]) == 9
        for k, got in enumerate(results[i]):
            _same(got, want[i][k % 3], f"thread {i}, iteration {k // 3}, step {k % 3}")


def test_last_error_is_per_thread(M):
    """No GPU work: two threads behind a barrier alternate 200 refusals that return before any launch (both checks stand in
    front of mf_composite_backward's n_rays == 0 return), and each reads mf_last_error() after its own call: always its own
    text."""
    lib = M._lib.lib()
    barrier = threading.Barrier(2)
    calls = [dict(S=4096, activation=0, text=b"S=4096 (1..2048)"), dict(S=64, activation=7, text=b"activation 7")]
    seen, errors = [[], []], [None, None]

    def work(i):
        try:
            c = calls[i]
            barrier.wait(timeout=60)
            for _ in range(200):
                rc = lib.mf_composite_backward(None, 0, 0, c["S"], None, None, None, c["activation"], None, None, None, None, None, None)
                seen[i].append((rc, lib.mf_last_error()))
        except BaseException as e:
            errors[i] = e
            barrier.abort()

    threads = [threading.Thread(target=work, args=(i,), daemon=True) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=60)
    assert not any(t.is_alive() for t in threads)
    for e in errors:
        if e is not None:
            raise e
    for i in range(2):
        assert len(seen[i]) == 200
        for rc, text in seen[i]:
            assert rc != 0 and calls[i]["text"] in text and calls[1 - i]["text"] not in text, (i, rc, text)
