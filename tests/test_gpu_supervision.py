"""moco_flow_amd.supervision on the device (csrc/mf_supervise.hip): mf_point_correspond against an integer-arithmetic oracle on a
lattice and, bit for bit, against the kernels it fuses (mf_knn1 + mf_apply_vertex_transforms) at every lanes_per_query; the
three point losses and their backward against the torch restatement of the reference (tests/supervision_oracle.py); the whole
path against the compacting path it replaces (smpl.frame_correspondence + module calls + nn.L1Loss / nn.BCELoss); and the
absence of a host synchronisation.  Every test prints the figures it asserts on."""
import functools

import numpy as np
import pytest
import torch
from torch import nn

import supervision_oracle as O

pytestmark = pytest.mark.gpu

LANES = (1, 4, 16, 64, 0)


@pytest.fixture(scope="module")
def M():
    import moco_flow_amd
    return moco_flow_amd


def l2rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


# ---- 1. the lattice -------------------------------------------------------------------------------------------------

def _lattice_case(V, Q):
    """Integer coordinates k (the points are k / 8, |k| <= 512), integer transforms t (the entries are t / 4, |t| <= 8), and the
    plants: (query, the index it must get)."""
    rng = np.random.default_rng(100 * V + Q)
    ref = rng.integers(-400, 401, size=(V, 3))
    qry = rng.integers(-400, 401, size=(Q, 3))
    tk = rng.integers(-8, 9, size=(V, 3, 4))
    plants = []
    if V >= 1061:
        # duplicates of a query's nearest vertex, outside the cloud's box: on the same lane at T = 4 (3 and 11), on neighbouring
        # lanes (5 and 6), on the two sides of the tile boundary (1020 and 1030)
        for (a, b), pt in (((3, 11), (505, -509, 500)), ((5, 6), (-507, 503, -501)), ((1020, 1030), (511, 508, -506))):
            ref[a] = ref[b] = pt
            plants.append((np.array(pt) + (1, 0, 0), a))
        ref[V - 1] = (-500, -500, 510)                                      # the last tile holds 37 vertices: its last one
        plants.append((np.array([-500, -501, 510]), V - 1))
    # one query at exactly dist == thickness = 0.25 (2 lattice steps) from its vertex: outside
    ref[0] = (480, 480, 480)
    plants.append((np.array([480, 482, 480]), 0))
    plants = plants[Q % len(plants):] + plants[:Q % len(plants)]            # Q = 1 has room for one
    for j, (pt, _) in enumerate(plants[:Q]):
        qry[j] = pt
    return ref, qry, tk, plants[:Q]


def _lattice_oracle(ref, qry, tk, thickness_steps):
    d2 = ((ref[None, :, :] - qry[:, None, :]).astype(np.int64) ** 2).sum(-1)             # units of 1 / 64
    ind = d2.argmin(1)                                                                   # numpy: the first minimum
    best = d2[np.arange(len(qry)), ind]
    cano32 = (tk[ind, :, :3] * qry[:, None, :]).sum(-1) + 8 * tk[ind, :, 3]              # units of 1 / 32
    return ind, best, best < thickness_steps ** 2, cano32


@pytest.mark.parametrize("Q", [1, 259])
@pytest.mark.parametrize("V", [1, 5, 1061])
def test_point_correspond_exact_on_a_lattice(M, V, Q):
    """Points k / 8 with |k| <= 512 and transform entries t / 4: every difference, square, fma and product of the kernel is
    exact in fp32, so int64 arithmetic gives THE answer -- index (first minimum), distance, flag and canonical point -- for
    every query, at every lanes_per_query, across the 1024-vertex tiles (1061 = one full tile + 37: a last tile with fewer than
    64 vertices; V = 1 and 5: fewer vertices than lanes) and the workgroups (259 queries: 2 workgroups at one lane per query,
    65 at 64)."""
    S = M.supervision
    ref, qry, tk, plants = _lattice_case(V, Q)
    want_i, want_d2, want_in, want_c32 = _lattice_oracle(ref, qry, tk, 2)
    for j, (_, idx) in enumerate(plants):
        assert want_i[j] == idx, (j, idx)                                                 # the plants are what they claim to be
    assert int(want_d2.max()) < 2 ** 24 and int(np.abs(want_c32).max()) < 2 ** 24         # exact in fp32
    T = np.zeros((V, 4, 4), dtype=np.float32)
    T[:, :3, :] = tk / 4.0
    T[:, 3, :] = (7.0, -3.0, 5.0, 11.0)                                                   # the last row is never read
    verts, trans = torch.from_numpy((ref / 8.0).astype(np.float32)).cuda(), torch.from_numpy(T).cuda()
    query = torch.from_numpy((qry / 8.0).astype(np.float32)).cuda()
    want_d = np.sqrt((want_d2 / 64.0).astype(np.float32))
    want_pairs = np.concatenate([(qry / 8.0), want_c32 / 32.0], axis=1).astype(np.float32)
    outs = []
    for lanes in LANES:
        c = S.point_correspond(verts, trans, query, 0.25, lanes_per_query=lanes)
        torch.cuda.synchronize()
        assert c.pairs.shape == (Q, 6) and c.inside.dtype == torch.uint8 and c.ind.dtype == torch.int64
        wrong = int((c.ind.cpu().numpy() != want_i).sum())
        print(f"V={V} Q={Q} lanes={lanes}: {wrong} wrong indices, inside {int(c.inside.sum())} of {Q}")
        assert np.array_equal(c.ind.cpu().numpy(), want_i), (lanes, wrong)
        assert np.array_equal(c.dist.cpu().numpy(), want_d), lanes
        assert np.array_equal(c.inside.cpu().numpy(), want_in.astype(np.uint8)), lanes
        assert np.array_equal(c.pairs.cpu().numpy(), want_pairs), lanes
        outs.append(c)
    for c in outs[1:]:
        for name in ("pairs", "inside", "dist", "ind"):
            assert torch.equal(getattr(c, name), getattr(outs[0], name)), name
    for j, (_, idx) in enumerate(plants):
        if idx == 0:
            assert float(outs[0].dist[j]) == 0.25 and int(outs[0].inside[j]) == 0          # dist == thickness: outside


# ---- 2, 3. the kernels it fuses --------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def smpl_case():
    """The 6890-vertex synthetic model, a source and a target pose, and what every test below shares of them (computed once,
    never written): verts, trans, 2000 queries in the 3-cube, and mf_knn1 + mf_apply_vertex_transforms on them."""
    from moco_flow_amd import smpl as S, synth
    from moco_flow_amd.knn import KNN
    m = S.SMPL(model=synth.smpl_model(1, 6890)).cuda()
    pose, betas = synth.smpl_pose(5, batch=2, scale=0.6)
    pose, betas = torch.from_numpy(pose).cuda(), torch.from_numpy(betas).cuda()
    verts = m(pose[:1], betas[:1])[0]
    T = m.get_vertex_transformation(pose, betas)
    trans = S.frame_transforms(T[0], T[1])
    Q = 2000
    query = torch.from_numpy(((synth.uniform01(3, Q * 3).reshape(Q, 3) - 0.5) * 3.0).astype(np.float32)).cuda()
    dist, ind = KNN(k=1, transpose_mode=True)(verts[None], query[None])
    cano = S.apply_vertex_transforms(trans, ind[0], query)
    return dict(smpl=m, pose=pose, betas=betas, verts=verts, trans=trans, query=query, dist=dist[0, :, 0], ind=ind[0, :, 0], cano=cano)


def test_point_correspond_bit_identical_to_knn_and_transform(M):
    """Non-lattice input at the joint stage's size (Q = 2000, V = 6890): pairs, dist and ind are torch.equal to mf_knn1 followed
    by mf_apply_vertex_transforms at every lanes_per_query, and correspondence(...).split() to smpl.frame_correspondence."""
    from moco_flow_amd import smpl as S0
    S, c = M.supervision, smpl_case()
    for lanes in LANES:
        got = S.point_correspond(c["verts"], c["trans"], c["query"], 0.2, lanes_per_query=lanes)
        assert torch.equal(got.ind, c["ind"]), lanes
        assert torch.equal(got.dist, c["dist"]), lanes
        assert torch.equal(got.pairs, torch.cat([c["query"], c["cano"]], -1)), lanes
        assert torch.equal(got.inside.bool(), c["dist"] < 0.2), lanes
    corr = S.correspondence(c["smpl"], c["pose"][:1], c["betas"][:1], c["pose"][1:], c["betas"][1:], 0, thickness=0.2, queries=c["query"])
    inside, outside = S0.frame_correspondence(c["smpl"], c["pose"][:1], c["betas"][:1], c["pose"][1:], c["betas"][1:], c["query"], thickness=0.2)
    a, b = corr.split()
    print(f"inside {a.shape[0]}, outside {b.shape[0]} of {c['query'].shape[0]}")
    assert a.shape[0] > 10 and b.shape[0] > 10
    assert torch.equal(a, inside) and torch.equal(b, outside)


def test_fused_query_generation(M):
    """pick and noise given: the query columns are verts[pick] + noise * thickness as torch evaluates it on the device's own verts
    (product and sum rounded once each), bit for bit; the rest of the row is what the same points give when passed in; the
    sampled correspondence puts the cube points first."""
    S, c = M.supervision, smpl_case()
    g = torch.Generator(device="cuda").manual_seed(11)
    n = 777
    u = torch.rand((n, 3), device="cuda", generator=g)
    pick = torch.randint(6890, (n,), device="cuda", generator=g)
    pick[:2] = torch.tensor([0, 6889], device="cuda")
    noise = torch.randn((n, 3), device="cuda", generator=g)
    for thickness in (0.2, 0.1):
        want = c["verts"][pick] + noise * thickness
        for lanes in (1, 16, 0):
            got = S.point_correspond(c["verts"], c["trans"], None, thickness, pick=pick, noise=noise, lanes_per_query=lanes)
            assert torch.equal(got.pairs[:, :3], want), (thickness, lanes)
            given = S.point_correspond(c["verts"], c["trans"], want, thickness, lanes_per_query=lanes)
            for name in ("pairs", "inside", "dist", "ind"):
                assert torch.equal(getattr(got, name), getattr(given, name)), name
    corr = S.correspondence(c["smpl"], c["pose"][:1], c["betas"][:1], c["pose"][1:], c["betas"][1:], n, thickness=0.2, draws=(u, pick, noise))
    want_q = O.sample_queries(c["verts"], u, pick, noise, 0.2)
    assert corr.pairs.shape == (2 * n, 6) and torch.equal(corr.pairs[:, :3], want_q)
    ref = S.point_correspond(c["verts"], c["trans"], want_q, 0.2)
    assert torch.equal(corr.pairs, ref.pairs) and torch.equal(corr.ind, ref.ind) and torch.equal(corr.inside, ref.inside)
    # drawn here: the same generator state gives the same draws in the reference's order
    g1, g2 = torch.Generator(device="cuda").manual_seed(5), torch.Generator(device="cuda").manual_seed(5)
    drawn = S.correspondence(c["smpl"], c["pose"][:1], c["betas"][:1], c["pose"][1:], c["betas"][1:], 64, generator=g1)
    d = (torch.rand((64, 3), device="cuda", generator=g2), torch.randint(6890, (64,), device="cuda", generator=g2),
         torch.randn((64, 3), device="cuda", generator=g2))
    again = S.correspondence(c["smpl"], c["pose"][:1], c["betas"][:1], c["pose"][1:], c["betas"][1:], 64, draws=d)
    assert torch.equal(drawn.pairs, again.pairs)


# ---- 4, 5. the losses ------------------------------------------------------------------------------------------------

DELTAS = (1 / 128, 1 / 256)


PT_LOSS_THREADS, PT_LOSS_MAX_BLOCKS = 256, 256       # mf_supervise.hip: kPtLossThreads, kPtLossMaxBlocks
Q_CAPPED = PT_LOSS_THREADS * PT_LOSS_MAX_BLOCKS + 300  # the 256-block cap binds; the first 300 threads take a second grid-stride trip


@functools.lru_cache(maxsize=None)
def loss_case(Q=300):
    """Q rows (300 unless said), about half inside, two sigma planes drawn from [-6, 6] (alpha <= 0.5 there: delta softplus(6) < 0.05) with
    25 and -40 planted on outside rows, and one prediction equal to its target."""
    g = torch.Generator().manual_seed(21)
    pairs = torch.randn((Q, 6), generator=g)
    inside = torch.rand(Q, generator=g) < 0.5
    inside[:4] = torch.tensor([False, False, True, False])
    pred_bw = pairs[:, 3:] + 0.3 * torch.randn((Q, 3), generator=g)
    pred_fw = pairs[:, :3] + 0.3 * torch.randn((Q, 3), generator=g)
    pred_bw[2, 1] = pairs[2, 4]                                              # an inside row: sign(0) = 0
    sig = [torch.rand(Q, generator=g) * 12 - 6 for _ in DELTAS]
    sig[0][0], sig[1][0], sig[0][1], sig[1][3] = 25.0, -40.0, -40.0, 25.0
    return dict(Q=Q, pairs=pairs, inside=inside, pred_bw=pred_bw, pred_fw=pred_fw, sig=sig, planted=((0, 0), (1, 0), (0, 1), (1, 3)))


def _partials(M, c, inside, use_all=False, sig=None):
    import ctypes as C
    import moco_flow_amd._lib as L
    S = M.supervision
    dev = lambda t: None if t is None else t.cuda().contiguous()
    sig = c["sig"] if sig is None else sig
    t = dict(pairs=dev(c["pairs"]), inside=None if inside is None else dev(inside.to(torch.uint8)), bw=dev(c["pred_bw"]), fw=dev(c["pred_fw"]),
             sig=[dev(s) for s in sig])
    a = S._loss_args(t["pairs"], t["inside"], use_all, t["bw"], t["fw"], t["sig"], DELTAS[:len(sig)])
    out6 = torch.full((6,), float("nan"), dtype=torch.float64, device="cuda")
    means = torch.full((3,), float("nan"), device="cuda")
    scratch = torch.empty(max(int(L.lib().mf_point_loss_partials_scratch_bytes(c["Q"])), 8), dtype=torch.uint8, device="cuda")
    L.check(L.lib().mf_point_loss_partials(C.byref(a), out6.data_ptr(), means.data_ptr(), scratch.data_ptr(),
                                           L.current_stream(out6.device)), "mf_point_loss_partials")
    torch.cuda.synchronize()
    return out6.cpu(), means.cpu()


def test_point_loss_partials_values(M):
    c = loss_case()
    Q, inside = c["Q"], c["inside"]
    out6, means = _partials(M, c, inside)
    n_in, n_out = int(inside.sum()), int((~inside).sum())
    assert out6[1] == 3 * n_in and out6[3] == 3 * n_in and out6[5] == 2 * n_out                       # counts are exact
    # L1: the float64 sum of the same fp32 |a - b|, in another order: 900 additions, 900 x 2^-53 ~ 1e-13 relative
    for k, (pred, target) in enumerate(((c["pred_bw"], c["pairs"][:, 3:]), (c["pred_fw"], c["pairs"][:, :3]))):
        want = (pred - target).abs()[inside].double().sum()
        rel = abs(float(out6[2 * k]) - float(want)) / float(want)
        print(f"L1 term {k}: sum {float(out6[2 * k]):.17g} vs {float(want):.17g}, relative difference {rel:.3e}")
        assert rel <= 1e-12
    want = O.point_losses(c["pairs"], inside, c["pred_bw"], c["pred_fw"], c["sig"], DELTAS)
    for k, key in enumerate(("nof_bw", "nof_fw", "alphas_mask")):
        diff = abs(float(means[k]) - float(want[key][0]))
        print(f"{key}: {float(means[k]):.9g} vs the oracle's {float(want[key][0]):.9g}, difference {diff:.3e}; count {want[key][1]}")
        assert out6[2 * k + 1] == want[key][1]
        assert diff <= 1e-6                                                                          # the issue's bar for the BCE mean
    mean_bce = float(out6[4] / out6[5])
    print(f"BCE mean from the float64 partials {mean_bce:.9g}, difference {abs(mean_bce - float(want['alphas_mask'][0])):.3e}")
    assert abs(mean_bce - float(want["alphas_mask"][0])) <= 1e-6
    # the planted rows one by one: a plane that is -40 everywhere but on the row, whose BCE is exactly 0 there (alpha rounds to 0)
    only = torch.zeros(Q, dtype=torch.bool)
    for plane, row in c["planted"]:
        sig = torch.full((Q,), -40.0)
        sig[row] = c["sig"][plane][row]
        one, _ = _partials(M, dict(c, sig=[sig] if plane == 0 else [torch.full((Q,), -40.0), sig]), only)
        want_row = float(O.bce_rows(c["sig"][plane][row:row + 1], DELTAS[plane]))
        ulp = float(np.spacing(np.float32(abs(want_row)))) if want_row else 0.0
        print(f"planted sigma {float(c['sig'][plane][row])} delta 1/{round(1 / DELTAS[plane])}: {float(one[4]):.9g} vs {want_row:.9g} (ulp {ulp:.3e})")
        assert abs(float(one[4]) - want_row) <= 4 * ulp
    # emptied terms
    all_in, _m = _partials(M, c, torch.ones(Q, dtype=torch.bool))
    assert all_in[5] == 0 and all_in[4] == 0 and _m[2] == 0 and all_in[1] == 3 * Q
    all_out, _m = _partials(M, c, torch.zeros(Q, dtype=torch.bool))
    assert all_out[1] == 0 and all_out[0] == 0 and all_out[3] == 0 and all_out[2] == 0 and _m[0] == 0 and _m[1] == 0 and all_out[5] == 2 * Q
    # a NULL mask / use_all: every row for the L1 terms
    no_mask, _ = _partials(M, c, None)
    every, _ = _partials(M, c, inside, use_all=True)
    assert torch.equal(no_mask[:4], all_in[:4]) and no_mask[5] == 0
    assert torch.equal(every[:4], all_in[:4]) and torch.equal(every[4:], out6[4:])
    again, means2 = _partials(M, c, inside)
    assert torch.equal(again, out6) and torch.equal(means2, means)                                     # bit-identical runs


def test_point_loss_partials_block_cap_binds_values(M):
    """loss_case()'s recipe at Q_CAPPED against the oracle, with test_point_loss_partials_values' bars."""
    c = loss_case(Q_CAPPED)
    inside = c["inside"]
    assert -(-c["Q"] // PT_LOSS_THREADS) > PT_LOSS_MAX_BLOCKS
    out6, means = _partials(M, c, inside)
    want = O.point_losses(c["pairs"], inside, c["pred_bw"], c["pred_fw"], c["sig"], DELTAS)
    for k, key in enumerate(("nof_bw", "nof_fw", "alphas_mask")):
        print(f"{key}: {float(means[k]):.9g} vs the oracle's {float(want[key][0]):.9g}, difference "
              f"{abs(float(means[k]) - float(want[key][0])):.3e}; count {float(out6[2 * k + 1])!r} vs {want[key][1]}")
        assert out6[2 * k + 1] == want[key][1]
    mean_bce = float(out6[4] / out6[5])
    assert abs(float(means[2]) - float(want["alphas_mask"][0])) <= 1e-6                                # the BCE mean's bar
    assert abs(mean_bce - float(want["alphas_mask"][0])) <= 1e-6


def test_point_loss_partials_block_cap_binds_exact_l1(M):
    """Predictions and targets that are multiples of 1/16 in [0, 1]: every fp32 |a - b| is one too, and a sum of 3 Q of them has
    fewer than 30 significant bits -- exact in float64 whatever the order of the additions, so the L1 sums must EQUAL the integer
    arithmetic's, and a row lost or taken twice on the second grid-stride trip shows in them and in the counts."""
    Q = Q_CAPPED
    g = torch.Generator().manual_seed(77)
    k16 = lambda *shape: torch.randint(0, 17, shape, generator=g)
    pairs, bw, fw = k16(Q, 6), k16(Q, 3), k16(Q, 3)
    inside = torch.rand(Q, generator=g) < 0.5
    sig = [torch.rand(Q, generator=g) * 12 - 6 for _ in DELTAS]
    c = dict(Q=Q, pairs=pairs.float() / 16, pred_bw=bw.float() / 16, pred_fw=fw.float() / 16, sig=sig)
    out6, means = _partials(M, c, inside)
    n_in, n_out = int(inside.sum()), int((~inside).sum())
    want_bw = int((bw - pairs[:, 3:]).abs()[inside].sum()) / 16
    want_fw = int((fw - pairs[:, :3]).abs()[inside].sum()) / 16
    print(f"Q={Q}: L1 sums {float(out6[0])!r} {float(out6[2])!r} exact {want_bw!r} {want_fw!r}; counts {out6[1::2].tolist()} "
          f"for {n_in} inside, {n_out} outside")
    assert float(out6[0]) == want_bw and float(out6[2]) == want_fw
    assert out6[1] == 3 * n_in and out6[3] == 3 * n_in and out6[5] == 2 * n_out
    again, means2 = _partials(M, c, inside)
    assert torch.equal(again, out6) and torch.equal(means2, means)                                     # bit-identical runs


def test_point_loss_partials_backward(M):
    S, c = M.supervision, loss_case()
    inside = c["inside"]
    seeds = torch.tensor([0.7, -1.3, 2.5])
    leaf = lambda t: t.clone().requires_grad_(True)
    # the oracle's autograd
    o = dict(bw=leaf(c["pred_bw"]), fw=leaf(c["pred_fw"]), sig=[leaf(s) for s in c["sig"]])
    want = O.point_losses(c["pairs"], inside, o["bw"], o["fw"], o["sig"], DELTAS)
    sum(s * want[k][0] for s, k in zip(seeds, ("nof_bw", "nof_fw", "alphas_mask"))).backward()
    d = dict(bw=leaf(c["pred_bw"].cuda()), fw=leaf(c["pred_fw"].cuda()), sig=[leaf(s.cuda()) for s in c["sig"]])
    means = S.loss_means(c["pairs"].cuda(), inside.to(torch.uint8).cuda(), d["bw"], d["fw"], d["sig"], DELTAS)
    (means * seeds.cuda()).sum().backward()
    for key in ("bw", "fw"):
        got, ref = d[key].grad.cpu(), o[key].grad
        ulps = float(((got - ref).abs() / torch.from_numpy(np.spacing(ref.abs().numpy())).clamp_min(1e-45)).max())
        print(f"g_pred_{key}: max difference {ulps:.2f} ulp")
        assert ulps <= 1.0
        assert float(got[~inside].abs().max()) == 0.0 and float(ref[~inside].abs().max()) == 0.0      # exact zeros on masked rows
        assert int((got[inside] == 0).sum()) == int((ref[inside] == 0).sum())
    assert float(d["bw"].grad[2, 1]) == 0.0 and float(d["bw"].grad[2, 0]) != 0.0                        # pred == target: sign(0) = 0
    for k in range(2):
        got, ref = d["sig"][k].grad.cpu(), o["sig"][k].grad
        err = float(((got - ref).abs() - 1e-9).clamp_min(0).div(ref.abs().clamp_min(1e-30)).max())
        print(f"g_sigma{k}: max (|difference| - 1e-9) / |oracle| = {err:.3e}")
        assert bool(((got - ref).abs() <= 1e-5 * ref.abs() + 1e-9).all())
        assert float(got[inside].abs().max()) == 0.0
    for plane, row in c["planted"]:
        got, ref = float(d["sig"][plane].grad[row]), float(o["sig"][plane].grad[row])
        print(f"planted sigma {float(c['sig'][plane][row])}: gradient {got:.9g} vs torch's {ref:.9g}")
        if float(c["sig"][plane][row]) == -40.0:
            assert got == ref == 0.0                                                                 # alpha rounds to 0, the 1e-12 clamp
    # an emptied term has zero gradients
    d2 = dict(bw=leaf(c["pred_bw"].cuda()), sig=[leaf(c["sig"][0].cuda())])
    m = S.loss_means(c["pairs"].cuda(), torch.zeros(c["Q"], dtype=torch.uint8).cuda(), d2["bw"], None, d2["sig"], DELTAS[:1])
    m.sum().backward()
    assert float(d2["bw"].grad.abs().max()) == 0.0 and float(d2["sig"][0].grad.abs().max()) > 0.0


def test_point_loss_seeds_bit_identical_to_torch_on_the_device(M):
    """The seeds of mf_point_loss_partials_backward against torch's OWN device kernels for the compacted sets (nn.L1Loss,
    nn.BCELoss of 1 - exp(-delta softplus(sigma)) over the cat of both planes): torch.equal on every row the mask keeps.  The
    bound is 0 because the kernel restates those kernels operation by operation on the same device maths library -- it is what
    lets the end-to-end gradients below sit at the compacted path's own run-to-run floor.  Unit seeds (what summing the losses
    gives) and uneven ones."""
    S, c = M.supervision, loss_case()
    inside = c["inside"].cuda()
    out = ~inside
    pairs = c["pairs"].cuda()
    leaf = lambda t: t.cuda().clone().requires_grad_(True)
    for seeds in (torch.ones(3), torch.tensor([0.7, -1.3, 0.37])):
        seeds = seeds.cuda()
        d = dict(bw=leaf(c["pred_bw"]), fw=leaf(c["pred_fw"]), sig=[leaf(s) for s in c["sig"]])
        means = S.loss_means(pairs, inside.to(torch.uint8), d["bw"], d["fw"], d["sig"], DELTAS)
        (means * seeds).sum().backward()
        t = dict(bw=leaf(c["pred_bw"]), fw=leaf(c["pred_fw"]), sig=[leaf(s) for s in c["sig"]])
        alphas = torch.cat([1 - torch.exp(-dl * nn.Softplus()(s[out])) for s, dl in zip(t["sig"], DELTAS)])
        (seeds[0] * nn.L1Loss()(t["bw"][inside], pairs[inside][:, 3:]) + seeds[1] * nn.L1Loss()(t["fw"][inside], pairs[inside][:, :3])
         + seeds[2] * nn.BCELoss()(alphas, torch.zeros_like(alphas))).backward()
        for name, got, ref in (("g_pred_bw", d["bw"].grad, t["bw"].grad), ("g_pred_fw", d["fw"].grad, t["fw"].grad),
                               ("g_sigma0", d["sig"][0].grad, t["sig"][0].grad), ("g_sigma1", d["sig"][1].grad, t["sig"][1].grad)):
            print(f"seeds {[round(float(x), 2) for x in seeds]} {name}: {int((got != ref).sum())} of {got.numel()} elements differ from torch's")
            assert bool(torch.isfinite(got).all()) and float(ref.abs().max()) > 0.0
            assert torch.equal(got, ref), name


# ---- 6. end to end ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def nets():
    import moco_flow_amd as M
    from moco_flow_amd import synth
    load = lambda m, sd: (m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}), m.cuda())[1]
    bw = load(M.NoF(4, 128, 33, [2], "ind", 33, True), synth.nof_state(3, use_quat=True, tag="bw", head_scale=0.25))
    fw = load(M.NoF(4, 128, 33, [2], "ind", 33, True), synth.nof_state(4, use_quat=True, tag="fw", head_scale=0.25))
    nerf = load(M.NeRF(8, 256, 63, [4], "ind", 5), synth.nerf_state(3, extra_feat_type="ind", extra_feat_dim=5, regime="dense"))
    return bw, fw, nerf, (M.Embedding(3, 5), M.Embedding(1, 16)), M.Embedding(3, 10)


IND = 0.1
DELTA = 1 / 128


def _parent_step(inside_pts, outside_pts, only_msk=False, stage2=False):
    """The path this replaces: module calls on the compacted sets with nn.L1Loss / nn.BCELoss (trainer_moco_flow.py:330-363;
    stage2: trainer_nof.py:115-125) -> ({term: value}, {module: [gradients]})."""
    import torch.nn.functional as F
    bw, fw, nerf, (exyz, eind), nxyz = nets()
    for m in (bw, fw, nerf):
        m.zero_grad(set_to_none=True)

    def nof(m, xyz):
        ind = torch.full((xyz.shape[0], 1), IND, device="cuda")
        return m(torch.cat([exyz(xyz), eind(ind)], -1), xyz)

    losses = {}
    if stage2:
        pts = torch.cat([inside_pts, outside_pts], 0)
        q, cn = pts[:, :3].contiguous(), pts[:, 3:].contiguous()
        losses["nof_bw"] = nn.L1Loss()(nof(bw, q), cn)
        losses["nof_fw"] = nn.L1Loss()(nof(fw, cn), q)
    else:
        if not only_msk:
            q, cn = inside_pts[:, :3].contiguous(), inside_pts[:, 3:].contiguous()
            losses["nof_bw"] = nn.L1Loss()(nof(bw, q), cn)
            losses["nof_fw"] = nn.L1Loss()(nof(fw, cn), q)
        oq = outside_pts[:, :3].contiguous()
        emb = nxyz(nof(bw, oq))
        sig = nerf(F.pad(emb, (0, nerf.in_channels_xyz - emb.shape[1])), sigma_only=True)
        alphas = 1 - torch.exp(-DELTA * nn.Softplus()(sig))
        losses["alphas_mask"] = nn.BCELoss()(alphas, torch.zeros_like(alphas))
    sum(losses.values()).backward()
    grads = {name: [None if p.grad is None else p.grad.clone() for p in m.parameters()] for name, m in (("bw", bw), ("fw", fw), ("nerf", nerf))}
    return {k: float(v) for k, v in losses.items()}, grads


def _masked_step(M, corr, **kw):
    bw, fw, nerf, nof_embs, nxyz = nets()
    for m in (bw, fw, nerf):
        m.zero_grad(set_to_none=True)
    losses = M.point_losses(corr, IND, bw, fw, nof_embs, nerfs=(nerf,), nerf_embedding_xyz=nxyz, deltas=(DELTA,), **kw)
    sum(losses.values()).backward()
    grads = {name: [None if p.grad is None else p.grad.clone() for p in m.parameters()] for name, m in (("bw", bw), ("fw", fw), ("nerf", nerf))}
    return {k: float(v) for k, v in losses.items()}, grads


def _compare(tag, got, first, second):
    """Losses within 1e-6 relative; every gradient tensor within max(4 x the parent's own run-to-run difference, 1e-6) l2-rel:
    -> the tensors over that bar."""
    (gl, gg), (fl, fg), (_, sg) = got, first, second
    assert set(gl) == set(fl), (set(gl), set(fl))
    for k in fl:
        rel = abs(gl[k] - fl[k]) / abs(fl[k])
        print(f"{tag} {k}: {gl[k]:.9g} vs the compacted path's {fl[k]:.9g}, relative difference {rel:.3e}")
        assert rel <= 1e-6, k
    worst, bad = (0.0, 0.0, None), []
    for name in fg:
        for i, (a, b, c) in enumerate(zip(gg[name], fg[name], sg[name])):
            if b is None or float(b.abs().max()) == 0.0:
                assert a is None or float(a.abs().max()) == 0.0, (name, i)
                continue
            floor, diff = l2rel(c, b), l2rel(a, b)
            print(f"{tag} {name}[{i}]: difference {diff:.3e} l2-rel, the compacted path's own run-to-run floor {floor:.3e}")
            if diff > worst[1]:
                worst = (floor, diff, f"{name}[{i}]")
            if diff > max(4 * floor, 1e-6):
                bad.append((tag, name, i, diff, floor))
    print(f"{tag}: largest gradient difference {worst[1]:.3e} l2-rel at {worst[2]} (the compacted path's own run-to-run floor there {worst[0]:.3e})")
    return bad


def test_point_losses_end_to_end_vs_the_compacted_path(M, wgrad):
    """2 x 150 sampled points on the 6890-vertex model through c2f's networks: values and every parameter gradient of
    point_losses against the parent's path on corr.split(); the yardstick for the gradients is that path's own difference
    between two runs, the second with each compacted set's rows reversed (another summation order in the weight gradients).

    Run in both arithmetics of the backward's matrix work (conftest's `wgrad`: exact-fp32 MFMA, and the default three bf16
    products for the dX chains and the weight gradients).

    MEASURED on an MI355X: every loss value agrees to <= 7.8e-8 relative.  Largest gradient difference against the floor at
    the same tensor (all at the backward NoF's last bias but stage 2's, at the forward NoF's first weight):
      "f32"     joint 1.43e-7 (floor 6.9e-8), alphas_mask alone 1.67e-7 (1.63e-7), stage 2 6.7e-8 (6.8e-8)
      "bf16x3"  joint 1.38e-7 (floor 7.1e-8), alphas_mask alone 2.57e-7 (8.9e-8), stage 2 5.8e-8 (6.0e-8)
    so every tensor is inside the 1e-6 arm of the bar.  That rests on the seeds: mf_point_loss_partials_backward rounds every
    step where torch's device kernels round it (test_point_loss_seeds_bit_identical_to_torch_on_the_device), so each row enters
    the networks' backward with the very bits the compacted path gives it and only the weight gradients' summation order
    differs.  With seeds a last bit off (sum / count as a true division, a z / (z + 1) as a (z / (z + 1))) the backward NoF's
    gradients behind the mask loss differed by up to 1.6e-6 ("f32") and 7.0e-6 ("bf16x3")."""
    S, c = M.supervision, smpl_case()
    g = torch.Generator(device="cuda").manual_seed(3)
    corr = S.correspondence(c["smpl"], c["pose"][:1], c["betas"][:1], c["pose"][1:], c["betas"][1:], 150, thickness=0.2, generator=g)
    ins, outs = corr.split()
    print(f"inside {ins.shape[0]}, outside {outs.shape[0]}")
    assert ins.shape[0] > 20 and outs.shape[0] > 20
    flip = lambda t: t.flip(0).contiguous()
    bad = _compare("joint", _masked_step(M, corr), _parent_step(ins, outs), _parent_step(flip(ins), flip(outs)))
    # only_msk_loss: the forward NoF is not part of the step
    got = _masked_step(M, corr, terms=("alphas_mask",))
    assert all(x is None for x in got[1]["fw"]) and set(got[0]) == {"alphas_mask"}
    bad += _compare("only_msk", got, _parent_step(ins, outs, only_msk=True), _parent_step(flip(ins), flip(outs), only_msk=True))
    # stage 2: both sets, no NeRF
    bw, fw, nerf, nof_embs, nxyz = nets()
    for m in (bw, fw, nerf):
        m.zero_grad(set_to_none=True)
    losses = M.point_losses(corr, IND, bw, fw, nof_embs, terms=("nof_bw", "nof_fw"), all_points=True)
    sum(losses.values()).backward()
    got = ({k: float(v) for k, v in losses.items()},
           {name: [None if p.grad is None else p.grad.clone() for p in m.parameters()] for name, m in (("bw", bw), ("fw", fw), ("nerf", nerf))})
    bad += _compare("stage 2", got, _parent_step(ins, outs, stage2=True), _parent_step(flip(outs), flip(ins), stage2=True))
    # fw_nof = None drops nof_fw
    assert set(M.point_losses(corr, IND, bw, None, nof_embs, terms=("nof_bw", "nof_fw"))) == {"nof_bw"}
    assert not bad, bad                                     # (tag, module, tensor, difference, floor) of every tensor over its bar


# ---- 7. no host synchronisation ---------------------------------------------------------------------------------------

def test_no_host_sync(M):
    """Under torch.cuda.set_sync_debug_mode("error") the draws, the correspondence, the losses and the backward run clean;
    Correspondence.split() -- the compaction -- raises."""
    S, c = M.supervision, smpl_case()
    bw, fw, nerf, nof_embs, nxyz = nets()
    g = torch.Generator(device="cuda").manual_seed(9)
    args = (c["smpl"], c["pose"][:1], c["betas"][:1], c["pose"][1:], c["betas"][1:], 150)

    def step():
        for m in (bw, fw, nerf):
            m.zero_grad(set_to_none=True)
        corr = S.correspondence(*args, thickness=0.2, generator=g)
        losses = M.point_losses(corr, IND, bw, fw, nof_embs, nerfs=(nerf,), nerf_embedding_xyz=nxyz, deltas=(DELTA,))
        (losses["nof_bw"] + losses["nof_fw"] + 0.5 * losses["alphas_mask"]).backward()
        return corr

    step()                                                  # warm: packed weights, descriptors, allocator
    torch.cuda.synchronize()
    probe = torch.ones(1, device="cuda")
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            detects = False
        except RuntimeError:
            detects = True
        if detects:
            corr = step()
            with pytest.raises(RuntimeError):
                corr.split()
    finally:
        torch.cuda.set_sync_debug_mode(old)
    if not detects:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not make .item() raise on this build")
    torch.cuda.synchronize()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in bw.parameters())
