"""Device marching cubes (moco_flow_amd.mesh, mf_mc_*) on the MI355X: bit for bit against the numpy oracle of its contract
(tests/mc_oracle.py), as sets against scikit-image's Lorensen meshes (tests/golden/m_mesh.npz), determinism, edge cases,
one 512^3 volume, and extract_mesh against visualize_mesh's pipeline restated on the CPU."""
import os

import numpy as np
import pytest
import torch

import mc_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "m_mesh.npz"))
NAMES = ("ball", "torus", "noise", "noncubic", "boundary", "nerf")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M():
    import moco_flow_amd
    return moco_flow_amd


def run(M, vol, iso, clamp=False):
    v, t = M.marching_cubes(torch.from_numpy(np.ascontiguousarray(vol)).cuda(), iso, clamp_zero=clamp)
    torch.cuda.synchronize()
    assert v.dtype == torch.float32 and t.dtype == torch.int64 and v.is_cuda and t.is_cuda
    return v.cpu(), t.cpu()


def ulp_close(a, b):
    """a == b bitwise, or at worst 1 ulp apart (fp32)."""
    a, b = a.numpy(), np.asarray(b, np.float32)
    if a.shape != b.shape:
        return False
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    return bool(np.all(np.abs(ia - ib) <= 1))


def assert_equals_oracle(M, vol, iso, clamp=False, what=""):
    v, t = run(M, vol, iso, clamp)
    ov, ot = O.marching_cubes(vol, iso, clamp)
    assert t.shape == ot.shape and torch.equal(t, torch.from_numpy(ot)), what
    assert ulp_close(v, ov), what
    exact = torch.equal(v, torch.from_numpy(ov))
    return v, t, exact


@pytest.mark.parametrize("name", NAMES)
def test_fixtures_equal_oracle_and_skimage(M, name):
    vol, iso, clamp = GOLD[name + "_vol"], float(GOLD[name + "_iso"]), bool(GOLD[name + "_clamp"])
    v, t, exact = assert_equals_oracle(M, vol, iso, clamp, name)
    print(f"{name}: V {len(v)} T {len(t)}, vertices bit-exact: {exact}")
    ok, msg = O.same_mesh_as_sets(v.numpy(), t.numpy(), GOLD[name + "_verts"], GOLD[name + "_faces"])
    assert ok, f"{name}: {msg}"


@pytest.mark.parametrize("shape,iso,clamp", [((9, 11, 13), 0.0, False), ((7, 5, 64), 0.3, False), ((40, 37, 64), -0.1, False),
                                             ((33, 29, 31), 0.25, True), ((3, 2, 1027), 0.0, False), ((64, 2, 3), 0.5, True),
                                             ((5, 7, 30000), 0.8, False), ((3, 5, 70001), 0.8, False)])
def test_random_volumes_equal_oracle(M, shape, iso, clamp):
    """White noise: every case, many blocks (> 1024 points), rows of n2 % 4 == 0 (float4 loads) and not.  The last two hold
    1026 blocks: the scan workgroup's 1024 threads take a ragged share of the block totals (2 each, threads 0-512 only)."""
    vol = np.random.default_rng(sum(shape)).standard_normal(shape).astype(np.float32)
    v, t, exact = assert_equals_oracle(M, vol, iso, clamp, str(shape))
    assert len(t) > 0


def test_all_cases_volume(M):
    vol = O.all_cases_volume()
    v, t, _ = assert_equals_oracle(M, vol, 0.0)
    assert len(t) >= 820


def test_every_case_on_the_smallest_volume(M):
    for case in range(256):
        vol = O.all_cases_volume(seed=case)[:, :, 2 * case:2 * case + 2].copy()
        v, t, _ = assert_equals_oracle(M, vol, 0.0, what=f"case {case}")
        assert len(t) == O.NTRI[case]


def test_repeat_runs_bit_identical(M):
    vol = torch.from_numpy(GOLD["nerf_vol"]).cuda()
    noise = torch.from_numpy(np.random.default_rng(3).standard_normal((48, 40, 36)).astype(np.float32)).cuda()
    for x, iso, clamp in ((vol, 10.0, True), (noise, 0.0, False)):
        a = M.marching_cubes(x, iso, clamp)
        for _ in range(3):
            b = M.marching_cubes(x, iso, clamp)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_empty_and_all_inside(M):
    for fill in (1.0, -1.0):                              # nothing below / everything below: no surface
        v, t = run(M, np.full((17, 9, 12), fill, np.float32), 0.0)
        assert v.shape == (0, 3) and t.shape == (0, 3)
    v, t = run(M, np.zeros((2, 2, 2), np.float32), 0.0)  # all exactly at the isovalue: not below -> empty
    assert len(v) == 0 and len(t) == 0


def test_clamp_zero(M):
    vol = np.random.default_rng(9).standard_normal((21, 18, 16)).astype(np.float32)
    for iso in (0.5, 1e-3):
        v, t, _ = assert_equals_oracle(M, vol, iso, True)
        ov, ot = O.marching_cubes(np.maximum(vol, 0), iso)
        assert torch.equal(t, torch.from_numpy(ot)) and ulp_close(v, ov)


def test_non_contiguous_and_non_fp32_input(M):
    vol = np.random.default_rng(4).standard_normal((12, 10, 14)).astype(np.float32)
    x = torch.from_numpy(vol).cuda()
    xt = x.permute(2, 0, 1)                               # a view: copied to a contiguous volume of its own shape
    v, t = M.marching_cubes(xt, 0.1)
    ov, ot = O.marching_cubes(np.ascontiguousarray(vol.transpose(2, 0, 1)), 0.1)
    assert torch.equal(t.cpu(), torch.from_numpy(ot)) and ulp_close(v.cpu(), ov)
    v2, t2 = M.marching_cubes(x.double(), 0.1)
    ov, ot = O.marching_cubes(vol, 0.1)
    assert torch.equal(t2.cpu(), torch.from_numpy(ot)) and ulp_close(v2.cpu(), ov)


def test_bad_shapes_rejected(M):
    for shape in [(1, 4, 4), (4, 4, 1), (4, 4)]:
        with pytest.raises(RuntimeError):
            M.marching_cubes(torch.zeros(shape, device="cuda"), 0.0)
    huge = torch.zeros(1, device="cuda").expand(2048, 2048, 1024)   # 2^32 points, never materialised
    with pytest.raises(RuntimeError, match="2\\^31"):
        M.marching_cubes(huge, 0.0)


def test_512_cubed(M):
    """One 512^3 volume, run once: the counts and a slab of rows match the oracle exactly."""
    N = 512
    ax = torch.linspace(0, 1, N, device="cuda")
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    vol = (torch.sin(23.0 * x + 3.0 * y * y) + torch.sin(17.0 * y + 5.0 * z) + torch.sin(29.0 * z + 7.0 * x * y)).contiguous()
    del x, y, z
    v, t = M.marching_cubes(vol, 0.3)
    torch.cuda.synchronize()
    h = vol.cpu().numpy()
    V, T = O.counts(h, 0.3)
    print(f"512^3: V {len(v)} T {len(t)}")
    assert (len(v), len(t)) == (V, T) and T > 0
    sv, st, V0, T0 = O.slab(h, 0.3, 250, 258)
    assert torch.equal(t[T0:T0 + len(st)].cpu(), torch.from_numpy(st))
    assert ulp_close(v[V0:V0 + len(sv)].cpu(), sv)


# ---- extract_mesh against visualize_mesh (trainer_moco_flow.py:490-538) restated on the CPU
def reference_pipeline(sigma, N, threshold=10.0):
    """max(sigma, 0) -> marching cubes (the oracle) -> the reference's post-processing, in float64 as numpy does it."""
    verts, tris = O.marching_cubes(np.maximum(sigma.reshape(N, N, N), 0), threshold)
    verts = verts.astype(np.float64)
    verts[:, [0, 1]] = verts[:, [1, 0]]
    tris[:, [0, 1, 2]] = tris[:, [0, 2, 1]]
    return verts / N * 3.0 - 1.5, tris


def mesh_models(M, with_nof):
    from moco_flow_amd import synth
    sd = synth.nerf_state(0, extra_feat_type="ind", extra_feat_dim=5, regime="dense")
    sd["sigma.weight"] = sd["sigma.weight"] * np.float32(3.0)          # raw sigma then crosses 10 (mesh_golden's NeRF)
    nerf = M.NeRF(8, 256, 63, [4], "ind", 5)
    nerf.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    out = dict(nerf=nerf.cuda(), emb=M.Embedding(3, 10), sd=sd)
    if with_nof:
        sdf = synth.nof_state(1, use_quat=True, tag="bw", head_scale=0.25)
        nof = M.NoF(4, 128, 33, [2], "ind", 33, True)
        nof.load_state_dict({k: torch.from_numpy(v) for k, v in sdf.items()})
        out.update(nof=nof.cuda(), nof_embs=[M.Embedding(3, 5), M.Embedding(1, 16)], sdf=sdf)
    return out


@pytest.mark.parametrize("with_nof", [False, True])
@pytest.mark.parametrize("precision", ["f32", "bf16", "bf16x3"])
def test_extract_mesh_matches_reference_pipeline(M, with_nof, precision):
    from oracle import cpu_ref as R
    N, frame, num_frames = 32, 17, 300
    ind = frame * 2 / num_frames - 1.0
    m = mesh_models(M, with_nof)
    x = np.linspace(-1.5, 1.5, N)
    xyz = torch.FloatTensor(np.stack(np.meshgrid(x, x, x), -1).reshape(-1, 3))     # visualize_mesh:490-497
    kw = dict(bw_nof=m["nof"], nof_embeddings=m["nof_embs"], ind=ind) if with_nof else {}
    with torch.no_grad():
        verts, tris = M.extract_mesh(m["nerf"], m["emb"], N_grid=N, sigma_threshold=10, precision=precision, **kw)
        sigma = M.query_sigma(xyz.cuda(), m["nerf"], m["emb"], precision=precision, **kw).cpu().numpy()
    assert verts.is_cuda and verts.dtype == torch.float32 and tris.dtype == torch.int64
    rv, rt = reference_pipeline(sigma, N)
    assert len(rt) > 0
    assert torch.equal(tris.cpu(), torch.from_numpy(rt))
    gap = float(np.abs(verts.cpu().numpy().astype(np.float64) - rv).max())
    print(f"extract_mesh {precision} {'bw NoF' if with_nof else 'canonical'}: V {len(verts)} T {len(tris)}, "
          f"vertex gap to the restated pipeline {gap:.2e}")
    assert gap <= 2e-6
    if precision == "f32":
        # the sigma that pipeline was fed is the oracle's within the package's 1e-4 max-rel contract
        onerf = R.NeRF(8, 256, 63, [4], "ind", 5, state=m["sd"])
        with torch.no_grad():
            pts = xyz
            if with_nof:
                onof = R.NoF(4, 128, 33, [2], "ind", 33, True, state=m["sdf"])
                pts = R.forward_nof_points(xyz, torch.tensor([frame]), num_frames, R.Embedding(3, 5), R.Embedding(1, 16), onof)
            osig = onerf(R.Embedding(3, 10)(pts), sigma_only=True).numpy()
        err = float(np.abs(sigma - osig).max() / np.abs(osig).max())
        ov, ot = reference_pipeline(osig, N)
        print(f"  sigma max-rel to the CPU oracle {err:.2e}; mesh from the oracle's sigma: V {len(ov)} T {len(ot)}")
        assert err <= 1e-4
