"""The coloured-mesh path on the MI355X: query_radiance (mf_points_radiance) against the CPU oracle around the 128-point
tile and past the first trip of the persistent loop, vertex_normals (mf_mc_normals) against the numpy oracle of its contract
(tests/mesh_color_oracle.py), extract_colored_mesh against extract_mesh / vertex_normals / the oracle, determinism."""
import functools
import os

import numpy as np
import pytest
import torch

import mc_oracle as O
import mesh_color_oracle as N

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = np.load(os.path.join(HERE, "golden", "m_mesh.npz"))

pytestmark = pytest.mark.gpu

TOL = 1e-4                       # the package's fp32 contract, max|a - b| / max|b|
TILE = 128                       # points per workgroup trip (kTile)
BLOCKS_PER_CU = 1                # persistent_grid (mf_host.hpp): at most one workgroup per CU
# 4 x the largest componentwise gap between the float32 and the float64 evaluation of the numpy oracle on NORMAL_CASES
# (vertices whose float64 |g| is above 1e-3 of the volume's value range): measured 1.316e-7 (noncubic) on the CPU by
# tests/test_mesh_color_cpu.py::test_normals_fixture_list_and_tolerance, which holds this figure to the measurement
NORMALS_TOL = 5.3e-7
NORMAL_CASES = (("ball", False), ("noncubic", False), ("boundary", False), ("noise", False), ("noise", True))
# what INTEGRATION.md says about extract_mesh's winding and the normals (test_winding_against_normals_on_the_ball)
WINDING_SENTENCE = "opposite to the triangles' right-hand face normals"
WINDING_SIGN = -1


@pytest.fixture(scope="module")
def M():
    import moco_flow_amd
    return moco_flow_amd


@pytest.fixture(scope="module")
def R():
    from oracle import cpu_ref
    return cpu_ref


def relerr(a, b):
    a, b = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max())


# ---------------------------------------------------------------- radiance against the oracle
def second_trip_points():
    """Smallest point count at which one workgroup of the persistent launch takes a second trip: one tile more than the
    grid has workgroups, and one point into the tile after it (a ragged last tile): (CUs x blocks per CU + 1) x 128 + 1."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return (cus * BLOCKS_PER_CU + 1) * TILE + 1


def load(module, sd):
    module.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return module.cuda()


NETWORKS = ("ind_canonical", "ind_nof_scalar", "ind_nof_tensor", "dir", "none")
IND_SCALAR = float(np.float32(17 * 2 / 300 - 1.0))


@functools.lru_cache(maxsize=None)
def radiance_case(name):
    """Models, inputs and the oracle's answer for one network at the largest size, computed once; the smaller sizes are
    prefixes (every point is independent)."""
    import moco_flow_amd as M
    from moco_flow_amd import synth
    from oracle import cpu_ref as R
    B = second_trip_points()
    seed = NETWORKS.index(name)
    g = torch.Generator().manual_seed(100 + seed)
    xyz = torch.rand(B, 3, generator=g) * 3 - 1.5
    kind, dim = {"dir": ("dir", 27), "none": ("none", 0)}.get(name, ("ind", 5))
    sd = synth.nerf_state(50 + seed, extra_feat_type=kind, extra_feat_dim=dim, regime="dense", tag="rad")
    nerf = load(M.NeRF(8, 256, 63, [4], kind, dim), sd)
    embs = [M.Embedding(3, 10), M.Embedding(1, 2) if kind == "ind" else None, M.Embedding(3, 4) if kind == "dir" else None]
    onerf = R.NeRF(8, 256, 63, [4], kind, dim, state=sd)
    kw, ind, dirs, canon = {}, None, None, None
    pts = xyz
    with torch.no_grad():
        if kind == "ind":
            ind = torch.full((B,), IND_SCALAR)
            if name == "ind_nof_tensor":
                ind = torch.rand(B, generator=g) * 2 - 1
            kw["ind"] = ind if name == "ind_nof_tensor" else IND_SCALAR
        if "nof" in name:
            sdf = synth.nof_state(60 + seed, use_quat=True, tag="rad", head_scale=0.25)
            kw.update(bw_nof=load(M.NoF(4, 128, 33, [2], "ind", 33, True), sdf), nof_embeddings=[M.Embedding(3, 5), M.Embedding(1, 16)])
            onof = R.NoF(4, 128, 33, [2], "ind", 33, True, state=sdf)
            inp = torch.cat([R._embed_padded(R.Embedding(3, 5), xyz, 33), R._embed_padded(R.Embedding(1, 16), ind[:, None], 33)], -1)
            pts = canon = onof(inp, xyz)
        inp = R._embed_padded(R.Embedding(3, 10), pts, 63)
        if kind == "ind":
            inp = torch.cat([inp, R._embed_padded(R.Embedding(1, 2), ind[:, None], dim)], -1)
        if kind == "dir":
            dirs = torch.randn(B, 3, generator=g)
            unit = torch.arange(B) % 2 == 0                          # every other row a unit vector, the rest as drawn
            dirs[unit] = dirs[unit] / dirs[unit].norm(dim=1, keepdim=True)     # (lengths ~0.1 .. 3: nothing normalises them)
            kw["view_dirs"] = dirs
            inp = torch.cat([inp, R._embed_padded(R.Embedding(3, 4), dirs, dim)], -1)
        want = onerf(inp)                                            # (B, 4) [rgb | sigma]
    return dict(B=B, xyz=xyz, nerf=nerf, embs=embs, kw=kw, want=want, canon=canon)


def device_kw(kw, B):
    out = dict(kw)
    for k in ("ind", "view_dirs"):
        if torch.is_tensor(out.get(k)):
            out[k] = out[k][:B].cuda()
    return out


def sizes():
    return (1, TILE - 1, TILE, TILE + 1, second_trip_points())


@pytest.mark.parametrize("name", NETWORKS)
def test_radiance_matches_the_oracle(M, name):
    c = radiance_case(name)
    nerf, embs = c["nerf"], c["embs"]
    for B in sizes():
        xyz = c["xyz"][:B].cuda()
        kw = device_kw(c["kw"], B)
        with torch.no_grad():
            out = M.query_radiance(xyz, nerf, embs, return_canonical=True, **kw)
            out, canon = out
            nof_kw = {k: kw[k] for k in ("bw_nof", "nof_embeddings", "ind") if k in kw and "bw_nof" in kw}
            sigma = M.query_sigma(xyz, nerf, embs[0], precision="f32", **nof_kw)
        torch.cuda.synchronize()
        assert out.shape == (B, 4) and out.dtype == torch.float32 and out.is_cuda
        want = c["want"][:B]
        e_rgb, e_sigma = relerr(out[:, :3], want[:, :3]), relerr(out[:, 3], want[:, 3])
        gap = relerr(out[:, 3:4], sigma)
        line = f"{name} B={B}: rgb max-rel {e_rgb:.2e}, sigma max-rel {e_sigma:.2e}, sigma gap to query_sigma {gap:.2e}"
        if c["canon"] is not None:
            e_canon = relerr(canon, c["canon"][:B])
            line += f", canonical point max-rel {e_canon:.2e}"
        print(line)
        assert e_rgb <= TOL and e_sigma <= TOL and gap <= TOL
        if c["canon"] is not None:
            assert canon.shape == (B, 3) and e_canon <= TOL
        else:
            assert canon is None
        if B == sizes()[-1]:                                          # a second run of the largest launch: bit-identical
            with torch.no_grad():
                again = M.query_radiance(xyz, nerf, embs, **kw)
            assert torch.equal(out, again)


def test_scalar_and_tensor_index_agree(M):
    """A python float, a (1,) tensor, a (B,) and a (B, 1) tensor of the same value give the same bits."""
    c = radiance_case("ind_nof_scalar")
    B = 300
    xyz = c["xyz"][:B].cuda()
    kw = {k: v for k, v in c["kw"].items() if k != "ind"}
    with torch.no_grad():
        a = M.query_radiance(xyz, c["nerf"], c["embs"], ind=IND_SCALAR, **kw)
        for ind in (torch.tensor([IND_SCALAR]), torch.full((B,), IND_SCALAR).cuda(), torch.full((B, 1), IND_SCALAR)):
            assert torch.equal(a, M.query_radiance(xyz, c["nerf"], c["embs"], ind=ind, **kw))


def test_radiance_empty_and_argument_errors(M):
    c = radiance_case("dir")
    nerf, embs = c["nerf"], c["embs"]
    empty = torch.zeros(0, 3, device="cuda")
    out = M.query_radiance(empty, nerf, embs, view_dirs=empty)
    assert out.shape == (0, 4) and out.dtype == torch.float32 and out.is_cuda
    xyz = c["xyz"][:10].cuda()
    with pytest.raises(RuntimeError, match="view_dirs"):
        M.query_radiance(xyz, nerf, embs)
    with pytest.raises(RuntimeError, match="view_dirs"):
        M.query_radiance(xyz, nerf, embs, view_dirs=torch.zeros(9, 3, device="cuda"))
    ci = radiance_case("ind_nof_scalar")
    kw = {k: v for k, v in ci["kw"].items() if k != "ind"}
    with pytest.raises(RuntimeError, match="ind"):
        M.query_radiance(xyz, ci["nerf"], ci["embs"])                                  # an "ind" NeRF without ind
    with pytest.raises(RuntimeError, match="ind"):
        M.query_radiance(xyz, radiance_case("none")["nerf"], radiance_case("none")["embs"], **kw)   # a NoF without ind
    with pytest.raises(RuntimeError, match="elements"):
        M.query_radiance(xyz, ci["nerf"], ci["embs"], ind=torch.zeros(7), **kw)
    out = M.query_radiance(torch.zeros(0, 3, device="cuda"), ci["nerf"], ci["embs"], ind=0.25, **kw)
    assert out.shape == (0, 4)


# ---------------------------------------------------------------- normals against the numpy oracle
@functools.lru_cache(maxsize=None)
def normals_case(name, clamp):
    """(volume, marching-cubes vertices, mask of the vertices compared to tolerance, float32-vs-float64 gap of the oracle on
    them).  CPU only: tests/test_mesh_color_cpu.py checks the fixture list and NORMALS_TOL with it."""
    vol, iso = GOLD[name + "_vol"], float(GOLD[name + "_iso"])
    verts, _ = O.marching_cubes(vol, iso, clamp)
    g64 = N.gradient_at(vol, verts, clamp, np.float64)
    keep = np.linalg.norm(g64, axis=1) > 1e-3 * (float(vol.max()) - float(vol.min()))
    n32, n64 = N.normals(vol, verts, clamp, np.float32), N.normals(vol, verts, clamp, np.float64)
    gap = float(np.abs(n32.astype(np.float64) - n64)[keep].max())
    return vol, verts, keep, gap


@pytest.mark.parametrize("name,clamp", NORMAL_CASES)
def test_normals_match_the_oracle(M, name, clamp):
    """Tolerance NORMALS_TOL = 5.3e-7: four times the float32-vs-float64 gap of the oracle itself on these inputs (1.316e-7
    on noncubic, 1.05e-7 .. 1.23e-7 on the others, measured on the CPU; no vertex of any fixture is left out), because the kernel may fuse multiply-adds and use a hardware reciprocal square root.  Vertices with
    a float64 gradient under 1e-3 of the value range (at most 1 % of a fixture; their direction is ill-conditioned) are only
    required to be finite and of length 0 or 1."""
    vol, verts, keep, gap = normals_case(name, clamp)
    with torch.no_grad():
        got = M.vertex_normals(torch.from_numpy(vol).cuda(), torch.from_numpy(verts).cuda(), clamp_zero=clamp)
        again = M.vertex_normals(torch.from_numpy(vol).cuda(), torch.from_numpy(verts).cuda(), clamp_zero=clamp)
    torch.cuda.synchronize()
    assert got.shape == verts.shape and got.dtype == torch.float32 and got.is_cuda
    assert torch.equal(got, again)
    got = got.cpu().numpy()
    want = N.normals(vol, verts, clamp, np.float32)
    err = float(np.abs(got.astype(np.float64) - want)[keep].max())
    print(f"{name} clamp={clamp}: V {len(verts)}, max gap to the oracle {err:.2e} (oracle float32-float64 {gap:.2e}, "
          f"tolerance {NORMALS_TOL:.2e}), bit-equal {np.array_equal(got, want)}, left out {int((~keep).sum())}")
    assert err <= NORMALS_TOL
    rest = got[~keep].astype(np.float64)
    assert np.isfinite(rest).all()
    length = np.linalg.norm(rest, axis=1)
    assert np.all((length == 0) | (np.abs(length - 1) <= NORMALS_TOL))


def test_normals_on_plateaus_are_exactly_zero(M):
    """A volume that is constant where it is positive: with clamp_zero its two plateaus (the constant, and the clamped
    negative part) have no gradient, on lattice points and on edges alike; without the clamp the negative part has one."""
    rng = np.random.default_rng(11)
    vol = (-0.1 - np.abs(rng.standard_normal((20, 22, 24)))).astype(np.float32)
    vol[6:15, 6:15, 6:15] = 5.0
    inside = 8 + 4 * rng.random((200, 3))                                  # stencils stay in [7, 13]
    inside[::3] = np.floor(inside[::3])                                    # some exactly on lattice points
    outside = 1 + 3 * rng.random((200, 3))                                 # stencils stay in [0, 5]
    outside[::3] = np.floor(outside[::3])
    pts = np.concatenate([inside, outside]).astype(np.float32)
    pts[1::3, 1:] = np.floor(pts[1::3, 1:])                                # and some on lattice edges
    v, p = torch.from_numpy(vol).cuda(), torch.from_numpy(pts).cuda()
    clamped = M.vertex_normals(v, p, clamp_zero=True).cpu()
    assert torch.equal(clamped, torch.zeros(400, 3))
    assert np.array_equal(N.normals(vol, pts, True), np.zeros((400, 3), np.float32))
    plain = M.vertex_normals(v, p).cpu()
    assert torch.equal(plain[:200], torch.zeros(200, 3))
    assert (np.abs(np.linalg.norm(plain[200:].numpy().astype(np.float64), axis=1) - 1) <= NORMALS_TOL).all()
    # the marching-cubes vertices of the box's surface carry unit normals that leave the box
    verts, _ = M.marching_cubes(v, 2.5, clamp_zero=True)
    nn = M.vertex_normals(v, verts, clamp_zero=True)
    outward = ((verts - 10.0) * nn).sum(1)
    assert len(verts) > 0 and bool((outward > 0).all())
    assert M.vertex_normals(v, torch.zeros(0, 3, device="cuda")).shape == (0, 3)


def test_winding_against_normals_on_the_ball(M):
    """marching_cubes + extract_mesh's post-processing on the ball: face_normal . vertex_normal has one sign for every
    triangle, the one INTEGRATION.md states."""
    vol = torch.from_numpy(GOLD["ball_vol"]).cuda()
    raw, tris = M.marching_cubes(vol, float(GOLD["ball_iso"]))
    normals = M.vertex_normals(vol, raw)[:, [1, 0, 2]].double().cpu()
    n = vol.shape[0]
    verts = (raw[:, [1, 0, 2]] / n * 3.0 - 1.5).double().cpu()             # extract_mesh's post-processing
    tris = tris[:, [0, 2, 1]].cpu()
    a, b, c = verts[tris[:, 0]], verts[tris[:, 1]], verts[tris[:, 2]]
    face = torch.linalg.cross(b - a, c - a)
    dots = (face * (normals[tris[:, 0]] + normals[tris[:, 1]] + normals[tris[:, 2]])).sum(1)
    signs = torch.sign(dots)
    print(f"ball: {len(tris)} triangles, face . vertex normal signs {sorted(set(signs.tolist()))}")
    assert len(tris) > 0 and bool((signs == WINDING_SIGN).all())
    text = " ".join(open(os.path.join(ROOT, "INTEGRATION.md")).read().split())
    assert WINDING_SENTENCE in text


# ---------------------------------------------------------------- extract_colored_mesh
def mesh_models(M, with_nof):
    """The NeRF of tests/test_gpu_mesh.py (raw sigma crosses 10) and its backward flow."""
    from moco_flow_amd import synth
    sd = synth.nerf_state(0, extra_feat_type="ind", extra_feat_dim=5, regime="dense")
    sd["sigma.weight"] = sd["sigma.weight"] * np.float32(3.0)
    out = dict(nerf=load(M.NeRF(8, 256, 63, [4], "ind", 5), sd), embs=[M.Embedding(3, 10), M.Embedding(1, 2), None], sd=sd)
    if with_nof:
        sdf = synth.nof_state(1, use_quat=True, tag="bw", head_scale=0.25)
        out.update(nof=load(M.NoF(4, 128, 33, [2], "ind", 33, True), sdf), nof_embs=[M.Embedding(3, 5), M.Embedding(1, 16)], sdf=sdf)
    return out


@pytest.mark.parametrize("with_nof", [False, True])
def test_extract_colored_mesh(M, R, with_nof):
    Ng = 32
    m = mesh_models(M, with_nof)
    kw = dict(bw_nof=m["nof"], nof_embeddings=m["nof_embs"]) if with_nof else {}
    with torch.no_grad():
        verts, tris, normals, colors = M.extract_colored_mesh(m["nerf"], m["embs"], N_grid=Ng, sigma_threshold=10, ind=IND_SCALAR, **kw)
        v0, t0 = M.extract_mesh(m["nerf"], m["embs"][0], N_grid=Ng, sigma_threshold=10, ind=IND_SCALAR, **kw)
        sigma = M.query_sigma(M.mesh.lattice(Ng, verts.device), m["nerf"], m["embs"][0], ind=IND_SCALAR, **kw).view(Ng, Ng, Ng)
        raw, _ = M.marching_cubes(sigma, 10, clamp_zero=True)
        n0 = M.vertex_normals(sigma, raw, clamp_zero=True)[:, [1, 0, 2]]
        again = M.extract_colored_mesh(m["nerf"], m["embs"], N_grid=Ng, sigma_threshold=10, ind=IND_SCALAR, **kw)
    V = len(verts)
    assert V > 0 and len(tris) > 0
    assert torch.equal(verts, v0) and torch.equal(tris, t0)
    assert normals.shape == (V, 3) and colors.shape == (V, 3) and colors.dtype == torch.float32 and colors.is_cuda
    assert torch.equal(normals, n0)
    for x, y in zip((verts, tris, normals, colors), again):
        assert torch.equal(x, y)
    # colours: the oracle's NeRF.forward at the returned vertices
    pts = verts.cpu()
    ind = torch.full((V, 1), IND_SCALAR)
    with torch.no_grad():
        if with_nof:
            onof = R.NoF(4, 128, 33, [2], "ind", 33, True, state=m["sdf"])
            inp = torch.cat([R._embed_padded(R.Embedding(3, 5), pts, 33), R._embed_padded(R.Embedding(1, 16), ind, 33)], -1)
            pts = onof(inp, pts)
        inp = torch.cat([R._embed_padded(R.Embedding(3, 10), pts, 63), R._embed_padded(R.Embedding(1, 2), ind, 5)], -1)
        want = R.NeRF(8, 256, 63, [4], "ind", 5, state=m["sd"])(inp)
    err = relerr(colors, want[:, :3])
    print(f"extract_colored_mesh {'bw NoF' if with_nof else 'canonical'}: V {V} T {len(tris)}, colour max-rel to the oracle {err:.2e}")
    assert err <= TOL
    # above the volume's maximum: four empty tensors
    with torch.no_grad():
        e = M.extract_colored_mesh(m["nerf"], m["embs"], N_grid=Ng, sigma_threshold=float(sigma.max()) + 1.0, ind=IND_SCALAR, **kw)
    assert [tuple(x.shape) for x in e] == [(0, 3)] * 4
    assert e[0].dtype == torch.float32 and e[1].dtype == torch.int64 and all(x.is_cuda for x in e)


def test_colored_mesh_of_a_dir_nerf_looks_along_the_normal(M):
    """A "dir" NeRF is queried with view_dirs = -normal, (0, 0, -1) where the normal is zero."""
    from moco_flow_amd import synth
    sd = synth.nerf_state(0, regime="dense")
    sd["sigma.weight"] = sd["sigma.weight"] * np.float32(3.0)
    nerf = load(M.NeRF(8, 256, 63, [4], "dir", 27), sd)
    embs = [M.Embedding(3, 10), None, M.Embedding(3, 4)]
    with torch.no_grad():
        verts, tris, normals, colors = M.extract_colored_mesh(nerf, embs, N_grid=32, sigma_threshold=10)
        assert len(verts) > 0
        dirs = -normals
        dirs[(normals == 0).all(1)] = torch.tensor([0.0, 0.0, -1.0], device="cuda")
        want = M.query_radiance(verts, nerf, embs, view_dirs=dirs)[:, :3]
    assert torch.equal(colors, want)
