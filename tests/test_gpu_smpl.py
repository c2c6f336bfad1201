"""The SMPL unit (csrc/mf_smpl.hip: mf_smpl_lbs, mf_smpl_frame_transforms, mf_apply_vertex_transforms) against the float64 oracle
of tests/smpl_oracle.py at the edges of its launches (-m gpu).  tests/test_smpl_oracle_cpu.py holds the preconditions.

Bars.  helpers.relerr (max |a - b| / max |b|) against the float64 oracle.  The yardstick of one tensor of one case is the larger
of fp32 oracle/smpl_ref.py's own distance from float64 on the same inputs and the median of that distance over this file's
cases (smpl_oracle.bar); the kernel must lie within 3 x the yardstick -- its FMA chains, 256-way strided joint sums and wave
shuffles are a different but equally good order of the same additions -- and never above the existing contract (1e-5 verts and
T, 1e-4 trans and cano).  No number here is read off the kernel.

  (1) mf_smpl_lbs against the oracle: V in {1, 2, 3, 4, 5, 255, 256, 257, 431, 6890} (one wave per vertex, four per workgroup;
      256-wide joint and shape strides); standard / chain / star trees at pose scales 0.6 and 2.5; all 24 joints at pi,
      pi - 1e-4, 2 pi, 1e-4, 1e-7, 3e-9 and the zero pose, as one B = 7 launch and row by row; rotation-matrix input, one view
      non-contiguous; B = 65535 (grid.y's limit) at V = 3, every row; B = 65536 refused.
  (2) exact: a row of a batch = its B = 1 launch; verts and T of one raw-ABI launch = the two single-output launches; the last
      row of T; a NaN row (theta + 1e-8 == 0 in fp32: the reference's rule) stays in its row; repeats; host refusals.
  (3) mf_smpl_frame_transforms: per-vertex error in units of cond2(T_src) * 2^-24 (smpl_oracle.normalised_inverse_error), the
      kernel's worst at most 3 x the worst of the fp32 reference expression `T_tgt @ torch.inverse(T_src)` over the buckets
      rigid, blend, c30, c300 (1000 matrices each); a bucket of full 4 x 4 matrices (last row not (0, 0, 0, 1), so every
      cofactor is live) to the same bar.  Bucket c3000 is measured and printed, NOT asserted: an adjugate inverse in fp32 loses to
      pivoted LU as the matrix nears singular -- that is the method, not a bug.  V in {0, 1, 127, 128, 129, 1000}; T_src = I;
      permuted and sliced launches; one singular vertex; the LBS pipeline's own T at V = 431 and 6890.
  (4) mf_apply_vertex_transforms: Q in {1, 255, 256, 257, 5000} x V in {1, 7, 6890}, ind (Q,) / (Q,1) / int32 with duplicates;
      permuted queries; row i = the Q = 1 launch; indices out of range clamp to 0 / V - 1 (the kernel clamps before it forms an
      address); frame_correspondence with every query inside and with every query outside.
  (5) the SMPL module's cached device copies follow every buffer (reassigned or edited in place, module on either device).

Measured on the MI355X (89 cases, 2 s in all; every test prints kernel, yardstick and ratio).  Kernel max-rel in yardsticks:
  verts  0.20 .. 1.10 (V sweep 0.26 .. 1.10, chain 0.73 .. 0.75, star 0.64 .. 0.67, special angles 1.06, rows 0.20 .. 1.06,
         rotation matrices 0.43, B = 65535 1.05); yardsticks 3.6e-7 .. 1.0e-6
  T      0.21 .. 1.35 (V sweep 0.82 .. 1.35, chain 0.88 .. 0.90, star 0.48 .. 0.64, special angles 0.74, B = 65535 0.86);
         yardsticks 4.2e-7 .. 1.1e-6
  cano   0.09 .. 1.10; yardsticks 7.7e-8 .. 1.0e-7
  trans, worst normalised error kernel / fp32 reference (bar 3 x 2.09 = 6.27): rigid 2.47 / 2.09, blend 2.37 / 1.76, c30 0.68 /
         0.57, c300 1.09 / 0.36, general 1.76 / 1.23, pipeline V = 431 2.98 / 1.78, V = 6890 3.11 / 2.39; c3000 4.13 / 0.37
         (max-rel 5.6e-4 / 5.2e-5: not asserted, see (3)); max-rel of the held buckets 1.7e-7 .. 1.8e-5
No case lies between 3 yardsticks and the contract: no bar falls back to the contract, and no kernel bug was found.
"""
import functools

import numpy as np
import pytest
import torch

import smpl_oracle as O
from helpers import relerr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M():
    import moco_flow_amd
    assert torch.cuda.is_available()
    moco_flow_amd._lib.lib()          # fail loudly if the HIP library is missing
    return moco_flow_amd


def _cu(a):
    return torch.as_tensor(a).cuda()


@functools.lru_cache(maxsize=None)
def _module(V, tree="standard"):
    from moco_flow_amd import smpl as S
    return S.SMPL(model=O.model(V, tree)).cuda()


def _forward(m, pose, betas):
    """(verts, T) of the module's two calls, on the host."""
    pose, betas = _cu(pose), _cu(betas)
    return m(pose, betas).cpu(), m.get_vertex_transformation(pose, betas).cpu()


@functools.lru_cache(maxsize=None)
def _got(name):
    c = O.lbs_cases()[name]
    return _forward(_module(c["V"], c["tree"]), c["pose"], c["betas"])


def _hold(label, kind, got, want, own, median):
    bar, yard = O.bar(kind, own, median)
    e = relerr(got, want)
    print(f"{label:24s} {kind:5s} kernel {e:.2e}  yardstick {yard:.2e}  ratio {e / yard:5.2f}  (bar {bar:.2e})")
    assert e <= bar, (label, kind, e, yard, bar)


# ------------------------------------------------------------------------------------------------ (1) mf_smpl_lbs vs the oracle
@pytest.mark.parametrize("name", list(O.lbs_cases()))
def test_lbs_vs_float64_oracle(M, name):
    per, med = O.lbs_yardsticks()
    verts, T = _got(name)
    want = O.lbs_oracle(name)
    assert torch.isfinite(verts).all() and torch.isfinite(T).all()
    _hold(name, "verts", verts, want["verts"], per[name]["verts"], med["verts"])
    _hold(name, "T", T, want["T"], per[name]["T"], med["T"])


def test_lbs_special_angles_row_by_row(M):
    """Each special-angle row as its own B = 1 launch: held to the oracle's row with that row's own yardstick, and bit-equal to
    the row of the B = 7 launch."""
    _, med = O.lbs_yardsticks()
    c, want = O.lbs_cases()["special"], O.lbs_oracle("special")
    v32, T32 = O.lbs_ref32("special")
    m = _module(c["V"], c["tree"])
    for r in range(7):
        verts, T = _forward(m, c["pose"][r:r + 1], c["betas"][r:r + 1])
        _hold(f"special row {r}", "verts", verts[0], want["verts"][r], relerr(v32[r], want["verts"][r]), med["verts"])
        _hold(f"special row {r}", "T", T[0], want["T"][r], relerr(T32[r], want["T"][r]), med["T"])
        assert torch.equal(verts[0], _got("special")[0][r]) and torch.equal(T[0], _got("special")[1][r]), r


def test_lbs_rotation_matrix_views(M):
    """(B,24,3,3) input through a non-contiguous view (every other column of a (B,24,3,6) buffer) = the contiguous launch."""
    c = O.lbs_cases()["rotmat"]
    wide = torch.zeros(3, 24, 3, 6)
    wide[..., ::2] = torch.from_numpy(c["pose"])
    view = wide.cuda()[..., ::2]
    assert not view.is_contiguous() and view.shape == (3, 24, 3, 3)
    m = _module(c["V"], c["tree"])
    betas = _cu(c["betas"])
    assert torch.equal(m(view, betas).cpu(), _got("rotmat")[0])
    assert torch.equal(m.get_vertex_transformation(view, betas).cpu(), _got("rotmat")[1])


def test_lbs_batch_limit(M):
    """grid.y = B: 65535 launches (test_lbs_vs_float64_oracle), 65536 is refused on the host."""
    p, b = np.zeros((O.B_MAX + 1, 72), dtype=np.float32), np.zeros((O.B_MAX + 1, 10), dtype=np.float32)
    with pytest.raises(RuntimeError, match="mf_smpl_lbs: batch 65536"):
        _module(3)(_cu(p), _cu(b))


# ------------------------------------------------------------------------------------------------------ (2) exact properties
@pytest.mark.parametrize("name", ["special", "B300"])
def test_lbs_batch_rows_are_independent(M, name):
    """Every kernel works per batch row in a fixed order: row b of a B-row launch is the B = 1 launch of that row, bit for bit."""
    from moco_flow_amd import synth
    if name == "special":
        c = O.lbs_cases()["special"]
        m, pose, betas = _module(c["V"], c["tree"]), c["pose"], c["betas"]
    else:
        m = _module(5)
        pose, betas = synth.smpl_pose(11, batch=300, scale=0.6)
    verts, T = _forward(m, pose, betas)
    for r in range(pose.shape[0]):
        v1, T1 = _forward(m, pose[r:r + 1], betas[r:r + 1])
        assert torch.equal(v1[0], verts[r]) and torch.equal(T1[0], T[r]), r
    assert not torch.equal(verts[0], verts[1]) and not torch.equal(T[-1], T[-2])


def _raw_lbs(m, pose, betas, want_verts, want_T):
    """mf_smpl_lbs through the C ABI: outputs pre-filled with NaN, (verts | None, T | None)."""
    from moco_flow_amd import _lib as L
    B, V, dev = pose.shape[0], m.vert_num, pose.device
    verts = torch.full((B, V, 3), float("nan"), device=dev) if want_verts else None
    T = torch.full((B, V, 4, 4), float("nan"), device=dev) if want_T else None
    scratch = torch.empty((max(int(L.lib().mf_smpl_scratch_bytes(V, B)), 4),), device=dev, dtype=torch.uint8)
    L.check(L.lib().mf_smpl_lbs(m._model(dev), L.ptr(pose), 0, L.ptr(betas), B, L.ptr(verts), L.ptr(T), L.ptr(scratch),
                                L.current_stream(dev)), "mf_smpl_lbs")
    return verts, T


@pytest.mark.parametrize("V", [5, 257])
def test_lbs_combined_launch(M, V):
    """The ABI allows verts and T from one launch (the module never asks for both): there smpl_skin_kernel's LDS copy of T
    feeds verts while T is stored.  Equal to the two single-output launches, which are the module's."""
    c = O.lbs_cases()[f"V{V}"]
    m, pose, betas = _module(V), _cu(c["pose"]).contiguous(), _cu(c["betas"]).contiguous()
    verts, T = _raw_lbs(m, pose, betas, True, True)
    v_only, none_T = _raw_lbs(m, pose, betas, True, False)
    none_v, T_only = _raw_lbs(m, pose, betas, False, True)
    assert none_T is None and none_v is None
    assert torch.equal(verts, v_only) and torch.equal(T, T_only)
    assert torch.equal(verts.cpu(), _got(f"V{V}")[0]) and torch.equal(T.cpu(), _got(f"V{V}")[1])


@pytest.mark.parametrize("name", ["V257", "chain_s2.5", "special"])
def test_lbs_last_row_of_T(M, name):
    """The chain keeps (0, 0, 0, 1) exactly, so T[..., 3, :3] is exactly 0 and T[..., 3, 3] is the fp32 sum of the vertex's 24
    weights in the kernel's order: acc = fma(w[j], 1, acc) for j = 0..23."""
    c = O.lbs_cases()[name]
    T = _got(name)[1]
    assert bool((T[..., 3, :3] == 0).all())
    w = O.model(c["V"], c["tree"])["weights"].astype(np.float32)
    acc = np.zeros(c["V"], dtype=np.float32)
    for j in range(24):
        acc = (acc + w[:, j]).astype(np.float32)
    assert torch.equal(T[..., 3, 3], torch.from_numpy(acc).expand(T.shape[0], -1))


def test_lbs_nan_row_is_contained(M):
    """All 72 components float32(-1e-8) in row 1 of 3: theta + 1e-8 is exactly 0 in fp32, the reference's rodrigues divides by it
    and that row is NaN (the float64 oracle is finite there: fp32 smpl_ref is the reference of this case).  The kernel's row 1
    is non-finite wherever smpl_ref's is; rows 0 and 2 are bit-equal to the launch without it."""
    from moco_flow_amd import synth
    from oracle import smpl_ref
    pose, betas = synth.smpl_pose(5, batch=3, scale=0.6)
    clean = pose.copy()
    pose[1] = O.nan_pose()[0]
    m = _module(5)
    verts, T = _forward(m, pose, betas)
    o = smpl_ref.SMPL(O.model(5))
    v32, T32 = o.forward(torch.from_numpy(pose), torch.from_numpy(betas)), o.get_vertex_transformation(torch.from_numpy(pose), torch.from_numpy(betas))
    assert not torch.isfinite(v32[1]).any() and not torch.isfinite(T32[1]).any()
    assert torch.equal(torch.isfinite(verts), torch.isfinite(v32)) and torch.equal(torch.isfinite(T), torch.isfinite(T32))
    v0, T0 = _forward(m, clean, betas)
    assert torch.equal(verts[[0, 2]], v0[[0, 2]]) and torch.equal(T[[0, 2]], T0[[0, 2]])
    assert torch.isfinite(v0).all() and torch.isfinite(T0).all()


@pytest.mark.parametrize("name", ["V6890", "special"])
def test_lbs_repeats_are_bit_identical(M, name):
    c = O.lbs_cases()[name]
    verts, T = _forward(_module(c["V"], c["tree"]), c["pose"], c["betas"])
    assert torch.equal(verts, _got(name)[0]) and torch.equal(T, _got(name)[1])


def test_lbs_host_refusals(M):
    from moco_flow_amd import smpl as S, synth
    pose, betas = synth.smpl_pose(5, batch=2, scale=0.6)
    for joint, parent, msg in ((6, 7, r"parent\[6\] = 7 is not an earlier joint"), (6, 6, r"parent\[6\] = 6 is not"),
                               (4, -1, r"parent\[4\] = -1 is not"), (23, 23, r"parent\[23\] = 23 is not")):
        bad = dict(O.model(5))
        bad["parent"] = O.tree("standard").copy()
        bad["parent"][joint - 1] = parent
        with pytest.raises(RuntimeError, match=msg):
            S.SMPL(model=bad).cuda()(_cu(pose), _cu(betas))
    m = _module(5)
    with pytest.raises(RuntimeError, match="pose must be"):
        m(_cu(pose).view(2, 24, 3), _cu(betas))
    with pytest.raises(RuntimeError, match="pose must be"):
        m(_cu(pose).view(2, 24, 3, 1, 1), _cu(betas))
    with pytest.raises(RuntimeError, match="betas must be"):
        m(_cu(pose), _cu(betas)[:, :9])
    with pytest.raises(RuntimeError):
        m(_cu(pose)[:, :71], _cu(betas))
    assert m(_cu(pose)[:0], _cu(betas)[:0]).shape == (0, 5, 3)
    assert m.get_vertex_transformation(_cu(pose)[:0], _cu(betas)[:0]).shape == (0, 5, 4, 4)


# -------------------------------------------------------------------------------------------- (3) mf_smpl_frame_transforms
def _frame(src, tgt):
    from moco_flow_amd import smpl as S
    return S.frame_transforms(_cu(src), _cu(tgt)).cpu()


def _normalised(label, got, src, tgt, ref_worst, asserted=True):
    t64 = O.frame_transforms(src, tgt)
    e = O.normalised_inverse_error(got, t64, src)
    r = O.normalised_inverse_error(tgt @ torch.inverse(src), t64, src)
    bar = O.MARGIN * ref_worst
    print(f"{label:16s} trans normalised error: kernel worst {float(e.max()):6.2f} median {float(e.median()):5.2f}   fp32 reference worst "
          f"{float(r.max()):5.2f} median {float(r.median()):5.2f}   (bar {bar:.2f}{'' if asserted else ', not asserted'})   "
          f"max-rel kernel {relerr(got, t64):.2e} reference {relerr(tgt @ torch.inverse(src), t64):.2e}")
    if asserted:
        assert float(e.max()) <= bar, (label, float(e.max()), bar)
        assert relerr(got, t64) <= O.CONTRACT["trans"], (label, relerr(got, t64))


def test_frame_transforms_buckets(M):
    """See (3) of the module docstring; c3000 is printed, not asserted."""
    _, ref_worst = O.inverse_ref_errors()
    for name in O.BUCKETS:
        src, tgt = O.bucket(name)
        _normalised(name, _frame(src, tgt), src, tgt, ref_worst, asserted=name in O.HELD_BUCKETS)


@pytest.mark.parametrize("V", [1, 127, 128, 129])
def test_frame_transforms_sizes_and_slices(M, V):
    """128 vertices per workgroup.  A launch of the first V vertices: held to the bar, and bit-equal to those rows of the
    1000-vertex launch (vertex v's 16 outputs depend on vertex v alone)."""
    _, ref_worst = O.inverse_ref_errors()
    for name in ("blend", "general"):
        src, tgt = O.bucket(name)
        got = _frame(src[:V], tgt[:V])
        _normalised(f"{name}[:{V}]", got, src[:V], tgt[:V], ref_worst)
        assert torch.equal(got, _frame(src, tgt)[:V])
        assert torch.equal(_frame(src[1000 - V:], tgt[1000 - V:]), _frame(src, tgt)[1000 - V:])


def test_frame_transforms_exact(M):
    from moco_flow_amd import smpl as S
    assert S.frame_transforms(torch.zeros(0, 4, 4).cuda(), torch.zeros(0, 4, 4).cuda()).shape == (0, 4, 4)
    src, tgt = O.bucket("general")
    # T_src = I: every cofactor is 0 or 1, det is 1 and the product adds zeros
    eye = torch.eye(4).expand(1000, 4, 4).contiguous()
    assert torch.equal(_frame(eye, src), src)
    # a permuted launch is the permuted output
    perm = torch.randperm(1000, generator=torch.Generator().manual_seed(3))
    full = _frame(src, tgt)
    assert torch.equal(_frame(src[perm], tgt[perm]), full[perm])
    # a singular T_src at one vertex makes only that vertex non-finite
    bad = src.clone()
    bad[129, 0] = 0                                            # a zero row: six of the 2 x 2 minors and det are exactly 0
    got = _frame(bad, tgt)
    assert not torch.isfinite(got[129]).any()
    keep = torch.arange(1000) != 129
    assert torch.equal(got[keep], full[keep])


@pytest.mark.parametrize("V", [431, 6890])
def test_frame_transforms_of_the_pipeline(M, V):
    """T of two poses from mf_smpl_lbs itself (near-rigid blends, the datasets' input) through the same normalised bar."""
    _, ref_worst = O.inverse_ref_errors()
    T = _got(f"V{V}")[1]
    _normalised(f"pipeline V{V}", _frame(T[0], T[1]), T[0], T[1], ref_worst)


# ------------------------------------------------------------------------------------------ (4) mf_apply_vertex_transforms
def _apply(trans, ind, query):
    from moco_flow_amd import smpl as S
    return S.apply_vertex_transforms(_cu(trans), _cu(ind), _cu(query)).cpu()


@pytest.mark.parametrize("V", O.APPLY_V)
@pytest.mark.parametrize("Q", O.APPLY_Q)
def test_apply_vs_float64_oracle(M, Q, V):
    per, med = O.apply_yardsticks()
    trans, ind, query = O.apply_case(Q, V)
    want = O.apply_vertex_transforms(trans, ind, query)
    got = _apply(trans, ind, query)
    _hold(f"apply Q{Q} V{V}", "cano", got, want, per[(Q, V)], med)
    assert torch.equal(_apply(trans, ind.view(Q, 1), query), got)
    assert torch.equal(_apply(trans, ind.to(torch.int32), query), got)


def test_apply_rows_depend_on_their_own_inputs(M):
    trans, ind, query = O.apply_case(257, 7)
    got = _apply(trans, ind, query)
    perm = torch.randperm(257, generator=torch.Generator().manual_seed(4))
    assert torch.equal(_apply(trans, ind[perm], query[perm]), got[perm])
    for i in range(257):
        assert torch.equal(_apply(trans[ind[i]][None], torch.zeros(1, dtype=torch.int64), query[i:i + 1])[0], got[i]), i


def test_apply_clamps_indices(M):
    """include/mocoflow_hip.h: an index outside [0, V - 1] is clamped before any address is formed."""
    trans, ind, query = O.apply_case(257, 7)
    out_of_range = torch.tensor([-1, -2 ** 40, 7, 2 ** 40], dtype=torch.int64)
    clamped = torch.tensor([0, 0, 6, 6], dtype=torch.int64)
    where = torch.tensor([0, 100, 255, 256])                   # both workgroups of the launch
    bad, good = ind.clone(), ind.clone()
    bad[where], good[where] = out_of_range, clamped
    assert torch.equal(_apply(trans, bad, query), _apply(trans, good, query))
    assert torch.equal(_apply(trans[:1], out_of_range, query[:4]), _apply(trans[:1], torch.zeros(4, dtype=torch.int64), query[:4]))


def test_frame_correspondence_with_an_empty_side(M):
    """Every query inside (the outside set is empty) and every query outside: the same rows on the other side, and the canonical
    half against the oracle's chain on the float64 nearest vertex."""
    from moco_flow_amd import smpl as S
    c, o = O.lbs_cases()["V431"], O.lbs_oracle("V431")
    m = _module(431)
    pose, betas = _cu(c["pose"]), _cu(c["betas"])
    query = (torch.rand(300, 3, generator=torch.Generator().manual_seed(5)) - 0.5) * 2.0
    args = (m, pose[:1], betas[:1], pose[1:], betas[1:], query.cuda())
    inside, none_out = S.frame_correspondence(*args, thickness=1e9)
    none_in, outside = S.frame_correspondence(*args, thickness=0.0)
    assert inside.shape == (300, 6) and none_out.shape == (0, 6) and none_in.shape == (0, 6) and outside.shape == (300, 6)
    assert torch.equal(inside, outside) and torch.equal(inside[:, :3].cpu(), query)
    ind = torch.cdist(query.double(), o["verts"][0]).argmin(1)
    want = O.apply_vertex_transforms(O.frame_transforms(o["T"][0], o["T"][1]), ind, query)
    e = relerr(inside[:, 3:], want)
    print(f"frame_correspondence V431 Q300: cano max-rel {e:.2e} (contract {O.CONTRACT['cano']:.0e})")
    assert e <= O.CONTRACT["cano"]


# ------------------------------------------------------------------------------------------------------ (5) the module's cache
@pytest.mark.parametrize("how", ["register_buffer", "setattr", "in_place"])
@pytest.mark.parametrize("name", ["weights", "J_regressor", "v_template", "posedirs", "shapedirs"])
@pytest.mark.parametrize("where", ["cuda", "cpu"])
def test_module_cache_follows_its_buffers(M, where, name, how):
    """After a first forward a model buffer is reassigned (register_buffer, or attribute assignment on the registered name) or
    edited in place, on a module on the GPU and on one left on the CPU and called with GPU poses: the next forward equals a
    freshly built module's bit for bit.  Unchanged, the module reuses its cached descriptor (no copy, no sync)."""
    from moco_flow_amd import smpl as S, synth
    assets = synth.smpl_model(1, 5)
    pose, betas = synth.smpl_pose(5, batch=2, scale=0.6)
    pose, betas = _cu(pose), _cu(betas)
    m = S.SMPL(model=assets)
    m = m.cuda() if where == "cuda" else m
    first = (m(pose, betas), m.get_vertex_transformation(pose, betas))
    desc = m._packed[1]
    m(pose, betas)
    assert m._packed[1] is desc and m._model(pose.device) is desc
    new = getattr(m, name) * 1.5
    if how == "register_buffer":
        m.register_buffer(name, new)
    elif how == "setattr":
        setattr(m, name, new)
    else:
        getattr(m, name).mul_(1.5)
    fresh = S.SMPL(model=dict(assets, **{name: new.cpu().numpy()})).cuda()
    want = (fresh(pose, betas), fresh.get_vertex_transformation(pose, betas))
    got = (m(pose, betas), m.get_vertex_transformation(pose, betas))
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert not torch.equal(got[0], first[0])
    assert name in ("posedirs",) or not torch.equal(got[1], first[1])        # the pose blend shapes move verts alone
    desc = m._packed[1]
    m.get_vertex_transformation(pose, betas)
    assert m._packed[1] is desc and m._model(pose.device) is desc
