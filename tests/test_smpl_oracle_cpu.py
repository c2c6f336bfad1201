"""Preconditions of tests/test_gpu_smpl.py on its own inputs, without a GPU: the float64 SMPL oracle (tests/smpl_oracle.py) is
pinned to the reference's recorded outputs and to oracle/smpl_ref.py, and every distance the GPU bars are made of -- fp32
smpl_ref's own distance from float64 per case and its median, the bucket sizes and condition numbers, the fp32 reference
inverse's normalised error, the NaN rule -- is computed here from the reference alone.  The deliberate breakages of the oracle
move it by more than those bars, so the GPU bars can see them.

Measured here (max-rel of fp32 smpl_ref to the float64 oracle, verts / T): V sweep 0.9e-7 .. 4.6e-7 / 2.9e-7 .. 5.0e-7; chain
tree 7.7e-7 .. 1.0e-6 / 9.1e-7 .. 1.1e-6; star 2.4e-7 .. 3.3e-7 / 1.9e-7 .. 2.7e-7; special angles 3.2e-7 / 7.7e-7; B = 65535
4.0e-7 / 3.7e-7; medians 3.6e-7 / 4.2e-7.  fp32 `T_tgt @ inverse(T_src)`, worst normalised error per bucket: rigid 2.2, blend
1.6, c30 0.44, c300 0.39, general 1.05, c3000 0.39.  cano: 0.7e-8 .. 1.0e-7, median 7.7e-8.

One breakage the issue behind these files asked for cannot be seen by any bar: dropping quat2mat's second normalisation.  The
quaternion is (cos h, sin h * theta / |theta + 1e-8|); its norm differs from 1 by sin^2 h * (|axis|^2 - 1), and |axis| is far
from 1 only where sin h is ~1e-8.  Measured: 1.8e-8 at pi, 1e-12 at 1e-4, exactly 0 at 3e-9
(test_second_normalisation_is_below_fp32_resolution pins that, so nobody reads a guarantee into the GPU file)."""
import numpy as np
import pytest
import torch

import smpl_oracle as O
from helpers import load_golden, relerr
from moco_flow_amd import synth
from oracle import smpl_ref

EPS32 = 2.0 ** -24


def test_float64_oracle_reproduces_the_reference_golden():
    """tests/golden/u_smpl.npz holds the reference's own fp32 outputs.  fp32 smpl_ref sits at most 1.1e-6 (chain tree) from
    float64 over this file's cases; the standard tree at B = 3, V = 431 is held to 1e-6, ten times under the GPU contract."""
    g = load_golden("u_smpl")
    m = synth.smpl_model(int(g["meta_seed"]), int(g["meta_V"]))
    o = O.lbs(m, g["in_pose"], g["in_betas"])
    assert relerr(g["out_R"], o["R"]) <= 4 * EPS32
    assert relerr(g["out_verts"], o["verts"]) <= 1e-6 and relerr(g["out_T"], o["T"]) <= 1e-6
    assert relerr(g["out_verts_from_R"], O.lbs(m, g["out_R"], g["in_betas"])["verts"]) <= 1e-6
    # the reference's fp32 T as the operand of both: what is left is its fp32 inverse and product
    trans = O.frame_transforms(g["out_T"][0], g["out_T"][1])
    e = O.normalised_inverse_error(g["out_trans"], trans, g["out_T"][0])
    assert float(e.max()) <= 4.0, float(e.max())
    assert relerr(g["out_cano"], O.apply_vertex_transforms(g["out_trans"], g["out_ind"], g["in_query"])) <= 4 * EPS32


@pytest.mark.parametrize("name", [n for n in O.lbs_cases() if not n.startswith("B")])
def test_float32_mode_agrees_with_smpl_ref(name):
    """The oracle in float32 is one more fp32 order of the same sums: held to the bar the kernel gets."""
    c = O.lbs_cases()[name]
    o32 = O.lbs(O.model(c["V"], c["tree"]), c["pose"], c["betas"], dtype=torch.float32)
    per, med = O.lbs_yardsticks()
    v32, T32 = O.lbs_ref32(name)
    for kind, ref in (("verts", v32), ("T", T32)):
        bar, _ = O.bar(kind, per[name][kind], med[kind])
        assert o32[kind].dtype == torch.float32 and relerr(o32[kind], ref) <= bar, (name, kind, relerr(o32[kind], ref), bar)


def test_trees_are_accepted_and_differ():
    assert O.tree("chain").tolist() == list(range(23)) and O.tree("star").tolist() == [0] * 23
    assert O.tree("standard").tolist() == list(synth.SMPL_PARENTS)
    c = O.lbs_cases()["chain_s0.6"]
    outs = [O.lbs(O.model(O.V_EDGE, t), c["pose"], c["betas"])["verts"] for t in O.TREES]
    assert relerr(outs[0], outs[1]) > 1e-2 and relerr(outs[0], outs[2]) > 1e-2 and relerr(outs[1], outs[2]) > 1e-2


def test_lbs_yardsticks_are_what_the_gpu_bars_need():
    """Every LBS case's fp32-vs-float64 distance, recorded; the median is the GPU file's yardstick, computed not typed in."""
    per, med = O.lbs_yardsticks()
    assert set(per) == set(O.lbs_cases()) and len(per) == len(O.LBS_V) + 6 + 3
    for name, d in per.items():
        print(f"{name:16s} verts {d['verts']:.2e}  T {d['T']:.2e}")
        for kind in ("verts", "T"):
            # an fp32 evaluation of sums this short lies within a few hundred roundings of float64, and is not float64
            assert EPS32 / 4 <= d[kind] <= 100 * EPS32, (name, kind, d[kind])
            bar, yard = O.bar(kind, d[kind], med[kind])
            assert bar == O.MARGIN * yard < O.CONTRACT[kind]                      # the contract never binds here
    print(f"median           verts {med['verts']:.2e}  T {med['T']:.2e}")
    assert med["verts"] == float(np.median([d["verts"] for d in per.values()]))
    worst = max(per, key=lambda n: per[n]["T"])
    print(f"worst T: {worst} (the 23-deep chain is the longest product; which case leads is the host's BLAS, not asserted)")


def test_special_poses_hold_their_angles():
    p = torch.from_numpy(O.special_poses()).double().view(7, 24, 3)
    for r, a in enumerate(O.SPECIAL_ANGLES):
        assert torch.allclose(p[r].norm(dim=1), torch.full((24,), a, dtype=torch.float64), rtol=2e-7, atol=0)
    assert not p[6].any()
    o = O.lbs_oracle("special")
    eye = torch.eye(3, dtype=torch.float64)
    assert relerr(o["R"][2], eye.expand(24, 3, 3)) <= 1e-6                       # 2 pi: the identity again
    assert float((o["R"][0] - eye).abs().max()) > 1.9                            # pi: a half turn
    assert relerr(o["R"][6], eye.expand(24, 3, 3)) <= 1e-15
    # 3e-9: |theta + 1e-8| is not |theta|, so the "unit" axis is not unit
    th = p[5]
    axis = th / (th + 1e-8).norm(dim=1, keepdim=True)
    assert float((axis.norm(dim=1) - 1).abs().max()) > 0.5


def test_nan_rule():
    """float32(-1e-8) + 1e-8 is exactly 0 in fp32: the reference's rodrigues divides by it and the batch row is NaN.  In
    float64 the sum is 6e-17, the oracle is finite: this case is compared with fp32 smpl_ref alone."""
    pose, betas = synth.smpl_pose(5, batch=3, scale=0.6)
    pose[1] = O.nan_pose()[0]
    m = O.model(5)
    o = smpl_ref.SMPL(m)
    v, T = o.forward(torch.from_numpy(pose), torch.from_numpy(betas)), o.get_vertex_transformation(torch.from_numpy(pose), torch.from_numpy(betas))
    assert torch.isnan(v[1]).all() and torch.isnan(T[1]).all()
    assert torch.isfinite(v[[0, 2]]).all() and torch.isfinite(T[[0, 2]]).all()
    o64 = O.lbs(m, pose, betas)
    assert torch.isfinite(o64["verts"]).all() and torch.isfinite(o64["T"]).all()
    assert torch.isnan(O.lbs(m, pose, betas, dtype=torch.float32)["verts"][1]).all()


def test_inverse_buckets():
    """Sizes, condition numbers and the fp32 reference's normalised error: the bar of the GPU file is 3 x `worst`."""
    worst = 0.0
    for name in O.BUCKETS:
        src, tgt = O.bucket(name)
        c = O.cond2(src)
        assert src.shape == tgt.shape == (O.BUCKET_N, 4, 4) and O.BUCKET_N >= 1000
        assert float(O.cond2(tgt).max()) < O.BUCKET_COND["rigid"][1]             # T_tgt is rigid
        if name in O.BUCKET_COND:
            lo, hi = O.BUCKET_COND[name]
            assert lo <= float(c.min()) and float(c.max()) < hi, (name, float(c.min()), float(c.max()))
        if name == "general":
            assert float(src[:, 3, :3].abs().min()) > 0 and float((src[:, 3, 3] - 1).abs().min()) > 0      # no (0, 0, 0, 1)
        else:
            assert torch.equal(src[:, 3], torch.tensor([0.0, 0, 0, 1]).expand(O.BUCKET_N, 4))
        t64 = O.frame_transforms(src, tgt)
        e = O.normalised_inverse_error(smpl_ref.frame_transforms(src, tgt), t64, src)
        print(f"{name:8s} cond {float(c.min()):9.2f} .. {float(c.max()):9.2f}   fp32 reference: worst normalised error "
              f"{float(e.max()):.2f}, median {float(e.median()):.2f}, max-rel {relerr(smpl_ref.frame_transforms(src, tgt), t64):.2e}")
        assert (float(e.max()), float(e.median())) == O.inverse_ref_errors()[0][name]
        if name in O.ASSERTED_BUCKETS:
            worst = max(worst, float(e.max()))
        if name in O.HELD_BUCKETS:
            assert relerr(smpl_ref.frame_transforms(src, tgt), t64) < O.CONTRACT["trans"] / O.MARGIN
    assert worst == O.inverse_ref_errors()[1] and 0.3 <= worst <= 8.0, worst                 # a backward-stable inverse: a few units of cond * 2^-24
    # the float64 adjugate is an inverse; with one cofactor's sign flipped it is not.  In the general bucket each of the 16 is
    # live (over 100 bars away); on affine input the three cofactors of the inverse's last row are zero and a flip there is
    # invisible -- why the general bucket is asserted at all
    for name in O.HELD_BUCKETS:
        src, tgt = O.bucket(name)
        t64 = O.frame_transforms(src, tgt)
        assert relerr(O.frame_transforms(src, tgt, inverse=O.adjugate_inverse), t64) <= 1e-12
        for flip in [(i, j) for i in range(4) for j in range(4)]:
            bad = O.frame_transforms(src, tgt, inverse=lambda A: O.adjugate_inverse(A, flip=flip))
            e = float(O.normalised_inverse_error(bad, t64, src).max())
            if name == "general" or flip[0] < 3:
                assert e >= 100 * O.MARGIN * worst, (name, flip, e)
            elif flip[1] < 3:
                assert e <= 1e-3, (name, flip, e)


def test_apply_yardsticks():
    per, med = O.apply_yardsticks()
    assert set(per) == {(Q, V) for Q in O.APPLY_Q for V in O.APPLY_V}
    for (Q, V), d in per.items():
        trans, ind, query = O.apply_case(Q, V)
        assert ind.shape == (Q,) and int(ind.min()) >= 0 and int(ind.max()) < V
        assert Q < 2 or len(ind.unique()) < Q                                     # duplicates
        assert d <= 8 * EPS32 and O.bar("cano", d, med)[0] < O.CONTRACT["cano"]
    print("cano:", {k: f"{v:.1e}" for k, v in per.items()}, f"median {med:.2e}")
    assert EPS32 / 4 <= med


def _moved(broken, clean):
    return {k: relerr(broken[k], clean[k]) for k in ("verts", "T")}


def test_breakages_move_the_oracle_past_the_bars():
    """Each deliberate breakage of the oracle or of its inputs, measured against the intact oracle on the GPU file's own case:
    more than 10 x the bar of the tensor that has to see it."""
    per, med = O.lbs_yardsticks()
    bars = lambda name: {k: O.bar(k, per[name][k], med[k])[0] for k in ("verts", "T")}
    c, clean, m = O.lbs_cases()["V257"], O.lbs_oracle("V257"), O.model(257)
    # the parents rolled by one (still a valid tree)
    rolled = dict(m, parent=np.roll(m["parent"], -1))
    d = _moved(O.lbs(rolled, c["pose"], c["betas"]), clean)
    assert d["verts"] > 10 * bars("V257")["verts"] and d["T"] > 10 * bars("V257")["T"], d
    # the last vertex (V = 4k + 1: alone in its workgroup) on another vertex's weights: only that vertex moves
    for name in ("V5", "V257"):
        cc, mm = O.lbs_cases()[name], O.model(O.lbs_cases()[name]["V"])
        w = mm["weights"].copy()
        w[-1] = w[0]
        b = O.lbs(dict(mm, weights=w), cc["pose"], cc["betas"])
        d = _moved(b, O.lbs_oracle(name))
        assert d["verts"] > 10 * bars(name)["verts"] and d["T"] > 10 * bars(name)["T"], (name, d)
        assert torch.equal(b["T"][:, :-1], O.lbs_oracle(name)["T"][:, :-1])
    # the fourth trip (15 lanes) of the 207-wide pose-blend dot product: verts alone can see it
    pd = m["posedirs"].copy()
    pd[:, :, 192:] = 0
    d = _moved(O.lbs(dict(m, posedirs=pd), c["pose"], c["betas"]), clean)
    assert d["verts"] > 10 * bars("V257")["verts"] and d["T"] == 0.0, d
    # lrotmin rows read at stride 208: row 0 is intact, row 1 is off by one element
    b = O.lbs(m, c["pose"], c["betas"], lrot_stride=208)
    assert torch.equal(b["verts"][0], clean["verts"][0])
    assert relerr(b["verts"][1], clean["verts"][1]) > 10 * bars("V257")["verts"]
    # batch row b compared with row b + 1
    for name in ("V257", "special", f"B{O.B_MAX}"):
        o = O.lbs_oracle(name)
        for k in ("verts", "T"):
            assert relerr(torch.roll(o[k], 1, 0), o[k]) > 10 * bars(name)[k], (name, k)
    # ind + 1 in the second block of queries
    _, cmed = O.apply_yardsticks()
    trans, ind, query = O.apply_case(5000, 6890)
    bad = ind.clone()
    bad[256:512] = (bad[256:512] + 1) % 6890
    good = O.apply_vertex_transforms(trans, ind, query)
    assert relerr(O.apply_vertex_transforms(trans, bad, query), good) > 10 * O.bar("cano", 0.0, cmed)[0]
    assert torch.equal(O.apply_vertex_transforms(trans, bad, query)[:256], good[:256])


def test_second_normalisation_is_below_fp32_resolution():
    """See the module docstring: without quat2mat's second normalisation the float64 oracle moves by less than half an fp32
    rounding at every special angle, and not at all at 3e-9.  No fp32 bar can see this breakage."""
    c, m = O.lbs_cases()["special"], O.model(O.V_EDGE)
    a, b = O.lbs_oracle("special"), O.lbs(m, c["pose"], c["betas"], renorm=False)
    for r in range(7):
        for k in ("verts", "T"):
            assert relerr(b[k][r], a[k][r]) <= EPS32 / 2, (r, k)
    assert torch.equal(b["verts"][5], a["verts"][5]) and torch.equal(b["T"][5], a["T"][5])


def test_module_cache_follows_every_buffer():
    """SMPL._model's cached copies (no kernel runs: the descriptor is built for the CPU device): a reassigned or edited buffer
    rebuilds them, an unchanged model reuses the descriptor object."""
    from moco_flow_amd import smpl as S
    assets = synth.smpl_model(1, 5)
    names = {"weights": "w", "J_regressor": "jr", "v_template": "vt", "posedirs": "pd", "shapedirs": "sd"}
    for name, slot in names.items():
        for how in ("register_buffer", "setattr", "in_place"):
            m = S.SMPL(model=assets)
            d0 = m._model(torch.device("cpu"))
            assert m._model(torch.device("cpu")) is d0
            new = getattr(m, name) * 1.5
            if how == "register_buffer":
                m.register_buffer(name, new)
            elif how == "setattr":
                setattr(m, name, new)
            else:
                getattr(m, name).mul_(1.5)
            d1 = m._model(torch.device("cpu"))
            assert d1 is not d0 and m._model(torch.device("cpu")) is d1, (name, how)
            want = new[:, :, :10] if name == "shapedirs" else new
            assert torch.equal(m._packed[2][slot].reshape(want.shape), want), (name, how)
