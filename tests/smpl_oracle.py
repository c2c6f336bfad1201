"""Float64 oracle of the SMPL unit (csrc/mf_smpl.hip: mf_smpl_lbs, mf_smpl_frame_transforms, mf_apply_vertex_transforms) and
the inputs tests/test_gpu_smpl.py launches.  No GPU and no package code beyond the synthetic assets of moco_flow_amd.synth;
tests/test_smpl_oracle_cpu.py holds what is here to the preconditions the GPU bars need.

Written from the reference's formulas (utils/smpl/smpl_model.py:17-55, 96-186; datasets/moco_flow_dataset.py:96-99, 127-129),
vectorised over the batch, in the dtype asked for.  It does not call oracle/smpl_ref.py: that file stays the fp32
restatement of the reference, and its distance from this oracle in float64 is the yardstick of the GPU bars (`yardsticks`).

The keyword arguments `renorm`, `lrot_stride` and `flip` exist to BREAK the oracle on purpose (tests/test_smpl_oracle_cpu.py::
test_breakages_move_the_oracle_past_the_bars): their defaults are the reference's arithmetic."""
import functools
import math

import numpy as np
import torch

from moco_flow_amd import synth

F64 = torch.float64

LBS_V = (1, 2, 3, 4, 5, 255, 256, 257, 431, 6890)          # B = 2 each: V mod 4 = 0..3, the 256-wide tails, both fixture sizes
TREES = ("standard", "chain", "star")
TREE_SCALES = (0.6, 2.5)
V_EDGE = 257                                                # 4k + 1 and 256 + 1: the vertex count of the tree / angle / matrix cases
SPECIAL_ANGLES = (math.pi, math.pi - 1e-4, 2 * math.pi, 1e-4, 1e-7, 3e-9)       # one batch row each; row 6 is the zero pose
B_MAX = 65535                                               # grid.y of the launch; the host refuses more
CONTRACT = {"verts": 1e-5, "T": 1e-5, "trans": 1e-4, "cano": 1e-4}      # tests/test_gpu_parity.py::test_smpl_lbs_vs_reference_golden
MARGIN = 3.0
ASSERTED_BUCKETS = ("rigid", "blend", "c30", "c300")        # affine T_src; the reference's worst over these makes the bar
HELD_BUCKETS = ASSERTED_BUCKETS + ("general",)              # full 4 x 4 matrices, held to that same bar
BUCKETS = HELD_BUCKETS + ("c3000",)                         # measured and printed only
BUCKET_N = 1000
APPLY_Q = (1, 255, 256, 257, 5000)
APPLY_V = (1, 7, 6890)


def _t(a, dtype):
    return torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a).detach().cpu().to(dtype)


# ---------------------------------------------------------------------------------------------------------------- the oracle
def quat2mat(q, renorm=True):
    """smpl_model.py:17-37: (N,4) (w,x,y,z) -> (N,3,3); the quaternion is normalised first (renorm=False: a breakage)."""
    if renorm:
        q = q / q.square().sum(1, keepdim=True).sqrt()
    w, x, y, z = q.unbind(1)
    return torch.stack([w * w + x * x - y * y - z * z, 2 * x * y - 2 * w * z, 2 * w * y + 2 * x * z,
                        2 * w * z + 2 * x * y, w * w - x * x + y * y - z * z, 2 * y * z - 2 * w * x,
                        2 * x * z - 2 * w * y, 2 * w * x + 2 * y * z, w * w - x * x - y * y + z * z], dim=1).view(-1, 3, 3)


def rodrigues(theta, dtype=F64, renorm=True):
    """smpl_model.py:40-55: axis-angle (N,3) -> (N,3,3) through the half-angle quaternion.  The norm is taken of
    theta + 1e-8, the division uses theta, and quat2mat normalises again."""
    theta = _t(theta, dtype)
    angle = (theta + 1e-8).square().sum(1, keepdim=True).sqrt()
    axis = theta / angle
    half = angle * 0.5
    return quat2mat(torch.cat([torch.cos(half), torch.sin(half) * axis], dim=1), renorm)


def lbs(model, pose, betas, dtype=F64, renorm=True, lrot_stride=207):
    """SMPL.forward and SMPL.get_vertex_transformation (smpl_model.py:96-186) over model = dict(v_template (V,3), shapedirs
    (V,3,>=10), posedirs (V,3,207), J_regressor (24,V), weights (V,24), parent (23,) of joints 1..23, each an earlier joint).
    pose (B,72) axis-angle or (B,24,3,3) rotation matrices, betas (B,10) -> dict(verts (B,V,3), T (B,V,4,4), R, J, G, lrotmin).
    lrot_stride != 207 is a breakage: row b of lrotmin read at b * lrot_stride of the flat (B * 207) array."""
    vt, sd, pd = _t(model["v_template"], dtype), _t(model["shapedirs"], dtype), _t(model["posedirs"], dtype)
    jr, w = _t(model["J_regressor"], dtype), _t(model["weights"], dtype)
    parent = [int(p) for p in np.asarray(model["parent"]).tolist()]
    assert len(parent) == 23 and all(0 <= p <= i for i, p in enumerate(parent)), parent
    pose, betas = _t(pose, dtype), _t(betas, dtype)
    B, V = pose.shape[0], vt.shape[0]
    v_shaped = (betas @ sd[:, :, :10].reshape(V * 3, 10).T).view(B, V, 3) + vt                        # :100-103
    J = torch.einsum("jv,bvc->bjc", jr, v_shaped)                                                     # :105-108
    R = pose if pose.dim() == 4 else rodrigues(pose.reshape(-1, 3), dtype, renorm).view(B, 24, 3, 3)  # :110-116
    lrotmin = (R[:, 1:] - torch.eye(3, dtype=dtype)).reshape(B, 207)                                  # :117-119
    if lrot_stride != 207:
        flat = torch.cat([lrotmin.reshape(-1), torch.zeros(B * abs(lrot_stride - 207) + 207, dtype=dtype)])
        lrotmin = torch.stack([flat[b * lrot_stride:b * lrot_stride + 207] for b in range(B)])
    v_posed = v_shaped + (lrotmin @ pd.reshape(V * 3, 207).T).view(B, V, 3)                           # :120-121
    Gl = torch.zeros(B, 24, 4, 4, dtype=dtype)                                                        # :122-126
    Gl[..., :3, :3] = R
    Gl[..., :3, 3] = J
    Gl[:, 1:, :3, 3] -= J[:, parent]
    Gl[..., 3, 3] = 1
    G = [Gl[:, 0]]
    for i in range(1, 24):
        G.append(G[parent[i - 1]] @ Gl[:, i])                                                         # :127-129
    G = torch.stack(G, dim=1)
    G[..., :3, 3] = G[..., :3, 3] - torch.einsum("bjrc,bjc->bjr", G[..., :3, :3], J)                  # :131-135
    T = torch.einsum("vj,bjrc->bvrc", w, G)                                                           # :136
    verts = torch.einsum("bvrc,bvc->bvr", T[..., :3, :3], v_posed) + T[..., :3, 3]                    # :137-139
    return dict(verts=verts, T=T, R=R, J=J, G=G, lrotmin=lrotmin)


def adjugate_inverse(A, flip=None):
    """Inverse of (N,4,4) by the textbook cofactor expansion, inv[i,j] = (-1)^(i+j) det(A without row j, column i) / det A, in
    A's dtype.  flip = (i, j) negates that one cofactor: a breakage."""
    N = A.shape[0]
    cof = torch.empty_like(A)
    for i in range(4):
        for j in range(4):
            rows, cols = [r for r in range(4) if r != j], [c for c in range(4) if c != i]
            m = A[:, rows][:, :, cols]
            d = (m[:, 0, 0] * (m[:, 1, 1] * m[:, 2, 2] - m[:, 1, 2] * m[:, 2, 1])
                 - m[:, 0, 1] * (m[:, 1, 0] * m[:, 2, 2] - m[:, 1, 2] * m[:, 2, 0])
                 + m[:, 0, 2] * (m[:, 1, 0] * m[:, 2, 1] - m[:, 1, 1] * m[:, 2, 0]))
            cof[:, i, j] = d * (-1.0 if (i + j) % 2 else 1.0) * (-1.0 if flip == (i, j) else 1.0)
    det = (A[:, 0, :] * cof[:, :, 0]).sum(1)
    return cof / det.view(N, 1, 1)


def frame_transforms(T_src, T_tgt, dtype=F64, inverse=torch.linalg.inv):
    """moco_flow_dataset.py:96-99: T_tgt @ inverse(T_src) per vertex, (V,4,4)."""
    return _t(T_tgt, dtype) @ inverse(_t(T_src, dtype))


def apply_vertex_transforms(trans, ind, query, dtype=F64):
    """moco_flow_dataset.py:127-129: cano (Q,3) = (trans[ind] @ [query, 1])[:3]; ind (Q,) or (Q,1), any integer type."""
    trans, query = _t(trans, dtype), _t(query, dtype)
    ind = torch.as_tensor(ind).detach().cpu().reshape(-1).long()
    h = torch.cat([query, torch.ones(query.shape[0], 1, dtype=dtype)], dim=1)
    return torch.einsum("qrc,qc->qr", trans[ind], h)[:, :3]


def relerr(a, b):
    """helpers.relerr: max |a - b| / max |b| in float64."""
    a, b = _t(a, F64), _t(b, F64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return 0.0 if b.numel() == 0 else float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def cond2(A):
    """2-norm condition number of each (4,4) of A, in float64."""
    s = torch.linalg.svdvals(_t(A, F64))
    return s[:, 0] / s[:, -1]


def normalised_inverse_error(trans, trans64, T_src):
    """Per vertex: max |trans_v - trans64_v| / max |trans64_v|, in units of cond2(T_src_v) * 2^-24 -- what a backward-stable
    fp32 inverse may lose."""
    a, b = _t(trans, F64), _t(trans64, F64)
    e = (a - b).abs().flatten(1).max(1).values / b.abs().flatten(1).max(1).values
    return e / (cond2(T_src) * 2.0 ** -24)


# ------------------------------------------------------------------------------------------------------------------- builders
def _gen(seed):
    return torch.Generator().manual_seed(20000 + seed)


def tree(name):
    """parents of joints 1..23: SMPL's own, a 23-deep chain (parent[i] = i - 1), a star (all 0)."""
    return {"standard": np.array(synth.SMPL_PARENTS, dtype=np.int64), "chain": np.arange(23, dtype=np.int64),
            "star": np.zeros(23, dtype=np.int64)}[name]


@functools.lru_cache(maxsize=None)
def model(V, tree_name="standard"):
    m = synth.smpl_model(1, V)
    m["parent"] = tree(tree_name)
    return m


def random_axes(n, seed):
    a = torch.randn(n, 3, generator=_gen(seed), dtype=F64)
    return a / a.norm(dim=1, keepdim=True)


def special_poses(seed=0):
    """(7,72) fp32: row r < 6 has all 24 joints at SPECIAL_ANGLES[r] about random axes; row 6 is the all-zero pose."""
    rows = [(random_axes(24, seed * 16 + r) * a).reshape(72) for r, a in enumerate(SPECIAL_ANGLES)]
    return torch.stack(rows + [torch.zeros(72, dtype=F64)]).float().numpy()


def nan_pose():
    """Every component float32(-1e-8): theta + 1e-8 is exactly 0 in fp32 and the reference's rodrigues divides by it."""
    return np.full((1, 72), -1e-8, dtype=np.float32)


def rotations(n, seed):
    q, r = torch.linalg.qr(torch.randn(n, 3, 3, generator=_gen(seed), dtype=F64))
    q = q * torch.sign(torch.diagonal(r, dim1=1, dim2=2)).unsqueeze(1)
    return q * torch.linalg.det(q).view(n, 1, 1)              # det +1 (3 x 3: negating flips the sign)


def _affine(A, t):
    out = torch.zeros(A.shape[0], 4, 4, dtype=F64)
    out[:, :3, :3], out[:, :3, 3], out[:, 3, 3] = A, t, 1.0
    return out


def _translations(n, seed, half=0.5):
    return (torch.rand(n, 3, generator=_gen(seed), dtype=F64) - 0.5) * 2 * half


def rigid(n, seed):
    return _affine(rotations(n, seed), _translations(n, seed + 1)).float()


def blend(n, seed):
    """Four random rigid transforms under random convex weights: what smpl_skin_kernel's T is."""
    w = torch.rand(n, 4, generator=_gen(seed), dtype=F64) + 0.05
    w = w / w.sum(1, keepdim=True)
    parts = torch.stack([_affine(rotations(n, seed + 1 + k), _translations(n, seed + 5 + k)) for k in range(4)], dim=1)
    return (w.view(n, 4, 1, 1) * parts).sum(1).float()


def cond_bucket(n, c, seed):
    """rotation x diag(1, c^-1/2, c^-1) x rotation plus a translation: the 3 x 3 block has condition number c exactly."""
    d = torch.diag(torch.tensor([1.0, c ** -0.5, 1.0 / c], dtype=F64))
    return _affine(rotations(n, seed) @ d @ rotations(n, seed + 1), _translations(n, seed + 2, half=0.25)).float()


def general(n, seed, cmax=30.0):
    """Full 4 x 4 matrices, no structure in the last row: U diag(s) V' with random orthogonal U, V, log-spaced s from 1 to 1 / c,
    c uniform in [2, cmax / 1.5] so that fp32 rounding keeps the condition number under cmax."""
    g = _gen(seed)
    u, _ = torch.linalg.qr(torch.randn(n, 4, 4, generator=g, dtype=F64))
    v, _ = torch.linalg.qr(torch.randn(n, 4, 4, generator=g, dtype=F64))
    c = 2.0 + torch.rand(n, 1, generator=g, dtype=F64) * (cmax / 1.5 - 2.0)
    s = c ** (-torch.arange(4, dtype=F64).view(1, 4) / 3.0)
    return (u @ torch.diag_embed(s) @ v.transpose(1, 2)).float()


# where each bucket's name says its condition numbers lie: [lo, hi) of cond2 of the 4 x 4 (the translation column raises a
# rigid transform's to at most (1 + |t|)^2 and a c-bucket's by a similar factor)
BUCKET_COND = {"rigid": (1.0, 10.0), "c30": (30.0, 30.0 * 10 ** 0.5), "c300": (300.0, 300.0 * 10 ** 0.5),
               "c3000": (3000.0, 3000.0 * 10 ** 0.5), "general": (1.0, 30.0)}


@functools.lru_cache(maxsize=None)
def bucket(name, n=BUCKET_N):
    """(T_src, T_tgt) fp32 (n,4,4); T_tgt is rigid."""
    k = BUCKETS.index(name)
    src = {"rigid": lambda: rigid(n, 100), "blend": lambda: blend(n, 200), "general": lambda: general(n, 300),
           "c30": lambda: cond_bucket(n, 30.0, 400), "c300": lambda: cond_bucket(n, 300.0, 500),
           "c3000": lambda: cond_bucket(n, 3000.0, 600)}[name]()
    return src, rigid(n, 700 + k)


@functools.lru_cache(maxsize=None)
def inverse_ref_errors():
    """({bucket: (worst, median)}, worst over ASSERTED_BUCKETS) of the fp32 reference expression T_tgt @ torch.inverse(T_src)
    on the CPU, in normalised_inverse_error's units."""
    per = {}
    for name in BUCKETS:
        src, tgt = bucket(name)
        e = normalised_inverse_error(tgt @ torch.inverse(src), frame_transforms(src, tgt), src)
        per[name] = (float(e.max()), float(e.median()))
    return per, max(per[name][0] for name in ASSERTED_BUCKETS)


# ---------------------------------------------------------------------------------------------------- the LBS cases of the GPU file
@functools.lru_cache(maxsize=None)
def lbs_cases():
    """{name: dict(V, tree, pose, betas)}: every launch of tests/test_gpu_smpl.py that is held to the oracle."""
    cases = {}
    pose, betas = synth.smpl_pose(5, batch=2, scale=0.6)
    for V in LBS_V:
        cases[f"V{V}"] = dict(V=V, tree="standard", pose=pose, betas=betas)
    for name in TREES:
        for scale in TREE_SCALES:
            p, b = synth.smpl_pose(6, batch=2, scale=scale)
            cases[f"{name}_s{scale}"] = dict(V=V_EDGE, tree=name, pose=p, betas=b)
    cases["special"] = dict(V=V_EDGE, tree="standard", pose=special_poses(), betas=synth.smpl_pose(7, batch=7)[1])
    p, b = synth.smpl_pose(8, batch=3, scale=0.6)
    R = rodrigues(p.reshape(-1, 3)).view(3, 24, 3, 3).float().numpy()          # the oracle's Rodrigues output rounded to fp32
    cases["rotmat"] = dict(V=V_EDGE, tree="standard", pose=R, betas=b)
    p, b = synth.smpl_pose(9, batch=B_MAX, scale=0.6)
    cases[f"B{B_MAX}"] = dict(V=3, tree="standard", pose=p, betas=b)
    return cases


@functools.lru_cache(maxsize=None)
def lbs_oracle(name):
    c = lbs_cases()[name]
    return lbs(model(c["V"], c["tree"]), c["pose"], c["betas"])


def ref_rows(name):
    """The batch rows smpl_ref evaluates for the yardstick: all of them, but every 16th of the B_MAX case (smpl_ref loops over
    the batch in Python; rows are independent, and 4096 draws of the same distribution measure its fp32 distance as well)."""
    B = lbs_cases()[name]["pose"].shape[0]
    return slice(None) if B < 4096 else slice(0, B, 16)


@functools.lru_cache(maxsize=None)
def lbs_ref32(name):
    """fp32 oracle/smpl_ref.py on the case: (verts, T) of the batch rows ref_rows(name)."""
    from oracle import smpl_ref
    c = lbs_cases()[name]
    o = smpl_ref.SMPL(model(c["V"], c["tree"]))
    rows = ref_rows(name)
    pose, betas = torch.from_numpy(c["pose"])[rows], torch.from_numpy(c["betas"])[rows]
    return o.forward(pose, betas), o.get_vertex_transformation(pose, betas)


@functools.lru_cache(maxsize=None)
def lbs_yardsticks():
    """({case: {"verts": d, "T": d}}, {"verts": median, "T": median}): fp32 smpl_ref's max-rel distance from the float64 oracle."""
    per = {}
    for name in lbs_cases():
        v32, T32 = lbs_ref32(name)
        o = lbs_oracle(name)
        rows = ref_rows(name)
        per[name] = {"verts": relerr(v32, o["verts"][rows]), "T": relerr(T32, o["T"][rows])}
    med = {k: float(np.median([d[k] for d in per.values()])) for k in ("verts", "T")}
    return per, med


def bar(kind, own, median):
    """(bar, yardstick).  The yardstick of one tensor of one case is the larger of fp32 smpl_ref's own distance from float64 on
    the same inputs and the median of that distance over the cases (one fp32-vs-float64 pair is a single draw: the rule of
    helpers._check_grads_vs_float64); the bar is MARGIN x that, never above the existing contract."""
    yard = max(own, median)
    return min(MARGIN * yard, CONTRACT[kind]), yard


# -------------------------------------------------------------------------------------------- mf_apply_vertex_transforms' cases
@functools.lru_cache(maxsize=None)
def apply_trans(V):
    return blend(V, 900 + V % 97)


@functools.lru_cache(maxsize=None)
def apply_case(Q, V):
    """(trans (V,4,4) fp32, ind (Q,) int64 with duplicates, query (Q,3) fp32)."""
    g = _gen(1000 + Q * 7 + V)
    ind = torch.randint(0, V, (Q,), generator=g)
    if Q >= 2:
        ind[Q // 2] = ind[0]                                  # a duplicate even where V > Q
    query = (torch.rand(Q, 3, generator=g) - 0.5) * 3.0
    return apply_trans(V), ind, query


@functools.lru_cache(maxsize=None)
def apply_yardsticks():
    from oracle import smpl_ref
    per = {}
    for Q in APPLY_Q:
        for V in APPLY_V:
            trans, ind, query = apply_case(Q, V)
            per[(Q, V)] = relerr(smpl_ref.apply_vertex_transforms(trans, ind, query), apply_vertex_transforms(trans, ind, query))
    return per, float(np.median(list(per.values())))
