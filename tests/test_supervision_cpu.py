"""moco_flow_amd.supervision without a GPU: the package's exports and ctypes prototypes, the host-side argument validation of
mf_point_correspond / mf_point_loss_partials / mf_point_loss_partials_backward (include/mocoflow_hip.h) -- every refusal comes
before any launch --, the Python layer's refusals, and the torch restatement of the reference lines
(tests/supervision_oracle.py) on hand-computed values."""
import ctypes
import math

import pytest
import torch

import supervision_oracle as O


@pytest.fixture(scope="module")
def S():
    import moco_flow_amd
    return moco_flow_amd.supervision


def test_package_exports_supervision():
    import moco_flow_amd
    import moco_flow_amd._lib as L
    names = {"Correspondence", "correspondence", "point_correspond", "point_losses"}
    assert set(moco_flow_amd.supervision.__all__) == names
    for n in names | {"supervision"}:
        assert n in moco_flow_amd.__all__ and hasattr(moco_flow_amd, n)
    assert moco_flow_amd.point_losses is moco_flow_amd.supervision.point_losses
    lib = L.lib()
    C, P = ctypes, ctypes.c_void_p
    want = {"mf_point_correspond": (C.c_int32, [P, P, C.c_int64, P, C.c_int64, P, P, C.c_int64, C.c_float, C.c_int32, P, P, P, P, P]),
            "mf_point_loss_partials_scratch_bytes": (C.c_int64, [C.c_int64]),
            "mf_point_loss_partials": (C.c_int32, [C.POINTER(L.mf_point_loss_args), P, P, P, P]),
            "mf_point_loss_partials_backward": (C.c_int32, [C.POINTER(L.mf_point_loss_args), P, P, P, P, P, P, P])}
    for sym, (res, args) in want.items():
        assert L.SYMBOLS[sym] == (res, args), sym
        fn = getattr(lib, sym)
        assert fn.restype is res and list(fn.argtypes) == args, sym
    assert lib.mf_version() == 16 and L.MF_ABI_VERSION == 16


def test_loss_args_struct_layout():
    """The POD of include/mocoflow_hip.h, field by field: natural alignment, pointers on 8-byte boundaries."""
    import moco_flow_amd._lib as L
    A = L.mf_point_loss_args
    off = {name: getattr(A, name).offset for name, _ in A._fields_}
    assert [off[k] for k in ("Q", "pairs", "inside", "use_all", "pred_bw", "pred_fw", "n_nerfs", "sigma", "delta")] == \
        [0, 8, 16, 24, 32, 40, 48, 56, 72]
    assert ctypes.sizeof(A) == 80


def test_point_correspond_abi_validates_on_the_host():
    import moco_flow_amd._lib as L
    lib = L.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)

    def call(V=2, query=p, q_given=1, pick=None, noise=None, q_near=0, lanes=0, verts=p, trans=p, pairs=p, inside=p):
        return lib.mf_point_correspond(verts, trans, V, query, q_given, pick, noise, q_near, 0.2, lanes, pairs, inside, None, None, None)

    assert call(V=0) == -1 and b"V=0" in lib.mf_last_error()
    assert call(V=-3) == -1 and b"V=-3" in lib.mf_last_error()
    assert call(V=1 << 31) == -1
    assert call(q_given=-1) == -1 and b"q_given=-1" in lib.mf_last_error()
    assert call(q_near=-2) == -1 and b"q_near=-2" in lib.mf_last_error()
    assert call(q_given=1 << 31) == -1 and b"2^31" in lib.mf_last_error()
    for bad in (3, 2, 8, 32, 128, -1):
        assert call(lanes=bad) == -1 and b"lanes_per_query=%d" % bad in lib.mf_last_error(), bad
    for missing in ("verts", "trans", "pairs", "inside"):
        assert call(**{missing: None}) == -1 and b"null" in lib.mf_last_error(), missing
    assert call(query=None) == -1 and b"null query" in lib.mf_last_error()
    assert call(q_near=1, pick=p) == -1 and b"pick or noise" in lib.mf_last_error()
    assert call(q_near=1, noise=p) == -1 and b"pick or noise" in lib.mf_last_error()
    assert call(q_given=0, query=None, verts=None, trans=None, pairs=None, inside=None) == 0          # nothing is launched


def _loss_args(L, p, **kw):
    a = L.mf_point_loss_args()
    a.Q, a.pairs, a.inside, a.pred_bw, a.pred_fw = 4, p, p, p, p
    for k, v in kw.items():
        if k == "sigma":
            for i, s in enumerate(v):
                a.sigma[i] = s
        else:
            setattr(a, k, v)
    return a


def test_point_loss_abi_validates_on_the_host():
    import moco_flow_amd._lib as L
    lib = L.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    # 5 doubles per workgroup of 256 rows; the grid stops growing at 256 workgroups
    sb = lib.mf_point_loss_partials_scratch_bytes
    assert sb(0) == 0 and sb(1) == 40 and sb(256) == 40 and sb(257) == 80
    assert sb(256 * 256) == 40 * 256 and sb(256 * 256 + 1) == 40 * 256 and sb(1 << 40) == 40 * 256
    assert sb(-1) == -1 and b"negative" in lib.mf_last_error()
    fwd = lambda a, out=p, scratch=p: lib.mf_point_loss_partials(ctypes.byref(a) if a is not None else None, out, None, scratch, None)
    bwd = lambda a, out=p, seeds=p, g=(None,) * 4: lib.mf_point_loss_partials_backward(ctypes.byref(a) if a is not None else None,
                                                                                       out, seeds, *g, None)
    for f, name in ((fwd, b"mf_point_loss_partials:"), (bwd, b"mf_point_loss_partials_backward:")):
        assert f(None) == -1 and name in lib.mf_last_error() and b"null" in lib.mf_last_error()
        assert f(_loss_args(L, p, Q=-1)) == -1 and b"negative Q=-1" in lib.mf_last_error()
        assert f(_loss_args(L, p, n_nerfs=3)) == -1 and b"n_nerfs=3" in lib.mf_last_error()              # more than two NeRFs
        assert f(_loss_args(L, p, n_nerfs=-1)) == -1
        assert f(_loss_args(L, p, pairs=None)) == -1 and b"null pairs" in lib.mf_last_error()
        assert f(_loss_args(L, p, n_nerfs=2, sigma=(p, None))) == -1 and b"sigma[1]" in lib.mf_last_error()
        assert f(_loss_args(L, p), out=None) == -1 and b"out6" in lib.mf_last_error()
    assert fwd(_loss_args(L, p), scratch=None) == -1 and b"scratch" in lib.mf_last_error()
    assert bwd(_loss_args(L, p), seeds=None) == -1 and b"seeds3" in lib.mf_last_error()
    assert bwd(_loss_args(L, p, pred_bw=None), g=(p, None, None, None)) == -1 and b"without its prediction" in lib.mf_last_error()
    assert bwd(_loss_args(L, p, pred_fw=None), g=(None, p, None, None)) == -1 and b"without its prediction" in lib.mf_last_error()
    assert bwd(_loss_args(L, p, n_nerfs=1, sigma=(p,)), g=(None, None, p, p)) == -1 and b"beyond n_nerfs=1" in lib.mf_last_error()
    assert bwd(_loss_args(L, p, Q=0, pairs=None)) == 0                                                    # nothing is launched


def test_python_layer_refusals(S):
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        S.point_correspond(torch.zeros(4, 3), torch.zeros(4, 4, 4), torch.zeros(2, 3), 0.2)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        S.correspondence(None, torch.zeros(1, 72), torch.zeros(1, 10), torch.zeros(1, 72), torch.zeros(1, 10), 8)
    corr = S.Correspondence(torch.zeros(4, 6), torch.zeros(4, dtype=torch.uint8), torch.zeros(4), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(NotImplementedError, match="nof_loss='MSE'"):
        S.point_losses(corr, 0.0, None, None, (None, None), nof_loss="MSE")
    with pytest.raises(NotImplementedError, match="msk_loss='L1'"):
        S.point_losses(corr, 0.0, None, None, (None, None), msk_loss="L1")
    with pytest.raises(RuntimeError, match="1 deltas for 2 NeRFs"):
        S.point_losses(corr, 0.0, None, None, (None, None), nerfs=(object(), object()), deltas=(0.1,))
    with pytest.raises(RuntimeError, match="3 NeRFs"):
        S.point_losses(corr, 0.0, None, None, (None, None), nerfs=(object(),) * 3, deltas=(0.1,) * 3)
    with pytest.raises(RuntimeError, match="unknown term"):
        S.point_losses(corr, 0.0, None, None, (None, None), terms=("nof_sideways",))
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        S.point_losses(corr, 0.0, None, None, (None, None), terms=("nof_bw",))
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        S.loss_means(corr.pairs, corr.inside, pred_bw=torch.zeros(4, 3))


def test_oracle_on_hand_computed_values():
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    # two vertices on the x axis; the first point is exactly between them (a tie: the lower index), the second exactly at
    # dist == thickness from vertex 1 (outside: the comparison is strict), the third 0.125 from vertex 1
    verts = f([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
    query = f([[0.5, 0.0, 0.0], [1.0, 0.25, 0.0], [1.0, 0.0, -0.125]])
    trans = torch.eye(4).repeat(2, 1, 1)
    trans[0, :3, 3] = f([1.0, 2.0, 3.0])                                     # vertex 0: a translation
    trans[1, :3, :3] = 2 * torch.eye(3)                                      # vertex 1: a scaling
    pairs, inside, dist, ind = O.correspondence(verts, trans, query, 0.25)
    assert ind.tolist() == [0, 1, 1] and dist.tolist() == [0.5, 0.25, 0.125] and inside.tolist() == [False, False, True]
    assert torch.equal(pairs[:, :3], query)
    assert torch.equal(pairs[:, 3:], f([[1.5, 2.0, 3.0], [2.0, 0.5, 0.0], [2.0, 0.0, -0.25]]))
    ins, outs = O.split(pairs, inside)
    assert ins.shape == (1, 6) and outs.shape == (2, 6) and torch.equal(outs[1], pairs[1])
    # the sampling: cube points first, then verts[pick] + noise * thickness
    q = O.sample_queries(verts, f([[0.5, 1.0, 0.0]]), torch.tensor([1]), f([[1.0, -2.0, 0.0]]), 0.25)
    assert torch.equal(q, f([[0.0, 1.5, -1.5], [1.25, -0.5, 0.0]]))
    # L1 over the one inside row, both directions; all_points takes the three rows
    pred_bw = pairs[:, 3:] + f([[1.0, 1.0, 1.0], [0.0, 0.0, 0.0], [0.5, -0.25, 0.0]])
    pred_fw = pairs[:, :3] - 2.0
    sig = f([25.0, 0.0, -3.0])                                               # 25: above the softplus threshold of 20
    got = O.point_losses(pairs, inside, pred_bw, pred_fw, [sig, sig], [1 / 128, 1 / 256])
    assert got["nof_bw"][1] == 3 and float(got["nof_bw"][0]) == 0.25 and got["nof_fw"][1] == 3 and float(got["nof_fw"][0]) == 2.0
    every = O.point_losses(pairs, inside, pred_bw, pred_fw, all_points=True)
    assert every["nof_bw"][1] == 9 and float(every["nof_bw"][0]) == pytest.approx(3.75 / 9, rel=1e-6)
    # BCE against zero of alpha = 1 - exp(-delta softplus(sigma)) is delta softplus(sigma): at sigma = 25 softplus is the
    # identity, 25 / 128 and 25 / 256; at 0 it is log 2.  (1 - alpha carries half an ulp of 1, 3e-8, and so does its logarithm)
    assert got["alphas_mask"][1] == 4                                        # two outside rows x two NeRFs
    rows = O.bce_rows(sig, 1 / 128)
    assert float(rows[0]) == pytest.approx(25 / 128, abs=3e-7) and float(rows[1]) == pytest.approx(math.log(2.0) / 128, abs=3e-7)
    want = (25 / 128 + 25 / 256 + math.log(2.0) * (1 / 128 + 1 / 256)) / 4
    assert float(got["alphas_mask"][0]) == pytest.approx(want, abs=3e-7)
    assert float(O.bce_rows(f([200.0]), 1.0)) == 100.0                       # log(1 - 1) = -inf, clamped at -100
    # empty sets: value 0, count 0
    none = O.point_losses(pairs, torch.zeros(3, dtype=torch.bool), pred_bw, pred_fw)
    assert float(none["nof_bw"][0]) == 0.0 and none["nof_bw"][1] == 0 and none["nof_fw"][1] == 0
