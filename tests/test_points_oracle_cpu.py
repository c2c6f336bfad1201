"""Preconditions of tests/test_gpu_point_queries.py on its own inputs, without a GPU: the point-query oracle
(tests/points_oracle.py) is the cpu_ref spelling when its hooks are off, and the distances the GPU bars are made of -- the
floor (the fast oracle with fp32 instead of float64 accumulation against itself), the deliberately wrong oracles, the
indices rolled by one point -- are far enough apart on the subset the GPU test compares that those bars can fail.

Measured here (769 points of the 65 793-point fast launch; floor l2-rel canonical point / sigma through the NoF /
canonical-space sigma): 1.7e-6 / 1.3e-3 / 3.1e-4; lo products of the NoF's xyz block dropped 70 x / 17 x the floor; the
NeRF's hidden operands split 22 x; indices rolled by one point 13 000 x / 470 x; bf16x3 (513 points of the 32 897-point
launch): 1.5e-5 / 1.3e-5 from the fp32 oracle, hidden activations unsplit 4.7e-3 / 4.7e-3."""
import functools
from dataclasses import replace

import torch

import points_oracle as P
from oracle import bf16_ref as B
from oracle import cpu_ref as R

NAMES = ("canonical point", "sigma through the NoF", "canonical-space sigma")


@functools.lru_cache(maxsize=None)
def _points(prec):
    n = P.second_trip(P.TILE[prec])
    xyz, ind = P.inputs(n)
    idx = P.subset(n, P.TILE[prec])
    return xyz[idx], ind[idx]


@functools.lru_cache(maxsize=None)
def _query(arith, prec, roll=0):
    sd_n, sd_f = P.states()
    xyz, ind = _points(prec)
    return P.point_query(arith, sd_n, sd_f, xyz, torch.roll(ind, roll))


def _floors():
    return [B.l2rel(a, b) for a, b in zip(_query(replace(B.BF16, acc="f32"), "bf16"), _query(B.BF16, "bf16"))]


def test_subset_covers_first_tile_second_trip_and_ragged_tail():
    for tile in (128, 256):
        n = P.second_trip(tile)
        idx = P.subset(n, tile, seed=3)
        assert n == (P.MI355X_CUS + 1) * tile + 1 and len(idx) == 2 * tile + 1 + 256
        assert torch.equal(idx, idx.unique())                                         # sorted, no repeats
        assert torch.equal(idx[:tile], torch.arange(tile))
        assert torch.equal(idx[-(tile + 1):], torch.arange(P.MI355X_CUS * tile, n))   # tiles #CUs and #CUs + 1
        mid = idx[tile:-(tile + 1)]
        assert int(mid.min()) >= tile and int(mid.max()) < P.MI355X_CUS * tile
        assert torch.equal(idx, P.subset(n, tile, seed=3)) and not torch.equal(idx, P.subset(n, tile, seed=4))
        for small in (1, tile - 1, tile, tile + 1, 3 * tile):
            assert torch.equal(P.subset(small, tile), torch.arange(small))
    xyz, ind = P.inputs(1000)
    assert len(set(P.IND_VALUES)) == 5 and all(-1.0 <= v < 1.0 for v in P.IND_VALUES)
    assert all(bool((ind[i::5] == v).all()) for i, v in enumerate(P.IND_VALUES))
    assert float(xyz.min()) >= -1.5 and float(xyz.max()) < 1.5


def test_hooks_off_is_the_cpu_ref_spelling():
    """point_query(F32) against test_fused_point_query's spelling: forward_nof_points for one frame index, nof_inference
    for a per-point index; NeRF(sigma_only) on the embedded point.  Bit for bit."""
    sd_n, sd_f = P.states()
    xyz, ind = _points("f32")
    onerf = R.NeRF(8, 256, 63, [4], "ind", 5, state=sd_n)
    onof = R.NoF(4, 128, 33, [2], "ind", 33, True, state=sd_f)
    with torch.no_grad():
        canon = R.nof_inference(xyz[:, None, :], ind[:, None], [R.Embedding(3, 5), R.Embedding(1, 16)], onof)[:, 0, :]
        sig = onerf(R.Embedding(3, 10)(canon), sigma_only=True)
        sig0 = onerf(R.Embedding(3, 10)(xyz), sigma_only=True)
        frame, num_frames = torch.tensor([17]), 300
        canon_s = R.forward_nof_points(xyz, frame, num_frames, R.Embedding(3, 5), R.Embedding(1, 16), onof)
        sig_s = onerf(R.Embedding(3, 10)(canon_s), sigma_only=True)
    got = _query(B.F32, "f32")
    assert torch.equal(got[0], canon) and torch.equal(got[1], sig) and torch.equal(got[2], sig0)
    ind_s = (frame.float() * 2 / num_frames - 1.0).expand(xyz.shape[0])
    got_s = P.point_query(B.F32, sd_n, sd_f, xyz, ind_s)
    assert torch.equal(got_s[0], canon_s) and torch.equal(got_s[1], sig_s) and torch.equal(got_s[2], sig0)
    none = P.point_query(B.F32, sd_n, None, xyz, None)
    assert none[0] is None and none[1] is None and torch.equal(none[2], sig0)


def test_floor_and_wrong_oracles_are_resolved():
    """The floor of each output on the fast launch's own subset, and every distance the GPU test relies on in floors."""
    own = _query(B.BF16, "bf16")
    floors = _floors()
    print("floors (l2-rel) " + " / ".join(f"{f:.2e}" for f in floors))
    # the order of magnitude of the floors, so that a degenerate (zero or percent-sized) floor is noticed here
    assert 5e-7 <= floors[0] <= 2e-5 and 3e-4 <= floors[1] <= 5e-3 and 5e-5 <= floors[2] <= 2e-3, floors
    no_lo = _query(replace(B.BF16, nof_xyz="plain"), "bf16")
    hid = _query(replace(B.BF16, nerf_hidden="split"), "bf16")
    f32 = _query(B.F32, "bf16")
    wrong = [B.l2rel(no_lo[0], own[0]) / floors[0], B.l2rel(no_lo[1], own[1]) / floors[1], B.l2rel(hid[2], own[2]) / floors[2]]
    far = [B.l2rel(a, b) / f for a, b, f in zip(f32, own, floors)]
    print("wrong oracles, in floors: " + " / ".join(f"{w:.1f}" for w in wrong) + "; the fp32 oracle: " + " / ".join(f"{w:.1f}" for w in far))
    for name, w, d in zip(NAMES, wrong, far):
        assert w >= 10.0, (name, w)
        assert d >= 10.0, (name, d)          # "closer to its own oracle than to F32" has room: 3 floors against >= 10
    assert torch.equal(no_lo[2], own[2]) and torch.equal(hid[0], own[0])      # each hook moves only what is behind it


def test_rolled_indices_move_the_flow():
    """Every point with its neighbour's image index: what a kernel reading another point's bias rows would compute."""
    own, rolled = _query(B.BF16, "bf16"), _query(B.BF16, "bf16", roll=1)
    floors = _floors()
    moved = [B.l2rel(rolled[k], own[k]) / floors[k] for k in (0, 1)]
    print(f"indices rolled by one point, in floors: canonical point {moved[0]:.0f}, sigma through the NoF {moved[1]:.0f}")
    assert moved[1] > 100.0 and moved[0] > 100.0, moved
    assert torch.equal(rolled[2], own[2])


def test_bf16x3_wrong_oracle_is_resolved():
    """The NeRF's hidden activations unsplit sit more than 100 x farther from BF16X3 than BF16X3 is from F32."""
    own, f32 = _query(B.BF16X3, "bf16x3"), _query(B.F32, "bf16x3")
    wrong = _query(replace(B.BF16X3, nerf_hidden="wsplit"), "bf16x3")
    for k in (1, 2):
        near, far = B.l2rel(own[k], f32[k]), B.l2rel(wrong[k], own[k])
        print(f"bf16x3 {NAMES[k]}: {near:.1e} from the fp32 oracle, hidden activations unsplit {far:.1e}")
        assert far > 100.0 * near, (NAMES[k], near, far)
    assert torch.equal(wrong[0], own[0])
