"""Matte clean-up on the MI355X: frames.clean_mask and frames.mask_regions (csrc/mf_regions.hip) against the numpy oracle of their
contract (tests/regions_oracle.py), exactly (torch.equal: integers, no tolerance anywhere).  The canvas is (3 TH + 5) x (2 TW + 3)
with the tile size read from the source: every kind of tile seam, ragged last tiles, more than one workgroup.  The seam and the
no-wrap cases are the ones that catch a wrong kernel; the long paths and the late equivalences are hard on a concurrent
union-find; one stack runs past the first trip of every grid-stride loop."""
import os
import re

import numpy as np
import pytest
import torch

import regions_oracle as RO
import streams_util as SU

HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = open(os.path.join(HERE, "..", "moco_flow_amd", "csrc", "mf_regions.hip")).read()
TH, TW, THREADS, MAX_BLOCKS = (int(re.search(rf"constexpr int {n} = (\d+);", _SRC).group(1))
                               for n in ("kRegTileH", "kRegTileW", "kRegThreads", "kRegMaxBlocks"))
H0, W0 = 3 * TH + 5, 2 * TW + 3

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def FR():
    from moco_flow_amd import frames
    return frames


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def alpha_of(m):
    return np.where(np.asarray(m), 255, 0).astype(np.uint8)


def assert_regions(FR, alpha, what="", thres=196, conn=8, below=False, want=None):
    """mask_regions on the device equals the oracle's labels, counts and table; returns the oracle's."""
    want = RO.regions(alpha, thres, conn, below) if want is None else want
    got = FR.mask_regions(dev(alpha), thres, conn, below)
    torch.cuda.synchronize()
    assert isinstance(got, FR.Regions)
    for name, g, w, dt in zip(("labels", "counts", "table"), got, want, (torch.int32, torch.int64, torch.int32)):
        assert g.is_cuda and g.dtype == dt and tuple(g.shape) == w.shape, (what, conn, name, tuple(g.shape), w.shape)
        assert torch.equal(g.cpu(), torch.from_numpy(w)), (what, conn, name)
    return want


def assert_clean(FR, alpha, what="", **kw):
    want = RO.clean_mask(alpha, kw.get("thres", 196), kw.get("largest", True), kw.get("min_area", 0), kw.get("fill_holes", False))
    got = FR.clean_mask(dev(alpha), **kw)
    torch.cuda.synchronize()
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == want.shape, (what, kw)
    assert torch.equal(got.cpu(), torch.from_numpy(want)), (what, kw)
    return want


# ---------------------------------------------------------------- connectivity
@pytest.mark.parametrize("conn", (8, 4))
def test_pixels_joined_only_across_a_tile_seam(FR, conn):
    pairs = RO.seam_pairs(TH, TW)
    alpha = np.zeros((len(pairs), H0, W0), dtype=np.uint8)
    for f, (_, a, b, _) in enumerate(pairs):
        alpha[f][a] = alpha[f][b] = 255
    labels, counts, table = assert_regions(FR, alpha, "seams", conn=conn)
    for f, (name, a, b, joined4) in enumerate(pairs):
        joined = conn == 8 or joined4
        assert (labels[f][a] == labels[f][b]) == joined and counts[f] == (1 if joined else 2), name
    if conn == 8:
        assert table[:, 2].tolist() == [2] * len(pairs)


@pytest.mark.parametrize("conn", (8, 4))
def test_rows_and_frames_do_not_wrap(FR, conn):
    alpha = np.zeros((3, H0, W0), dtype=np.uint8)
    alpha[0, 7, W0 - 1] = alpha[0, 8, 0] = 255                  # consecutive in memory, a row apart
    alpha[0, TH - 1, W0 - 1] = alpha[0, TH, 0] = 255            # the same across a tile seam
    alpha[1, H0 - 1, W0 - 1] = alpha[2, 0, 0] = 255             # the last pixel of a frame and the first of the next
    alpha[1, 0, W0 - 1] = alpha[0, H0 - 1, 0] = 255
    labels, counts, table = assert_regions(FR, alpha, "no wrap", conn=conn)
    assert counts.tolist() == [5, 2, 1] and (table[:, 2] == 1).all()
    assert labels[2, 0, 0] == 0 and labels[1, H0 - 1, W0 - 1] == H0 * W0 - 1


@pytest.mark.parametrize("conn", (8, 4))
def test_long_paths_and_late_equivalences(FR, conn):
    makers = (RO.serpentine, RO.spirals, RO.comb, RO.nested_us)
    alpha = alpha_of(np.stack([make(H0, W0) for make in makers]))
    labels, counts, table = assert_regions(FR, alpha, "paths", conn=conn)
    assert counts[0] == 1 and table[0].tolist() == [0, 0, RO.serpentine_area(H0, W0), 0, 0, W0 - 1, H0 - 1]
    assert counts[1] == 2 and counts[2] == 1 and labels[2].max() == 0
    us = table[table[:, 0] == 3]
    assert us[:, 1].tolist() == list(range(0, 2 * len(us), 2)) and len(us) == counts[3] > 10
    assert_clean(FR, alpha, "paths")
    assert_clean(FR, alpha, "paths", fill_holes=True)


def test_extremes(FR):
    checker = (np.add.outer(np.arange(H0), np.arange(W0)) % 2 == 0)
    alpha = alpha_of(np.stack([np.ones((H0, W0), bool), np.zeros((H0, W0), bool), checker]))
    _, counts, table = assert_regions(FR, alpha, "extremes", conn=8)
    assert counts.tolist() == [1, 0, 1] and table.tolist() == [[0, 0, H0 * W0, 0, 0, W0 - 1, H0 - 1],
                                                             [2, 0, (H0 * W0 + 1) // 2, 0, 0, W0 - 1, H0 - 1]]
    _, counts, table = assert_regions(FR, alpha, "extremes", conn=4)
    assert counts.tolist() == [1, 0, (H0 * W0 + 1) // 2] and (table[1:, 2] == 1).all()
    out = assert_clean(FR, alpha, "extremes", fill_holes=True)
    assert out[0].min() == 255 and out[1].max() == 0
    none = np.zeros((2, H0, W0), dtype=np.uint8)
    _, counts, table = assert_regions(FR, none, "no members")
    assert counts.tolist() == [0, 0] and table.shape == (0, 7)
    assert assert_clean(FR, none, "no members", fill_holes=True).max() == 0


@pytest.mark.parametrize("shape", ((1, 1), (1, W0), (H0, 1), (TH, TW), (TH - 1, TW - 1), (TH + 1, TW + 1), (2, 2 * TW + 1), (2 * TH + 1, 2)))
def test_small_and_tile_sized_shapes(FR, shape):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    alpha = alpha_of(rng.random((3,) + shape) < np.array([0.5, 0.62, 1.0])[:, None, None])
    for conn in (8, 4):
        assert_regions(FR, alpha, shape, conn=conn)
    for kw in (dict(), dict(largest=False, min_area=2), dict(fill_holes=True)):      # 1 x W: runs of equal length tie
        assert_clean(FR, alpha, shape, **kw)


# ---------------------------------------------------------------- values and selection
@pytest.mark.parametrize("density", (0.30, 0.42, 0.50, 0.62))
def test_random_masks(FR, density):
    rng = np.random.default_rng(int(density * 100))
    alpha = rng.integers(0, 256, size=(3, H0, W0), dtype=np.uint8)
    thres = int(round(256 * (1 - density)))
    for conn in (8, 4):
        labels, counts, table = assert_regions(FR, alpha, density, thres=thres, conn=conn)
        assert table[:, 2].sum() == (alpha >= thres).sum() and counts.sum() == len(table)
    print(f"density {density}: {counts.tolist()} regions, largest {np.sort(table[:, 2])[::-1][:3].tolist()}")
    for kw in (dict(), dict(largest=False, min_area=1), dict(largest=False, min_area=2), dict(largest=False, min_area=50),
               dict(min_area=50), dict(min_area=2, fill_holes=True), dict(largest=False, min_area=10 ** 12)):
        assert_clean(FR, alpha, density, thres=thres, **kw)


def test_a_tie_for_the_largest_goes_to_the_smaller_label(FR):
    alpha = np.zeros((2, H0, W0), dtype=np.uint8)
    alpha[0, 40:43, 100:104] = 255                               # three regions of 12 pixels in three tiles
    alpha[0, 2:6, 70:73] = 255
    alpha[0, TH + 1, 3:15] = 255
    alpha[0, 0, 0] = 255
    alpha[1, H0 - 1, 0:5] = alpha[1, 0, W0 - 5:] = 255           # two of 5
    out = assert_clean(FR, alpha, "tie")
    assert out[0, 2:6, 70:73].min() == 255 and out[0].sum() == 12 * 255 and out[1, 0].sum() == 5 * 255 == out[1].sum()


def test_threshold_and_below(FR):
    rng = np.random.default_rng(7)
    alpha = rng.choice(np.array([0, 195, 196, 197, 255], dtype=np.uint8), size=(2, H0, W0))
    _, c196, _ = assert_regions(FR, alpha, "196")
    assert_regions(FR, alpha, "197", thres=197)
    _, c0, t0 = assert_regions(FR, alpha, "0", thres=0)
    _, c256, _ = assert_regions(FR, alpha, "256", thres=256)
    assert c0.tolist() == [1, 1] and t0[0, 2] == H0 * W0 and c256.tolist() == [0, 0]
    labels, _, _ = assert_regions(FR, alpha, "below", below=True)
    assert ((labels >= 0) == (alpha < 196)).all()
    assert_regions(FR, alpha, "below 256", thres=256, below=True, conn=4)
    assert_clean(FR, alpha, "196")
    assert assert_clean(FR, alpha, "0", thres=0).min() == 255
    assert assert_clean(FR, alpha, "256", thres=256).max() == 0


def hole_cases():
    def blank():
        return np.zeros((H0, W0), dtype=bool)
    cases = {}
    m = blank(); m[5:30, 10:100] = True; m[8:27, 13:97] = False; cases["ring"] = m.copy()
    m[15:18, 40:50] = True; cases["ring with island"] = m.copy()
    m[12:21, 30:60] = True; m[14:19, 33:57] = False; cases["ring inside the hole of a ring"] = m.copy()
    for side in range(4):
        m = blank(); m[10:40, 20:90] = True
        if side == 0: m[0:11, 30:60] = True; m[0:9, 33:57] = False
        if side == 1: m[38:H0, 30:60] = True; m[41:H0, 33:57] = False
        if side == 2: m[20:30, 0:21] = True; m[22:28, 0:18] = False
        if side == 3: m[20:30, 88:W0] = True; m[22:28, 92:W0] = False
        cases[f"bay on border {side}"] = m
    m = blank(); m[0:20, 0:40] = True; m[1:10, 1:30] = False; m[5, 0] = False; cases["a hole touching the border by one pixel"] = m
    m = blank(); m[0:20, 0:40] = True; m[1:10, 1:30] = False; cases["the same hole, closed"] = m
    m = blank(); m[20:30, 20] = m[20:30, 40] = m[20, 20:41] = m[30, 20:40] = True; cases["diagonal-only leak"] = m    # gap (30, 40)
    m = blank(); m[TH - 3:TH + 4, TW - 3:TW + 4] = True; m[TH - 1:TH + 2, TW - 1:TW + 2] = False; cases["hole over a tile corner"] = m
    return cases


@pytest.mark.parametrize("largest", (True, False))
def test_holes(FR, largest):
    cases = hole_cases()
    alpha = alpha_of(np.stack(list(cases.values())))
    plain = assert_clean(FR, alpha, "holes", largest=largest)
    filled = assert_clean(FR, alpha, "holes", largest=largest, fill_holes=True)
    names = list(cases)
    f = names.index
    assert filled[f("ring")][5:30, 10:100].min() == 255 and filled[f("ring")].sum() == 25 * 90 * 255
    assert np.array_equal(filled[f("ring with island")], filled[f("ring")])          # the island goes, or drowns in the hole
    assert np.array_equal(filled[f("ring inside the hole of a ring")], filled[f("ring")])
    assert plain[f("ring with island")][16, 45] == (0 if largest else 255)
    for side in range(4):
        k = f(f"bay on border {side}")
        assert np.array_equal(filled[k], plain[k]), side
    k = f("a hole touching the border by one pixel")
    assert np.array_equal(filled[k], plain[k]) and filled[f("the same hole, closed")][1:10, 1:30].min() == 255
    k = f("diagonal-only leak")
    assert filled[k][21:30, 21:40].min() == 255 and filled[k][30, 40] == 0 and plain[k][25, 30] == 0
    assert filled[f("hole over a tile corner")][TH - 3:TH + 4, TW - 3:TW + 4].min() == 255


@pytest.mark.parametrize("shape", ((2, 9), (9, 2), (1, 5), (3, 3)))
def test_nothing_to_fill_in_two_rows_or_columns(FR, shape):
    m = np.ones((2,) + shape, dtype=bool)
    m[0, shape[0] // 2, shape[1] // 2] = False
    out = assert_clean(FR, alpha_of(m), shape, fill_holes=True)
    assert (out[0].min() == 255) == (shape == (3, 3))


# ---------------------------------------------------------------- plumbing and repeatability
def test_rgba_is_read_in_place(FR):
    rng = np.random.default_rng(21)
    rgba = rng.integers(0, 256, size=(3, H0, W0, 4), dtype=np.uint8)
    alpha = np.ascontiguousarray(rgba[..., 3])
    want = assert_clean(FR, alpha, "alpha", thres=128, fill_holes=True)
    want_regions = RO.regions(alpha, 128)
    d = dev(rgba)
    keep = d.clone()
    for arg in (d, d[..., 3]):
        assert torch.equal(FR.clean_mask(arg, thres=128, fill_holes=True).cpu(), torch.from_numpy(want))
        got = FR.mask_regions(arg, 128)
        for g, w in zip(got, want_regions):
            assert torch.equal(g.cpu(), torch.from_numpy(w))
    assert torch.equal(d, keep)
    for arg, w in ((d[1], want[1]), (d[1, ..., 3], want[1]), (d[1, ..., 3].contiguous(), want[1])):       # single images
        got = FR.clean_mask(arg, thres=128, fill_holes=True)
        assert tuple(got.shape) == (H0, W0) and torch.equal(got.cpu(), torch.from_numpy(w))
    one = FR.mask_regions(d[2], 128)
    assert tuple(one.labels.shape) == (H0, W0) and tuple(one.counts.shape) == (1,)
    assert torch.equal(one.labels.cpu(), torch.from_numpy(want_regions[0][2]))
    assert torch.equal(one.table[:, 1:].cpu(), torch.from_numpy(want_regions[2][want_regions[2][:, 0] == 2][:, 1:]))


def test_chunks_of_frames_equal_the_whole(FR, monkeypatch):
    rng = np.random.default_rng(33)
    alpha = dev(alpha_of(rng.random((7, H0, W0)) < 0.45))
    whole_mask = FR.clean_mask(alpha, fill_holes=True)
    whole = FR.mask_regions(alpha)
    assert FR._region_chunk(7, H0, W0) == 7
    monkeypatch.setattr(FR, "SCRATCH_BUDGET", 12 * H0 * W0 * 3 + 5)
    assert FR._region_chunk(7, H0, W0) == 3                      # three chunks, a ragged last one
    assert torch.equal(FR.clean_mask(alpha, fill_holes=True), whole_mask)
    for g, w in zip(FR.mask_regions(alpha), whole):
        assert torch.equal(g, w)
    assert torch.equal(whole_mask.cpu(), torch.from_numpy(RO.clean_mask(alpha.cpu().numpy(), fill=True)))


def test_past_the_first_trip_of_every_loop(FR):
    # one large frame pair: more tiles than workgroups, more pixels than threads, ragged last trip; closed forms
    H = 2 * TH * 16 + 8
    W = (MAX_BLOCKS // (2 * -(-H // TH)) + 1) * TW + 12
    assert 2 * -(-H // TH) * -(-W // TW) > MAX_BLOCKS and 2 * H * W > THREADS * MAX_BLOCKS and (2 * H * W) % (THREADS * MAX_BLOCKS) != 0
    m = np.zeros((2, H, W), dtype=bool)
    m[0] = RO.serpentine(H, W)
    m[1, 0::2] = True                                            # stripes: region y W of W pixels per even row
    labels = np.where(m, 0, -1).astype(np.int32)
    labels[1] = np.where(m[1], (np.arange(H) * W)[:, None], -1)
    ys = np.arange(0, H, 2)
    stripes = np.stack([np.ones_like(ys), ys * W, np.full_like(ys, W), np.zeros_like(ys), ys, np.full_like(ys, W - 1), ys], axis=1)
    table = np.concatenate([[[0, 0, RO.serpentine_area(H, W), 0, 0, W - 1, H - 1]], stripes]).astype(np.int32)
    counts = np.array([1, len(ys)], dtype=np.int64)
    for conn in (8, 4):
        assert_regions(FR, alpha_of(m), "large", conn=conn, want=(labels, counts, table))
    got = FR.clean_mask(dev(alpha_of(m)), fill_holes=True)
    assert torch.equal(got[0].cpu(), torch.from_numpy(alpha_of(m[0]))) and int(got[1].sum()) == 255 * W and int(got[1, 0].sum()) == 255 * W
    # many small frames, four ragged tiles each: a 0.42 random mask by the oracle
    h, w = TH + 1, TW + 1
    F = max(-(-(MAX_BLOCKS + 1) // 4), -(-(THREADS * MAX_BLOCKS + 1) // (h * w))) + 1
    alpha = alpha_of(np.random.default_rng(42).random((F, h, w)) < 0.42)
    assert_regions(FR, alpha, "many frames")
    assert_clean(FR, alpha, "many frames", fill_holes=True)


def test_scratch_may_hold_anything_and_repeats_are_identical(FR):
    import moco_flow_amd._lib as L
    rng = np.random.default_rng(55)
    alpha = dev(alpha_of(rng.random((3, H0, W0)) < 0.5))
    keep = alpha.clone()
    want = RO.clean_mask(alpha.cpu().numpy(), fill=True)
    want_regions = RO.regions(alpha.cpu().numpy())
    sizes = (int(L.lib().mf_mask_label_scratch_bytes(3, H0, W0)), 4 * alpha.numel(), alpha.numel(), 28 * len(want_regions[2]), 8 * 3)
    runs = []
    for _ in range(2):
        SU.poison(sizes)
        mask = FR.clean_mask(alpha, fill_holes=True)
        SU.poison(sizes)
        reg = FR.mask_regions(alpha)
        runs.append((mask,) + tuple(reg))
    torch.cuda.synchronize()
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert torch.equal(runs[0][0].cpu(), torch.from_numpy(want))
    for g, w in zip(runs[0][1:], want_regions):
        assert torch.equal(g.cpu(), torch.from_numpy(w))
    assert torch.equal(alpha, keep)                              # the input is left alone


def test_clean_mask_makes_no_host_synchronisation(FR):
    rng = np.random.default_rng(66)
    alpha = dev(alpha_of(rng.random((3, H0, W0)) < 0.5))
    rgba = dev(rng.integers(0, 256, size=(2, H0, W0, 4), dtype=np.uint8))
    FR.clean_mask(alpha, fill_holes=True)                        # the library is loaded
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = FR.clean_mask(alpha, fill_holes=True)
        out2 = FR.clean_mask(rgba, thres=100, largest=False, min_area=3, fill_holes=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(out.cpu(), torch.from_numpy(RO.clean_mask(alpha.cpu().numpy(), fill=True)))
    assert torch.equal(out2.cpu(), torch.from_numpy(RO.clean_mask(rgba[..., 3].cpu().numpy(), 100, False, 3, True)))


def test_shapes_are_checked_and_empty_inputs_launch_nothing(FR):
    z = lambda *s: torch.zeros(s, dtype=torch.uint8, device="cuda")
    for bad in (z(5), z(2, 3, 4, 3), z(2, 3, 4, 4, 1)):
        for fn in (FR.clean_mask, FR.mask_regions):
            with pytest.raises(RuntimeError, match="alpha is"):
                fn(bad)
    for shape in ((0, 5, 6), (3, 0, 6), (3, 5, 0), (0, 5, 6, 4), (0, 6)):
        out = FR.clean_mask(z(*shape), fill_holes=True)
        want = shape[:-1] if len(shape) == 4 else shape
        assert tuple(out.shape) == want and out.dtype == torch.uint8
        reg = FR.mask_regions(z(*shape))
        assert tuple(reg.labels.shape) == want and tuple(reg.table.shape) == (0, 7) and int(reg.counts.sum()) == 0
        assert tuple(reg.counts.shape) == (shape[0] if len(want) == 3 else 1,)
