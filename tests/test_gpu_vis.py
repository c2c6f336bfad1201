"""moco_flow_amd.vis on the device (mf_vis.hip) against the numpy restatement of the reference (tests/vis_oracle.py).

Every comparison is EXACT -- torch.equal on the bytes and on the fp32 planes: the kernels restate the reference's fp32
arithmetic operation for operation (one rounding each), min and max do not depend on the order, and the table gather and
the division by 255 are the same fp32 operations on both sides.  An index that differs is a rounding bug in the kernel.

Sizes come from the unit's own constants: one workgroup's share of the range reduction +- 1, and one plane past the point
where the grid stops growing with more partials than the finishing workgroup has lanes."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import vis_oracle as O

pytestmark = pytest.mark.gpu

_SRC = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "moco_flow_amd", "csrc", "mf_vis.hip")).read()
_const = lambda name: int(re.search(r"\b%s = (\d+)" % name, _SRC).group(1))
RANGE_SHARE = _const("kRangeThreads") * _const("kRangePerThread")          # elements of one workgroup before the grid stops growing
RANGE_MAX_BLOCKS = _const("kRangeMaxBlocks")
FINISH_THREADS = _const("kRangeFinishThreads")
VIS_SHARE = _const("kVisThreads") * _const("kVisPerThread")                 # pixels of one colour-map / sheet workgroup
# past the cap (the last workgroups take a second trip) and more than one partial per finishing lane
BIG_N = RANGE_MAX_BLOCKS * RANGE_SHARE + RANGE_SHARE + 7
assert RANGE_MAX_BLOCKS > FINISH_THREADS
assert 37 * 53 > VIS_SHARE                                                  # the 37 x 53 cases span workgroups

PLANE_SHAPES = [(1, 1), (1, 63), (1, 65), (1, RANGE_SHARE - 1), (1, RANGE_SHARE), (1, RANGE_SHARE + 1), (37, 53)]


@pytest.fixture(scope="module")
def V():
    import moco_flow_amd
    return moco_flow_amd.vis


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def raw_range(t, nan_value=0.0):
    """mf_depth_range on a contiguous device tensor -> [min, max] as a host list."""
    import moco_flow_amd._lib as L
    lib = L.lib()
    out = torch.full((2,), -7.0, device="cuda")
    scratch = torch.empty(max(int(lib.mf_depth_range_scratch_bytes(t.numel())), 8), dtype=torch.uint8, device="cuda")
    L.check(lib.mf_depth_range(t.data_ptr(), t.numel(), nan_value, out.data_ptr(), scratch.data_ptr(), L.current_stream(t.device)),
            "mf_depth_range")
    return out.tolist()


@functools.lru_cache(maxsize=None)
def plane_case(shape):
    d = O.depth_plane(shape[0] * shape[1], seed=shape[0] * 1000 + shape[1]).reshape(shape)
    return d, O.visualize_depth(d)


@pytest.mark.parametrize("shape", PLANE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_range_and_visualize_depth(V, shape):
    d, want = plane_case(shape)
    g = dev(d)
    assert raw_range(g) == [float(d.min()), float(d.max())]
    got = V.visualize_depth(g)
    assert got.shape == (3,) + shape and got.dtype == torch.float32 and got.is_cuda
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    # the same plane one float into a larger buffer: contiguous, but not 16-byte aligned -- the scalar kernels
    buf = torch.full((d.size + 9,), 1e9, device="cuda")
    view = buf[1:1 + d.size].view(shape)
    view.copy_(g)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    assert raw_range(view) == [float(d.min()), float(d.max())]
    assert torch.equal(V.visualize_depth(view).cpu(), torch.from_numpy(want))
    assert float(buf[0]) == 1e9 and float(buf[1 + d.size]) == 1e9


def test_range_past_the_grid_cap(V):
    assert int(__import__("moco_flow_amd")._lib.lib().mf_depth_range_scratch_bytes(BIG_N)) == RANGE_MAX_BLOCKS * 8
    d = O.depth_plane(BIG_N, seed=77, sentinels=False)
    lo, hi = BIG_N - 3, RANGE_SHARE * (FINISH_THREADS + 5) + 1           # the min in the tail, the max in a partial of the second round
    d[lo], d[hi] = 1.25, 11.5
    g = dev(d)
    assert raw_range(g) == [1.25, 11.5]
    got = V.visualize_depth(g.view(1, BIG_N))
    assert torch.equal(got.cpu(), torch.from_numpy(O.visualize_depth(d.reshape(1, BIG_N))))
    # every element takes part: move the extremes through the plane's ends and a few workgroup seams
    for pos in (0, RANGE_SHARE - 1, RANGE_SHARE, RANGE_MAX_BLOCKS * RANGE_SHARE - 1, RANGE_MAX_BLOCKS * RANGE_SHARE, BIG_N - 1):
        e = g.clone()
        e[pos] = -3.0
        e[BIG_N - 1 - pos] = 99.0
        assert raw_range(e) == [-3.0, 99.0], pos


def test_nan_with_and_without_a_range(V):
    d = O.depth_plane(37 * 53, seed=5).reshape(37, 53)
    d[3, 4] = d[20, 52] = d[36, 0] = np.nan
    g = dev(d)
    assert raw_range(g) == [0.0, float(np.nanmax(d))]                       # NaN -> 0, which is then the minimum
    assert raw_range(g, nan_value=12.5) == [float(np.nanmin(d)), 12.5]
    assert torch.equal(V.visualize_depth(g).cpu(), torch.from_numpy(O.visualize_depth(d)))
    got = V.visualize_depth(g, 2.0, 10.0)                                   # NaN -> ma: the top colour
    assert torch.equal(got.cpu(), torch.from_numpy(O.visualize_depth(d, 2.0, 10.0)))
    lut = O.jet_lut()
    assert got[:, 3, 4].tolist() == (lut[255].astype(np.float32) / np.float32(255)).tolist()
    # only one of mi / ma: the reference ignores it (line 33)
    assert torch.equal(V.visualize_depth(g, mi=2.0).cpu(), torch.from_numpy(O.visualize_depth(d)))
    assert torch.equal(V.visualize_depth(g, ma=10.0).cpu(), torch.from_numpy(O.visualize_depth(d)))
    allnan = torch.full((2, 5), float("nan"), device="cuda")
    assert raw_range(allnan) == [0.0, 0.0]
    assert torch.equal(V.visualize_depth(allnan).cpu(), torch.from_numpy(O.visualize_depth(allnan.cpu().numpy())))


def test_constant_plane_is_index_zero(V):
    d = np.full((6, 7), 3.75, dtype=np.float32)
    got = V.visualize_depth(dev(d))
    want = O.visualize_depth(d)
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    lut = O.jet_lut()
    assert (got.cpu().numpy() == (lut[0].astype(np.float32) / np.float32(255))[:, None, None]).all()


def test_infinities(V):
    for vals in ((np.inf,), (-np.inf,), (np.inf, -np.inf), (np.inf, np.nan)):
        d = O.depth_plane(65, seed=9).reshape(5, 13)
        for j, v in enumerate(vals):
            d[j + 1, 2 * j + 3] = v
        g = dev(d)
        x = np.nan_to_num(d)
        assert raw_range(g) == [float(x.min()), float(x.max())]
        assert torch.equal(V.visualize_depth(g).cpu(), torch.from_numpy(O.visualize_depth(d))), vals
        assert torch.equal(V.visualize_depth(g, 2.0, 6.0).cpu(), torch.from_numpy(O.visualize_depth(d, 2.0, 6.0))), vals


def test_range_narrower_than_the_data_clamps(V):
    """The documented deviation: astype(np.uint8) is undefined outside [0, 256); kernel and oracle both clamp there."""
    d = O.depth_plane(37 * 53, seed=6).reshape(37, 53)
    for mi, ma in ((3.0, 5.0), (2.5, 8.0), (4.0, 4.0), (-1e30, 1e30)):
        got = V.visualize_depth(dev(d), mi, ma)
        assert torch.equal(got.cpu(), torch.from_numpy(O.visualize_depth(d, mi, ma))), (mi, ma)
    idx = O.depth_index(d, 3.0, 5.0)
    assert (idx[d < 3.0] == 0).all() and (idx[d > 5.0] == 255).all() and 0 < idx[(d > 3.1) & (d < 4.9)].min()


def test_small_spread_keeps_the_1e8(V):
    rng = np.random.default_rng(3)
    for spread in (0.09, 2.0 ** -10, 2.0 ** -20):
        d = (np.float32(1.0) + rng.uniform(0, spread, 37 * 53).astype(np.float32)).reshape(37, 53)
        d[0, 0], d[36, 52] = 1.0, np.float32(1.0 + spread)
        assert np.float32(d.max() - d.min()) + np.float32(1e-8) != np.float32(d.max() - d.min())      # not absorbed
        assert torch.equal(V.visualize_depth(dev(d)).cpu(), torch.from_numpy(O.visualize_depth(d)))


def test_strided_view_is_handled(V):
    """A (H, W) view with a non-unit stride is copied once and coloured as what it shows."""
    d = O.depth_plane(37 * 106, seed=8).reshape(37, 106)
    g = dev(d)
    view = g[:, ::2]
    assert view.stride() == (106, 2) and not view.is_contiguous()
    assert torch.equal(V.visualize_depth(view).cpu(), torch.from_numpy(O.visualize_depth(d[:, ::2])))
    t = g.t()
    assert torch.equal(V.visualize_depth(t).cpu(), torch.from_numpy(O.visualize_depth(np.ascontiguousarray(d.T))))
    assert torch.equal(V.visualize_depth(g.double()).cpu(), torch.from_numpy(O.visualize_depth(d)))
    with pytest.raises(RuntimeError, match=r"\(H, W\)"):
        V.visualize_depth(g.view(-1))


def test_custom_lut_is_honoured(V):
    rng = np.random.default_rng(11)
    lut = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    d, _ = plane_case((37, 53))
    want = torch.from_numpy(O.visualize_depth(d, lut=lut))
    assert torch.equal(V.visualize_depth(dev(d), cmap=torch.from_numpy(lut)).cpu(), want)            # host table: uploaded
    assert torch.equal(V.visualize_depth(dev(d), cmap=dev(lut)).cpu(), want)                         # device table: used in place
    assert not torch.equal(V.visualize_depth(dev(d)).cpu(), want)
    with pytest.raises(NotImplementedError):
        V.visualize_depth(dev(d), cmap=4)


# ---- frame sheets ----
def boundary_values():
    """rgb values on save_image's quantisation boundaries: k / 255 and its two fp32 neighbours, 0, 1, just outside [0, 1]."""
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    half = (np.arange(256, dtype=np.float32) + np.float32(0.5)) / np.float32(255)                    # v 255 + 0.5 near an integer
    edge = np.concatenate([k, np.nextafter(k, np.float32(2)), np.nextafter(k, np.float32(-1)),
                           half, np.nextafter(half, np.float32(2)), np.nextafter(half, np.float32(-1)),
                           np.array([0.0, -0.0, 1.0, -1e-3, 1.0 + 1e-3, -1e-8, 1.0 + 1e-7, -5.0, 7.0], dtype=np.float32)])
    return edge.astype(np.float32)


def rgb_rows(H, W, seed):
    rng = np.random.default_rng(seed)
    v = rng.uniform(-0.05, 1.05, H * W * 3).astype(np.float32)
    edge = boundary_values()
    take = edge if edge.size <= v.size else rng.choice(edge, v.size, replace=False)
    v[rng.choice(v.size, take.size, replace=False)] = take
    return v.reshape(H * W, 3)


@functools.lru_cache(maxsize=None)
def sheet_case(k, H, W):
    """(panels as numpy, oracle u8, oracle planar): rgb and depth panels mixed, every depth panel with data and a range of its own."""
    n = H * W
    depth = lambda seed, scale: (O.depth_plane(n, seed) * np.float32(scale)).astype(np.float32)
    nan_depth = depth(35, 1.0)
    nan_depth[n // 2] = np.nan
    pool = [rgb_rows(H, W, 21), rgb_rows(H, W, 22), depth(31, 1.0), rgb_rows(H, W, 23), (depth(32, 0.5), 1.5, 4.0),
            depth(33, 3.0).reshape(H, W), (nan_depth, 2.0, 10.0), depth(34, 0.01)]
    order = {1: [2], 2: [0, 2], 5: [0, 1, 2, 3, 5], 8: list(range(8))}[k]
    panels = tuple(pool[j] for j in order)
    u8, fl = O.sheet(list(panels), H, W)
    return panels, u8, fl


def to_dev(panels):
    return [(dev(p[0]), p[1], p[2]) if isinstance(p, tuple) else dev(p) for p in panels]


@pytest.mark.parametrize("H,W", [(3, 5), (37, 53)])
@pytest.mark.parametrize("k", [1, 2, 5, 8])
def test_frame_sheet(V, k, H, W):
    panels, u8, fl = sheet_case(k, H, W)
    sheet, stack = V.frame_sheet(to_dev(panels), H, W, planar=True)
    assert sheet.shape == (H, k * W, 3) and sheet.dtype == torch.uint8 and sheet.is_cuda
    assert stack.shape == (3, H, k * W) and stack.dtype == torch.float32
    assert torch.equal(sheet.cpu(), torch.from_numpy(u8))
    assert torch.equal(stack.cpu(), torch.from_numpy(fl))
    only = V.frame_sheet(to_dev(panels), H, W)
    assert isinstance(only, torch.Tensor) and torch.equal(only, sheet)


def test_frame_sheet_rgb_quantisation_boundaries(V):
    edge = boundary_values()
    n = -(-edge.size // 3)
    rows = np.zeros((n, 3), dtype=np.float32)
    rows.reshape(-1)[:edge.size] = edge
    sheet, stack = V.frame_sheet([dev(rows)], 1, n, planar=True)
    want = O.quantise(rows)
    assert torch.equal(sheet.cpu()[0], torch.from_numpy(want))
    assert torch.equal(stack.cpu()[:, 0, :].t(), torch.from_numpy(rows))      # the float stack carries the values as they are (-0.0 == 0.0)
    k255 = np.arange(256, dtype=np.float32) / np.float32(255)
    assert want.reshape(-1)[:256].tolist() == list(range(256))              # k / 255 -> k
    assert O.quantise(k255).tolist() == list(range(256))


def test_frame_sheet_panel_order_and_ranges(V):
    H, W = 37, 53
    panels, u8, _ = sheet_case(5, H, W)
    g = to_dev(panels)
    sheet = V.frame_sheet(g, H, W)
    back = V.frame_sheet(g[::-1], H, W)
    for j in range(5):
        assert torch.equal(back[:, j * W:(j + 1) * W], sheet[:, (4 - j) * W:(5 - j) * W]), j
    # each depth panel is normalised by its own range: alone or beside others, the same pixels
    for j in (2, 4):
        alone = V.frame_sheet([g[j]], H, W)
        assert torch.equal(alone, sheet[:, j * W:(j + 1) * W])
    # an explicit range equal to the data's is the data's
    d = panels[2]
    same = V.frame_sheet([(dev(d), float(d.min()), float(d.max()))], H, W)
    assert torch.equal(same, sheet[:, 2 * W:3 * W])
    # and equals visualize_depth on the plane
    pic = V.visualize_depth(dev(d).view(H, W))
    _, stack = V.frame_sheet([dev(d)], H, W, planar=True)
    assert torch.equal(stack, pic)


def test_frame_sheet_unaligned_outputs(V):
    """Outputs at odd addresses through the C ABI: the byte / scalar store paths, and nothing written outside the sheet."""
    import moco_flow_amd._lib as L
    lib = L.lib()
    H, W = 37, 53
    panels, u8, fl = sheet_case(2, H, W)
    g = to_dev(panels)
    n_out = H * W * 2
    items = (L.mf_sheet_panel * 2)()
    items[0].rows, items[0].kind = g[0].data_ptr(), 0
    items[1].rows, items[1].kind = g[1].data_ptr(), 1
    range2s = torch.zeros((2, 2), device="cuda")
    range2s[1, 0], range2s[1, 1] = float(panels[1].min()), float(panels[1].max())
    lut = dev(O.jet_lut())
    out_u8 = torch.full((3 * n_out + 8,), 77, dtype=torch.uint8, device="cuda")
    out_fl = torch.full((3 * n_out + 8,), -9.0, device="cuda")
    L.check(lib.mf_frame_sheet(items, 2, H, W, range2s.data_ptr(), lut.data_ptr(), out_u8.data_ptr() + 1, out_fl.data_ptr() + 4,
                               L.current_stream(out_u8.device)), "mf_frame_sheet")
    assert torch.equal(out_u8[1:1 + 3 * n_out].view(H, 2 * W, 3).cpu(), torch.from_numpy(u8))
    assert torch.equal(out_fl[1:1 + 3 * n_out].view(3, H, 2 * W).cpu(), torch.from_numpy(fl))
    assert out_u8[0] == 77 and (out_u8[1 + 3 * n_out:] == 77).all() and out_fl[0] == -9.0 and (out_fl[1 + 3 * n_out:] == -9.0).all()
    # one output at a time
    only_u8 = torch.empty((H, 2 * W, 3), dtype=torch.uint8, device="cuda")
    L.check(lib.mf_frame_sheet(items, 2, H, W, range2s.data_ptr(), lut.data_ptr(), only_u8.data_ptr(), None,
                               L.current_stream(out_u8.device)), "mf_frame_sheet")
    only_fl = torch.empty((3, H, 2 * W), device="cuda")
    L.check(lib.mf_frame_sheet(items, 2, H, W, range2s.data_ptr(), lut.data_ptr(), None, only_fl.data_ptr(),
                               L.current_stream(out_u8.device)), "mf_frame_sheet")
    assert torch.equal(only_u8.cpu(), torch.from_numpy(u8)) and torch.equal(only_fl.cpu(), torch.from_numpy(fl))


def test_frame_sheet_refusals_and_empty(V):
    rows = dev(rgb_rows(3, 5, 1))
    with pytest.raises(RuntimeError, match="9 panels"):
        V.frame_sheet([rows] * 9, 3, 5)
    with pytest.raises(RuntimeError, match="0 panels"):
        V.frame_sheet([], 3, 5)
    with pytest.raises(RuntimeError, match="panel 1 has shape"):
        V.frame_sheet([rows, rows[:14]], 3, 5)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        V.frame_sheet([rows, rows.cpu()], 3, 5)
    sheet, stack = V.frame_sheet([torch.zeros((0, 3), device="cuda"), torch.zeros((0,), device="cuda")], 0, 5, planar=True)
    assert sheet.shape == (0, 10, 3) and sheet.dtype == torch.uint8 and stack.shape == (3, 0, 10)
    sheet = V.frame_sheet([torch.zeros((0, 3), device="cuda")], 4, 0)
    assert sheet.shape == (4, 0, 3)
    assert V.visualize_depth(torch.zeros((0, 7), device="cuda")).shape == (3, 0, 7)
    assert raw_range(torch.zeros((0,), device="cuda")) == [0.0, 0.0]


@pytest.mark.parametrize("typ", ["fine", "coarse"])
def test_decode_results(V, typ):
    H, W = 37, 53
    rows, depth = rgb_rows(H, W, 41), O.depth_plane(H * W, 42)
    results = {"rgb_coarse": dev(rows), "depth_coarse": dev(depth), "opacity_coarse": torch.ones(H * W, device="cuda")}
    if typ == "fine":
        results["rgb_coarse"], results["depth_coarse"] = results["rgb_coarse"] * 0.5, results["depth_coarse"] + 1
        results.update({"rgb_fine": dev(rows), "depth_fine": dev(depth)})
    img_ori, img_pred, depth_ori, depth_pred = V.decode_results(results, (H, W))
    assert img_ori is results["rgb_" + typ] and depth_ori is results["depth_" + typ]
    assert img_pred.shape == (3, H, W) and img_pred.data_ptr() == img_ori.data_ptr()             # a view, as the reference's
    assert torch.equal(img_pred.cpu(), torch.from_numpy(rows).view(H, W, 3).permute(2, 0, 1))
    assert torch.equal(depth_pred.cpu(), torch.from_numpy(O.visualize_depth(depth.reshape(H, W))))


@pytest.mark.timeout(120)
def test_frame_sheet_graph_capture_and_replay(V):
    """One capture of frame_sheet (a range reduction per depth panel and the sheet launch: a single chain on one stream, no
    parallel branches) and one replay on new inputs give the bytes of a plain call on those inputs."""
    H, W = 37, 53
    panels, u8, fl = sheet_case(5, H, W)
    g = to_dev(panels)
    static = [(p[0].clone(), p[1], p[2]) if isinstance(p, tuple) else p.clone() for p in g]
    plain_sheet, plain_stack = V.frame_sheet(static, H, W, planar=True)      # warm-up: the table is on the device now
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sheet, stack = V.frame_sheet(static, H, W, planar=True)
    # new content in the captured inputs: the panels in another order of the same kinds
    static[0].copy_(g[1]); static[1].copy_(g[3]); static[3].copy_(g[0])
    static[2].copy_(g[4].view(-1)); static[4].copy_(g[2].view(H, W))
    graph.replay()
    torch.cuda.synchronize()
    want_u8, want_fl = O.sheet([panels[1], panels[3], panels[4].reshape(-1), panels[0], panels[2].reshape(H, W)], H, W)
    assert torch.equal(sheet.cpu(), torch.from_numpy(want_u8))
    assert torch.equal(stack.cpu(), torch.from_numpy(want_fl))
    assert torch.equal(plain_sheet.cpu(), torch.from_numpy(u8)) and torch.equal(plain_stack.cpu(), torch.from_numpy(fl))
