"""CPU-side checks (-m "not gpu") of matte clean-up (moco_flow_amd/frames.py: clean_mask, mask_regions; csrc/mf_regions.hip,
csrc/mf_unionfind.hpp): the numpy oracle the GPU tests compare with (tests/regions_oracle.py) on hand-written masks with the
answers written out; the kernels' decomposition (components per tile, then the seam rule) against the plain components, on random
masks and on the seam cases, with every seam union and with the thinned set the seam kernel makes, before anything runs on a GPU; scipy.ndimage where it imports; the header, the prototypes and the
exports; every refusal the six entries make before any launch; the Python layer's argument checks.  None of it touches a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import regions_oracle as RO

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "moco_flow_amd", "csrc")
NEW_SYMBOLS = ("mf_mask_label_scratch_bytes", "mf_mask_label", "mf_mask_select", "mf_mask_fill_holes", "mf_mask_table_count",
               "mf_mask_table_emit")


def grid(*rows):
    return np.array([[c == "#" for c in r] for r in rows])


RING = grid(".......",
            ".#####.",
            ".#...#.",
            ".#...#.",
            ".#####.",
            ".......")
RING_ISLAND = grid(".......",
                   ".#####.",
                   ".#...#.",
                   ".#.#.#.",
                   ".#...#.",
                   ".#####.",
                   ".......")
BAY = grid("..#.#..",
           "..#.#..",
           "..###..",
           ".......")
LEAK = grid(".......",          # the pocket at (2, 2) reaches the outside only through the diagonal gap between (2, 3) and (3, 2)
            ".###...",
            ".#.#...",
            ".##....",
            ".......")
TIE = grid("##..##",
           "......",
           "#..###")


def test_oracle_on_hand_written_masks():
    lab = RO.components(RING, 8)
    assert set(np.unique(lab)) == {-1, 8} and (lab == 8).sum() == 14           # first member: (1, 1) = 1 * 7 + 1
    filled = RO.fill_holes(RING.astype(np.uint8) * 255)
    assert filled.sum() // 255 == 14 + 6 and (filled[2:4, 2:5] == 255).all() and filled[0].sum() == 0

    lab = RO.components(RING_ISLAND, 8)
    assert sorted(np.unique(lab)) == [-1, 8, 24] and (lab == 24).sum() == 1    # the island at (3, 3)
    alpha = np.where(RING_ISLAND, 255, 0).astype(np.uint8)[None]
    kept = RO.clean_mask(alpha, largest=True)[0]
    assert kept[3, 3] == 0 and kept.sum() // 255 == 16
    whole = RO.clean_mask(alpha, largest=True, fill=True)[0]                   # island removed, then the hole fills whole
    assert (whole[1:6, 1:6] == 255).all() and whole.sum() // 255 == 25
    both = RO.clean_mask(alpha, largest=False, fill=True)[0]
    assert np.array_equal(both, whole)                                         # kept, the island lies inside the filled hole
    assert RO.clean_mask(alpha, largest=False, min_area=2)[0][3, 3] == 0

    assert np.array_equal(RO.fill_holes(BAY.astype(np.uint8) * 255), BAY.astype(np.uint8) * 255)     # a bay on the border

    m = LEAK.astype(np.uint8) * 255
    f = RO.fill_holes(m)
    assert f[2, 2] == 255 and (f != m).sum() == 1                              # the zeros' 4-connectivity keeps the pocket closed
    pocket = RO.components(~LEAK, 4)
    assert pocket[2, 2] == 2 * 7 + 2 and (pocket == 16).sum() == 1 and pocket[3, 3] == 0
    assert set(np.unique(RO.components(~LEAK, 8))) == {-1, 0}                  # under 8 the pocket would leak: not the rule
    assert len(np.unique(RO.components(LEAK, 8))) == 2 and len(np.unique(RO.components(LEAK, 4))) == 2

    lab = RO.components(TIE, 8)
    counts, rows = RO.table(lab[None])
    assert counts.tolist() == [4]
    assert rows.tolist() == [[0, 0, 2, 0, 0, 1, 0], [0, 4, 2, 4, 0, 5, 0], [0, 12, 1, 0, 2, 0, 2], [0, 15, 3, 3, 2, 5, 2]]
    assert np.array_equal(RO.select(lab), grid("......", "......", "...###").astype(np.uint8) * 255)
    two = grid("##..##", "......", "#...##")                                    # three regions of two: the first wins
    assert np.array_equal(RO.select(RO.components(two, 8)), grid("##....", "......", "......").astype(np.uint8) * 255)
    assert RO.select(np.full((3, 4), -1)).sum() == 0                           # no members: zeros
    # thresholds
    a = np.array([[195, 196, 197]], dtype=np.uint8)
    assert RO.members(a).tolist() == [[False, True, True]] and RO.members(a, below=True).tolist() == [[True, False, False]]
    assert RO.members(a, 0).all() and not RO.members(a, 256).any()
    # diagonal neighbours join under 8 only; rows do not wrap
    d = grid("#.", ".#")
    assert RO.components(d, 8).tolist() == [[0, -1], [-1, 0]] and RO.components(d, 4).tolist() == [[0, -1], [-1, 3]]
    w = grid("..#", "#..")
    assert RO.components(w, 8).tolist() == [[-1, -1, 2], [3, -1, -1]]


@pytest.mark.parametrize("conn", (8, 4))
def test_tiled_decomposition_equals_the_components(conn):
    rng = np.random.default_rng(3)
    H, W = 23, 37
    for density in (0.30, 0.42, 0.50, 0.62):
        m = rng.random((H, W)) < density
        want = RO.components(m, conn)
        for th, tw in ((1, 1), (4, 8), (5, 3), (16, 64), (23, 1), (1, 37)):
            assert np.array_equal(RO.components_tiled(m, conn, th, tw), want), (density, th, tw)
            assert np.array_equal(RO.components_tiled(m, conn, th, tw, thinned=True), want), (density, th, tw, "thinned")
    th, tw = 4, 8
    H, W = 3 * th + 5, 2 * tw + 3
    for name, a, b, joined4 in RO.seam_pairs(th, tw):
        m = np.zeros((H, W), dtype=bool)
        m[a] = m[b] = True
        lab = RO.components_tiled(m, conn, th, tw)
        assert np.array_equal(lab, RO.components(m, conn)), name
        assert np.array_equal(RO.components_tiled(m, conn, th, tw, thinned=True), lab), name
        assert (lab[a] == lab[b]) == (conn == 8 or joined4), name
    for make in (RO.serpentine, RO.comb, RO.nested_us, RO.spirals):
        m = make(H, W)
        assert np.array_equal(RO.components_tiled(m, conn, th, tw), RO.components(m, conn)), make.__name__
        assert np.array_equal(RO.components_tiled(m, conn, th, tw, thinned=True), RO.components(m, conn)), make.__name__
    lab = RO.components(RO.serpentine(H, W), conn)
    assert set(np.unique(lab)) == {-1, 0} and (lab == 0).sum() == RO.serpentine_area(H, W)
    assert set(np.unique(RO.components(RO.comb(H, W), conn))) == {-1, 0}
    us = RO.components(RO.nested_us(H, W), conn)
    assert sorted(np.unique(us))[1:] == list(range(0, 2 * (len(np.unique(us)) - 1), 2))
    assert len(np.unique(RO.components(RO.spirals(H, W), conn))) == 3


def test_oracle_equals_scipy_ndimage():
    nd = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(9)
    for conn, structure in ((4, None), (8, np.ones((3, 3)))):
        for density in (0.30, 0.42, 0.50, 0.62):
            m = rng.random((61, 83)) < density
            lab, n = nd.label(m, structure=structure)
            first = nd.minimum(np.arange(m.size).reshape(m.shape), lab, index=np.arange(1, n + 1)).astype(np.int64)
            want = np.where(m, np.concatenate([[-1], first])[lab], -1)
            got = RO.components(m, conn)
            assert np.array_equal(got, want), (conn, density)
            counts, rows = RO.table(got[None])
            assert counts[0] == n and np.array_equal(rows[:, 2], np.bincount(lab.ravel())[1:][np.argsort(first)])
        m = rng.random((40, 50)) < 0.55
        assert np.array_equal(RO.fill_holes(m), nd.binary_fill_holes(m).astype(np.uint8) * 255)


def test_header_library_and_package():
    import moco_flow_amd as M
    import moco_flow_amd._lib as L
    header = open(os.path.join(ROOT, "include", "mocoflow_hip.h")).read()
    declared = set(re.findall(r"^int(?:32|64)_t (mf_\w+)\(", header, re.M))
    lib = L.lib()
    assert lib.mf_version() == 16 and L.MF_ABI_VERSION == 16 and "#define MF_ABI_VERSION 16" in header
    listed = " ".join(header.split("additive entries since")[1].split("*/")[0].split())
    for name in NEW_SYMBOLS:
        assert name in declared and name in L.SYMBOLS and name in listed, name
        fn = getattr(lib, name)
        assert fn.restype is L.SYMBOLS[name][0] and list(fn.argtypes) == L.SYMBOLS[name][1]
        comment = header.split(name + "(")[0].rsplit("/*", 1)[1]
        assert "scripts/data_utils.py:102-114" in comment and ":135-147" in comment, name
    i64, i32, p = C.c_int64, C.c_int32, C.c_void_p
    assert L.SYMBOLS["mf_mask_label_scratch_bytes"] == (i64, [i64, i64, i64])
    assert L.SYMBOLS["mf_mask_label"] == (i32, [p, i32, i64, i64, i64, i32, i32, i32, p, p, p])
    assert L.SYMBOLS["mf_mask_select"] == (i32, [p, i64, i64, i64, i32, i64, p, p, p])
    assert L.SYMBOLS["mf_mask_fill_holes"] == (i32, [p, i64, i64, i64, p, p])
    assert L.SYMBOLS["mf_mask_table_count"] == (i32, [p, i64, i64, i64, p, p])
    assert L.SYMBOLS["mf_mask_table_emit"] == (i32, [p, i64, i64, i64, i64, i64, p, p, p])
    make = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS = (.*)$", make, re.M).group(1).split()
    hdrs = re.search(r"^HDRS = (.*)$", make, re.M).group(1).split()
    assert "mf_regions.hip" in srcs and "mf_unionfind.hpp" in hdrs
    # the union-find lives in one header that both units include
    mesh = open(os.path.join(CSRC, "mf_mesh_components.hip")).read()
    unit = open(os.path.join(CSRC, "mf_regions.hip")).read()
    shared = open(os.path.join(CSRC, "mf_unionfind.hpp")).read()
    for src in (mesh, unit):
        assert '#include "mf_unionfind.hpp"' in src
        for name in ("int find_root(", "void unite(", "struct WaveCount", "void wave_count(", "void wave_count_flush("):
            assert name not in src and name in shared, name
    for name in ("kThreads", "kMaxBlocks", "kUnionBlocks"):
        assert re.search(rf"constexpr int {name} = \d+;", mesh), name
    for name in ("kRegTileH", "kRegTileW", "kRegThreads", "kRegMaxBlocks"):
        assert re.search(rf"constexpr int {name} = \d+;", unit), name
    assert int(re.search(r"constexpr int kRegTileW = (\d+);", unit).group(1)) == 64
    for name in ("clean_mask", "mask_regions", "Regions"):
        assert name in M.__all__ and name in M.frames.__all__ and getattr(M, name) is getattr(M.frames, name)
    assert M.Regions._fields == ("labels", "counts", "table")
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert "clean_mask" in open(os.path.join(ROOT, doc)).read(), doc


def test_entries_refuse_before_any_launch():
    import moco_flow_amd._lib as L
    lib = L.lib()
    fake, odd = C.c_void_p(256), C.c_void_p(258)
    err = lambda: lib.mf_last_error()
    label = lambda F, H, W, **kw: lib.mf_mask_label(kw.get("alpha", fake), kw.get("stride", 1), F, H, W, kw.get("thres", 196),
                                                    kw.get("below", 0), kw.get("conn", 8), kw.get("labels", fake), kw.get("scratch", fake), None)
    select = lambda F, H, W, **kw: lib.mf_mask_select(kw.get("labels", fake), F, H, W, 1, kw.get("min_area", 0), kw.get("out", fake),
                                                      kw.get("scratch", fake), None)
    fill = lambda F, H, W, **kw: lib.mf_mask_fill_holes(kw.get("mask", fake), F, H, W, kw.get("scratch", fake), None)
    count = lambda F, H, W, **kw: lib.mf_mask_table_count(kw.get("labels", fake), F, H, W, kw.get("counts", fake), None)
    emit = lambda F, H, W, **kw: lib.mf_mask_table_emit(kw.get("labels", fake), F, H, W, kw.get("frame0", 0), kw.get("C", 1), kw.get("table", fake),
                                                        kw.get("scratch", fake), None)
    sbytes = lambda F, H, W: lib.mf_mask_label_scratch_bytes(F, H, W)
    entries = (label, select, fill, count, emit, sbytes)
    # sizes < 0 and F H W >= 2^31, every entry
    for shape in ((-1, 4, 4), (1, -4, 4), (1, 4, -4), (1 << 11, 1 << 10, 1 << 10), (1, 1 << 16, 1 << 15), (3, 1 << 15, 1 << 15),
                  (1 << 62, 1 << 62, 1 << 62), (1 << 40, 0, 4)):
        for fn in entries:
            assert fn(*shape) == -1 and b"2^31" in err(), shape
    assert sbytes(1 << 10, 1 << 10, (1 << 11) - 1) > 0                          # just below the bound
    n = 3 * 5 * 7
    assert sbytes(3, 5, 7) >= 8 * n + 8 * 3 and sbytes(3, 5, 7) % 16 == 0 and sbytes(0, 5, 7) >= 0
    assert sbytes(2, 5, 7) <= sbytes(3, 5, 7)                                   # a shorter last chunk fits the first one's scratch
    for thres in (-1, 257, 1000):
        assert label(1, 4, 4, thres=thres) == -1 and b"thres" in err()
    assert label(0, 4, 4, thres=-1) == -1                                       # refused even where nothing would be launched
    for conn in (0, 6, 9, -8):
        assert label(1, 4, 4, conn=conn) == -1 and b"connectivity" in err()
    for stride in (0, 2, 3, 5, -1):
        assert label(1, 4, 4, stride=stride) == -1 and b"stride" in err()
    for kw in (dict(alpha=None), dict(labels=None), dict(scratch=None)):
        assert label(1, 4, 4, **kw) == -1 and b"null" in err()
    assert label(1, 4, 4, labels=odd) == -1 and b"aligned" in err() and label(1, 4, 4, scratch=odd) == -1
    for kw in (dict(labels=None), dict(out=None), dict(scratch=None)):
        assert select(1, 4, 4, **kw) == -1 and b"null" in err()
    assert select(1, 4, 4, labels=odd) == -1 and b"aligned" in err()
    for kw in (dict(mask=None), dict(scratch=None)):
        assert fill(1, 4, 4, **kw) == -1 and b"null" in err()
    assert fill(1, 4, 4, scratch=odd) == -1 and b"aligned" in err()
    assert fill(3, 2, 9) == 0 and fill(3, 9, 1) == 0                            # no interior: nothing is launched
    assert count(1, 4, 4, labels=None) == -1 and count(1, 4, 4, counts=None) == -1 and b"null" in err()
    assert count(1, 4, 4, labels=odd) == -1 and b"aligned" in err()
    for kw in (dict(labels=None), dict(table=None), dict(scratch=None)):
        assert emit(1, 4, 4, **kw) == -1 and b"null" in err()
    assert emit(1, 4, 4, C=-1) == -1 and emit(1, 4, 4, C=17) == -1 and b"C=" in err()
    assert emit(1, 4, 4, frame0=-1) == -1 and emit(2, 4, 4, frame0=(1 << 31) - 2) == -1 and b"frame0" in err()
    assert emit(1, 4, 4, frame0=(1 << 63) - 1) == -1 and b"frame0" in err() and emit(1, 4, 4, frame0=(1 << 31) - 2, labels=None) == -1
    assert emit(1, 4, 4, table=odd) == -1 and b"aligned" in err()
    # no pixels or no rows: nothing is launched, whatever else is null
    for fn in (label, select, fill):
        assert fn(0, 4, 4, alpha=None, labels=None, out=None, mask=None, scratch=None) == 0
        assert fn(2, 0, 4, alpha=None, labels=None, out=None, mask=None, scratch=None) == 0
    assert count(0, 4, 4, labels=None, counts=None) == 0
    assert emit(1, 4, 4, C=0, labels=None, table=None, scratch=None) == 0 and emit(0, 4, 4, C=0, labels=None) == 0


def test_python_layer_refuses_before_any_launch():
    from moco_flow_amd import frames
    a = torch.zeros((2, 5, 6), dtype=torch.uint8)
    for fn in (frames.clean_mask, frames.mask_regions):
        with pytest.raises(RuntimeError, match="no CPU"):
            fn(a)
        with pytest.raises(RuntimeError, match="no CPU"):
            fn(torch.zeros((5, 6, 4), dtype=torch.uint8))
        with pytest.raises(RuntimeError, match="uint8"):
            fn(a.float())
        with pytest.raises(RuntimeError, match="uint8"):
            fn(a.numpy())
    assert frames.SCRATCH_BUDGET > 0
    assert frames._region_chunk(300, 1080, 1080) == frames.SCRATCH_BUDGET // (12 * 1080 * 1080) and frames._region_chunk(3, 5, 6) == 3
    assert frames._region_chunk(10, 1 << 15, 1 << 15) == 1 and frames._region_chunk(5, 0, 7) == 5
    for thres in (257, -1, 196.5, True, None):
        with pytest.raises(RuntimeError, match="thres"):
            frames.clean_mask(a, thres=thres)
        with pytest.raises(RuntimeError, match="thres"):
            frames.mask_regions(a, thres)
    for conn in (6, 0, "8"):
        with pytest.raises(RuntimeError, match="connectivity"):
            frames.mask_regions(a, connectivity=conn)
    for min_area in (-1, 2.5):
        with pytest.raises(RuntimeError, match="min_area"):
            frames.clean_mask(a, min_area=min_area)
    frames._region_args("clean_mask", 0, 4, 0)
    frames._region_args("clean_mask", np.int64(256), 8, 50)
