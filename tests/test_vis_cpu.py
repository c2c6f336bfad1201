"""moco_flow_amd.vis without a GPU: the Jet table against its closed form, the package's exports and ctypes prototypes, the
host-side argument validation of mf_depth_range / mf_depth_colormap / mf_frame_sheet (include/mocoflow_hip.h), the numpy
restatement (tests/vis_oracle.py) on hand-computed values, and the PNG writer read back chunk by chunk."""
import ctypes
import struct
import zlib

import numpy as np
import pytest
import torch

import vis_oracle as O


@pytest.fixture(scope="module")
def V():
    import moco_flow_amd
    return moco_flow_amd.vis


@pytest.fixture(scope="module")
def lut(V):
    return V.colormap_lut().numpy()


def test_lut_anchors_as_rgb(V, lut):
    assert lut.shape == (256, 3) and lut.dtype == np.uint8
    rgb = lambda i: (int(lut[i, 2]), int(lut[i, 1]), int(lut[i, 0]))        # column 2 is the r curve, column 0 the b curve
    assert rgb(0) == (0, 0, 128)                                            # b = 0.5 -> 127.5 -> 128 (ties to even)
    assert rgb(255) == (128, 0, 0)
    # i = 96: r = 4 * 96 / 255 - 1.5 = 0.00588..., times 255 = 1.5 in exact arithmetic; what float64 and ties-to-even give
    r96 = min(4 * (96 / 255) - 1.5, 4.5 - 4 * (96 / 255)) * 255
    assert rgb(96)[0] == int(np.rint(r96)) and rgb(96)[0] in (1, 2)
    assert rgb(96)[1] == 255
    assert rgb(128)[1] == 255
    assert V.colormap_lut() is V.colormap_lut(V.COLORMAP_JET)               # built once
    assert V.COLORMAP_JET == 2


def test_lut_equals_the_float64_closed_form(lut):
    for i in range(256):
        x = i / 255
        curve = lambda up, down: min(max(min(4 * x + up, down - 4 * x), 0.0), 1.0)
        want = [int(np.rint(255 * curve(0.5, 2.5))), int(np.rint(255 * curve(-0.5, 3.5))), int(np.rint(255 * curve(-1.5, 4.5)))]
        assert lut[i].tolist() == want, i
    assert np.array_equal(lut, O.jet_lut())


def test_lut_monotone_segments_and_channel_order(lut):
    b, g, r = (lut[:, c].astype(int) for c in range(3))
    # column 0 is the b curve: it starts at half, rises to full, is zero over the top of the range
    assert b[0] == 128 and b[32] == 255 and (b[160:] == 0).all()
    assert r[255] == 128 and r[223] == 255 and (r[:96] == 0).all()
    up, down = lambda a: (np.diff(a) >= 0).all(), lambda a: (np.diff(a) <= 0).all()
    assert up(b[:33]) and (b[32:96] == 255).all() and down(b[95:])
    assert up(g[:97]) and (g[96:160] == 255).all() and down(g[159:]) and g[0] == 0 and g[255] == 0
    assert up(r[:224]) and down(r[223:])
    assert lut.min() >= 0 and lut.max() <= 255 and lut.max() == 255


def test_bad_cmap_raises(V):
    for bad in (0, 1, 3, 20, -1):
        with pytest.raises(NotImplementedError, match="colour map"):
            V.colormap_lut(bad)
    with pytest.raises(NotImplementedError):
        V.colormap_lut("jet")
    with pytest.raises(RuntimeError, match=r"\(256, 3\) uint8"):
        V.colormap_lut(torch.zeros(256, 3))
    with pytest.raises(RuntimeError, match=r"\(256, 3\) uint8"):
        V.colormap_lut(torch.zeros(255, 3, dtype=torch.uint8))
    own = torch.arange(768, dtype=torch.int64).remainder(256).to(torch.uint8).view(256, 3)
    assert V.colormap_lut(own) is own


def test_package_exports_vis():
    import moco_flow_amd
    import moco_flow_amd._lib as L
    assert hasattr(moco_flow_amd, "vis")
    names = {"COLORMAP_JET", "colormap_lut", "visualize_depth", "decode_results", "frame_sheet", "write_png"}
    assert set(moco_flow_amd.vis.__all__) == names
    for n in ("vis", "visualize_depth", "decode_results", "frame_sheet", "write_png"):
        assert n in moco_flow_amd.__all__ and hasattr(moco_flow_amd, n)
    lib = L.lib()
    for sym in ("mf_depth_range_scratch_bytes", "mf_depth_range", "mf_depth_colormap", "mf_frame_sheet"):
        assert sym in L.SYMBOLS and hasattr(lib, sym)
    assert ctypes.sizeof(L.mf_sheet_panel) == 16
    assert lib.mf_version() == 16


def test_cpu_tensors_raise(V):
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        V.visualize_depth(torch.rand(4, 5))
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        V.frame_sheet([torch.rand(20, 3)], 4, 5)
    with pytest.raises(RuntimeError, match="from 1 to 8"):
        V.frame_sheet([], 4, 5)


def test_depth_range_abi_validates_on_the_host():
    import moco_flow_amd._lib as L
    lib = L.lib()
    buf = (ctypes.c_float * 8)()
    p = ctypes.addressof(buf)
    assert lib.mf_depth_range_scratch_bytes(0) == 0
    assert lib.mf_depth_range_scratch_bytes(1) == 8                         # one workgroup: (min, max) fp32
    assert lib.mf_depth_range_scratch_bytes(540 * 540) > 8
    cap = lib.mf_depth_range_scratch_bytes(1 << 40)                         # the grid stops growing
    assert cap == lib.mf_depth_range_scratch_bytes(1 << 41) and cap % 8 == 0
    assert lib.mf_depth_range_scratch_bytes(-1) == -1
    assert b"negative" in lib.mf_last_error()
    assert lib.mf_depth_range(p, -4, 0.0, p, p, None) == -1
    assert b"negative" in lib.mf_last_error()
    assert lib.mf_depth_range(p, 4, 0.0, None, p, None) == -1
    assert b"out2" in lib.mf_last_error()
    assert lib.mf_depth_range(None, 4, 0.0, p, p, None) == -1
    assert b"null" in lib.mf_last_error()
    assert lib.mf_depth_range(p, 4, 0.0, p, None, None) == -1
    assert lib.mf_depth_colormap(p, -1, p, 0.0, p, p, None) == -1
    assert b"negative" in lib.mf_last_error()
    for missing in range(4):
        args = [p, p, p, p]
        args[missing] = None
        assert lib.mf_depth_colormap(args[0], 8, args[1], 0.0, args[2], args[3], None) == -1
        assert b"null" in lib.mf_last_error()
    assert lib.mf_depth_colormap(None, 0, None, 0.0, None, None, None) == 0  # n = 0: nothing to do


def test_frame_sheet_abi_validates_on_the_host():
    import moco_flow_amd._lib as L
    lib = L.lib()
    buf = (ctypes.c_float * 8)()
    p = ctypes.addressof(buf)

    def call(n_panels, H, W, kinds=None, rows=True, range2s=p, lut=p, out_u8=p, out_planar=p, n_items=None):
        items = (L.mf_sheet_panel * max(n_items or n_panels, 1))()
        for k in range(len(items)):
            items[k].rows = p if rows else None
            items[k].kind = (kinds or [0] * len(items))[k]
        return lib.mf_frame_sheet(items, n_panels, H, W, range2s, lut, out_u8, out_planar, None)

    assert call(9, 4, 4) == -1
    assert b"n_panels=9" in lib.mf_last_error()
    assert call(0, 4, 4) == -1 and b"n_panels" in lib.mf_last_error()
    assert call(-1, 4, 4, n_items=1) == -1
    assert call(2, -4, 4) == -1 and b"negative" in lib.mf_last_error()
    assert call(2, 4, 4, out_u8=None, out_planar=None) == -1
    assert b"both null" in lib.mf_last_error()
    assert lib.mf_frame_sheet(None, 2, 4, 4, p, p, p, p, None) == -1
    assert b"panels is null" in lib.mf_last_error()
    # 32-bit indexing: H W n_panels 3 < 2^31
    assert call(1, 1 << 15, 21846) == -1                                    # 3 * 2^15 * 21846 = 2^31 + 2^16
    assert b"2^31" in lib.mf_last_error()
    assert call(8, 9460, 9460) == -1 and b"2^31" in lib.mf_last_error()     # 24 * 9460^2 = 2.1478e9
    assert call(2, 1 << 40, 1 << 40) == -1 and b"2^31" in lib.mf_last_error()
    assert call(2, 4, 4, kinds=[0, 2]) == -1 and b"kind=2" in lib.mf_last_error()
    assert call(2, 4, 4, kinds=[0, 1], lut=None) == -1 and b"depth panel" in lib.mf_last_error()
    assert call(2, 4, 4, kinds=[1, 0], range2s=None) == -1 and b"depth panel" in lib.mf_last_error()
    assert call(2, 4, 4, rows=False) == -1 and b"null rows" in lib.mf_last_error()
    assert call(3, 0, 7) == 0 and call(3, 7, 0) == 0                        # H W = 0: nothing is launched


def test_oracle_on_hand_computed_values():
    lut = O.jet_lut()
    # min 2, max 6: den = 4 + 1e-8 = 4 in fp32; 3 -> 255 * 0.25 = 63.75 -> 63; 6 -> 255; nan -> 0 -> below the min? no: nan_to_num
    # comes first, so 0 IS the min: (0, 2, 3, 6) / 6 -> 0, 85, 127 (127.5 truncated), 255
    assert O.depth_index(np.array([[2.0, 3.0, 6.0]], dtype=np.float32)).tolist() == [[0, 63, 255]]
    assert O.depth_index(np.array([[np.nan, 2.0, 3.0, 6.0]], dtype=np.float32)).tolist() == [[0, 85, 127, 255]]
    # given range: nan -> ma; outside the range: the documented clamp
    assert O.depth_index(np.array([[np.nan, 1.0, 2.0, 4.0, 7.0]], dtype=np.float32), 2.0, 6.0).tolist() == [[255, 0, 0, 127, 255]]
    # constant plane: 0 / 1e-8
    assert O.depth_index(np.full((2, 3), 3.5, dtype=np.float32)).tolist() == [[0] * 3] * 2
    # infinities: +-FLT_MAX, the range overflows to inf; (FLT_MAX + FLT_MAX) / inf is NaN -> 0
    assert O.depth_index(np.array([[-np.inf, 3.0, np.inf]], dtype=np.float32)).tolist() == [[0, 0, 0]]
    assert O.depth_index(np.array([[2.0, 3.0, np.inf]], dtype=np.float32)).tolist() == [[0, 0, 255]]
    # a spread of 2^-20 around 1: 1e-8 is NOT absorbed by the denominator (its ulp is 2^-43), the top index is 252
    d = np.array([[1.0, 1.0 + 2.0 ** -21, 1.0 + 2.0 ** -20]], dtype=np.float32)
    assert O.depth_index(d).tolist() == [[0, 126, 252]]
    pic = O.visualize_depth(np.array([[2.0, 6.0]], dtype=np.float32))
    assert pic.shape == (3, 1, 2) and pic.dtype == np.float32
    assert pic[:, 0, 0].tolist() == [np.float32(128) / np.float32(255), 0.0, 0.0]            # channel 0 is the b curve
    assert pic[:, 0, 1].tolist() == [0.0, 0.0, np.float32(128) / np.float32(255)]
    # save_image's quantisation: k / 255 lands on k + 0.5 -> k; just below 0 and above 1 clamp
    assert O.quantise(np.array([0.0, 1.0, -0.1, 1.2, 0.5, np.nan], dtype=np.float32)).tolist() == [0, 255, 0, 255, 128, 0]
    u8, fl = O.sheet([np.array([[0.0, 0.5, 1.0]] * 2, dtype=np.float32), np.array([2.0, 6.0], dtype=np.float32)], 1, 2)
    assert u8.shape == (1, 4, 3) and fl.shape == (3, 1, 4)
    assert u8[0].tolist() == [[0, 128, 255], [0, 128, 255], lut[0].tolist(), lut[255].tolist()]
    assert fl[:, 0, 0].tolist() == [0.0, 0.5, 1.0]


def _read_png(path):
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        (length,) = struct.unpack(">I", data[pos:pos + 4])
        tag, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + length]
        (crc,) = struct.unpack(">I", data[pos + 8 + length:pos + 12 + length])
        assert crc == zlib.crc32(tag + body) & 0xffffffff, tag
        chunks.append((tag, body))
        pos += 12 + length
    assert pos == len(data)
    return chunks


@pytest.mark.parametrize("H,W", [(5, 7), (1, 1)])
def test_write_png_round_trip(V, tmp_path, H, W):
    gen = torch.Generator().manual_seed(H * 10 + W)
    sheet = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=gen)
    path = tmp_path / "sheet.png"
    V.write_png(str(path), sheet)
    chunks = _read_png(path)
    assert [t for t, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    assert struct.unpack(">IIBBBBB", chunks[0][1]) == (W, H, 8, 2, 0, 0, 0)   # 8-bit, colour type 2 (RGB), no interlace
    raw = zlib.decompress(chunks[1][1])
    assert len(raw) == H * (1 + 3 * W)
    rows = np.frombuffer(raw, dtype=np.uint8).reshape(H, 1 + 3 * W)
    assert (rows[:, 0] == 0).all()                                          # filter 0 on every row
    assert np.array_equal(rows[:, 1:].reshape(H, W, 3), sheet.numpy())
    assert chunks[2][1] == b""
    # a non-contiguous view is written as what it shows
    V.write_png(str(path), sheet.flip(1))
    raw = zlib.decompress(_read_png(path)[1][1])
    assert np.array_equal(np.frombuffer(raw, dtype=np.uint8).reshape(H, 1 + 3 * W)[:, 1:].reshape(H, W, 3), sheet.flip(1).numpy())


def test_write_png_refuses_other_shapes(V, tmp_path):
    for bad in (torch.zeros(4, 5, 3), torch.zeros(4, 5, dtype=torch.uint8), torch.zeros(4, 5, 4, dtype=torch.uint8),
                torch.zeros(0, 5, 3, dtype=torch.uint8)):
        with pytest.raises(RuntimeError, match="write_png"):
            V.write_png(str(tmp_path / "x.png"), bad)
