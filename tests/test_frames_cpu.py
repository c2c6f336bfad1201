"""CPU-side checks (-m "not gpu") of frame ingest (moco_flow_amd/frames.py, csrc/mf_frames.hip): the numpy oracle the GPU tests
compare with (tests/frames_oracle.py) against PIL's recorded outputs (tests/golden/u_frames.npz, written by
tests/golden/gen_frames.py) and, where PIL imports, against live PIL over a sweep of sizes; the integer plate against the
reference's float64 expression; the host coefficient tables; the refusals every entry makes before any launch; the library's
exports and prototypes.  None of it touches a GPU."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import frames_oracle as FO

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW_SYMBOLS = ("mf_resize_u8_scratch_bytes", "mf_resize_u8", "mf_composite_rows", "mf_background_plate")
ALPHAS = np.array([0, 1, 3, 128, 254, 255], dtype=np.uint8)
# (H0, W0) -> (H, W): 1080 -> 540 and 540 -> 512 (the shipped configurations), 37 -> 16, 23 -> 40, 300 -> 7 (87 taps), 1 -> 5,
# 5 -> 1, one axis only, the identity
SWEEP = (((1080, 540), (540, 512)), ((37, 23), (16, 40)), ((300, 5), (7, 1)), ((1, 5), (5, 1)), ((5, 1), (1, 5)),
         ((20, 33), (20, 16)), ((33, 20), (16, 20)), ((9, 7), (9, 7)))


@pytest.fixture(scope="module")
def golden():
    d = np.load(os.path.join(HERE, "golden", "u_frames.npz"))
    return d, json.loads(str(d["cases"]))


def _image(rng, H, W, C):
    a = rng.integers(0, 256, size=(H, W, C), dtype=np.uint8)
    if C == 4:
        a[..., 3] = rng.choice(ALPHAS, size=(H, W))
    return a


def test_oracle_equals_the_recorded_pil_outputs(golden):
    d, cases = golden
    assert len(cases["resize"]) >= 20 and cases["pil"].split(".")[0] == "12"
    for name, (src, H, W) in cases["resize"].items():
        a = d["in_" + src]
        want = d["resize_" + name]
        assert want.shape == (a.shape[0], H, W, a.shape[3]), name
        assert np.array_equal(FO.resize(a, (H, W)), want), name
    assert os.path.getsize(os.path.join(HERE, "golden", "u_frames.npz")) < 256 * 1024


def test_oracle_equals_live_pil_over_the_sweep():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(5)
    for (H0, W0), (H, W) in SWEEP:
        for Cn in (1, 3, 4):
            a = _image(rng, H0, W0, Cn)
            want = np.asarray(Image.fromarray(a[..., 0] if Cn == 1 else a).resize((W, H), Image.BILINEAR)).reshape(H, W, Cn)
            assert np.array_equal(FO.resize(a, (H, W)), want), ((H0, W0), (H, W), Cn)


def test_identity_returns_the_input_bytes(golden):
    """No premultiply round trip: c = 200 under alpha = 3 would come back as 170."""
    d, _ = golden
    a = d["in_a4"]
    assert np.array_equal(FO.resize(a, a.shape[1:3]), a) and np.array_equal(d["resize_identity_rgba"], a)
    px = np.array([[[200, 100, 7, 3]]], dtype=np.uint8)
    assert np.array_equal(FO.resize(px, (1, 1)), px)
    assert not np.array_equal(FO.resize(np.repeat(px, 2, axis=1), (1, 1)), px)      # a resampled pixel does make the trip


def test_host_tables_equal_the_oracle_and_are_safe_to_index():
    from moco_flow_amd import frames
    pairs = {(a[i], b[i]) for a, b in SWEEP for i in (0, 1)} | {(53, 20), (257, 64), (2, 3), (1000, 333)}
    for n_in, n_out in sorted(pairs):
        bounds, kk, ksize = frames.resize_tables(n_in, n_out)
        ob, ok = FO.coeffs(n_in, n_out)
        assert np.array_equal(bounds, ob) and np.array_equal(kk, ok) and kk.shape == (n_out, ksize), (n_in, n_out)
        assert bounds.dtype == np.int32 and kk.dtype == np.int32
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 1).all() and (bounds.sum(axis=1) <= n_in).all() and (bounds[:, 1] <= ksize).all()
        assert (kk >= 0).all() and (np.abs(kk.sum(axis=1) - (1 << 22)) <= ksize).all()
    assert frames.resize_tables(300, 7)[2] == 87
    with pytest.raises(RuntimeError):
        frames.resize_tables(0, 4)


def test_integer_plate_equals_the_float64_expression(golden):
    d, cases = golden
    assert sorted(c[0] for c in cases["plate"].values()) == [1, 2, 5, 64, 65, 300]
    for name, (F, H, W, Cn, k, soft) in cases["plate"].items():
        frames, masks = d[f"plate_{name}_frames"], d[f"plate_{name}_masks"]
        assert frames.shape == (F, H, W, Cn) and k == int(F * 0.8)
        want = np.floor(255.0 * d[f"plate_{name}_f64"] + 0.5).astype(np.uint8)
        assert np.array_equal(FO.plate(frames, masks, k), want), name
        assert (want.reshape(-1, 3)[0] == 0).all()                                  # the always-masked pixel is black
        assert np.array_equal(want.reshape(-1, 3)[1], np.sort(frames.reshape(F, -1, Cn)[:, 1, :3], axis=0)[k])
    rng = np.random.default_rng(11)
    for F in (1, 2, 5, 64, 65, 300):
        for soft in (False, True):
            frames, masks = FO.plate_inputs(rng, F, 4, 5, 3, soft)
            for k in {0, int(F * 0.8), F - 1}:
                assert np.array_equal(FO.plate(frames, masks, k), FO.plate_float64_bytes(frames, masks, k)), (F, soft, k)
    # no value of the float64 image lies near a rounding boundary: every key u (255 - m) / 65025 is a multiple of 1 / 65025
    key = np.arange(0, 65026, dtype=np.int64)
    assert np.array_equal(np.floor(255.0 * (key / 65025.0) + 0.5).astype(np.int64), (key + 127) // 255)


def test_plate_index_and_its_range():
    from moco_flow_amd import frames
    for F in (1, 2, 5, 64, 65, 300, 65535):
        assert frames.plate_index(F) == int(F * 0.8) == frames.plate_index(F, 0.8)
    assert frames.plate_index(300) == 240 and frames.plate_index(5, 0.0) == 0 and frames.plate_index(5, 0.99) == 4
    for F, q in ((5, 1.0), (5, -0.5), (1, 1.0), (0, 0.8), (65536, 0.8)):
        with pytest.raises(RuntimeError):
            frames.plate_index(F, q)


def test_python_layer_refuses_before_any_launch():
    from moco_flow_amd import frames
    img = torch.zeros((4, 6, 4), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match=r"size must be \(H, W\)"):
        frames.resize(img, 540)
    for fn in (lambda: frames.resize(img, (2, 3)), lambda: frames.composite(img, torch.zeros(3)), lambda: frames.to_rows(img[..., :3]),
               lambda: frames.background_plate(img[None], torch.zeros((1, 4, 6), dtype=torch.uint8))):
        with pytest.raises(RuntimeError, match="no CPU"):
            fn()
    with pytest.raises(RuntimeError, match="uint8"):
        frames.resize(img.float(), (2, 3))


def test_library_exports_header_symbols_and_prototypes():
    import moco_flow_amd as M
    import moco_flow_amd._lib as L
    header = open(os.path.join(ROOT, "include", "mocoflow_hip.h")).read()
    declared = set(re.findall(r"^int(?:32|64)_t (mf_\w+)\(", header, re.M))
    lib = L.lib()
    assert lib.mf_version() == 16 and L.MF_ABI_VERSION == 16 and "#define MF_ABI_VERSION 16" in header
    listed = " ".join(header.split("additive entries since")[1].split("*/")[0].split())
    cites = {"mf_resize_u8_scratch_bytes": "moco_flow_dataset.py:51-55, 169", "mf_resize_u8": "moco_flow_dataset.py:51-55, 169",
             "mf_composite_rows": "moco_flow_dataset.py:169-176", "mf_background_plate": "data_utils.py:150-163"}
    for name in NEW_SYMBOLS:
        assert name in declared and name in L.SYMBOLS, name
        fn = getattr(lib, name)
        assert fn.restype is L.SYMBOLS[name][0] and list(fn.argtypes) == L.SYMBOLS[name][1]
        assert name in listed, name
        comment = header.split(name + "(")[0].rsplit("/*", 1)[1]
        assert cites[name] in comment, name
    i64, i32, p = C.c_int64, C.c_int32, C.c_void_p
    assert L.SYMBOLS["mf_resize_u8_scratch_bytes"] == (i64, [i64, i64, i64, i32, i64, i64])
    assert L.SYMBOLS["mf_resize_u8"] == (i32, [p, i64, i64, i64, i32, i64, i64, p, p, i32, p, p, i32, p, p, p])
    assert L.SYMBOLS["mf_composite_rows"] == (i32, [p, i32, i64, i64, p, i32, p, p])
    assert L.SYMBOLS["mf_background_plate"] == (i32, [p, p, i64, i64, i64, i32, i64, i32, p, p])
    assert (L.MF_BACKGROUND_U8, L.MF_PLATE_AUTO, L.MF_PLATE_STAGED, L.MF_PLATE_STREAMED) == (3, 0, 1, 2)
    assert "enum { MF_BACKGROUND_U8 = 3 }" in header and "MF_PLATE_AUTO = 0, MF_PLATE_STAGED = 1, MF_PLATE_STREAMED = 2" in header
    for name in ("frames", "resize", "composite", "to_rows", "background_plate"):
        assert name in M.__all__ and hasattr(M, name)
    assert M.resize is M.frames.resize
    make = open(os.path.join(ROOT, "moco_flow_amd", "csrc", "Makefile")).read()
    assert "mf_frames.hip" in make and "mf_pixels.hpp" in make
    # the per-pixel expression lives in one header that both units include
    batch = open(os.path.join(ROOT, "moco_flow_amd", "csrc", "mf_batch.hip")).read()
    unit = open(os.path.join(ROOT, "moco_flow_amd", "csrc", "mf_frames.hip")).read()
    assert '#include "mf_pixels.hpp"' in batch and '#include "mf_pixels.hpp"' in unit
    assert "kInv255" not in batch and "kInv255" not in unit and "composite_u8_rgba(" in batch and "composite_u8_rgba(" in unit
    assert "frames.py" in open(os.path.join(ROOT, "README.md")).read()


def test_resize_refusals_before_any_launch():
    import moco_flow_amd._lib as L
    lib = L.lib()
    fake, odd = C.c_void_p(256), C.c_void_p(258)
    err = lambda: lib.mf_last_error()
    call = lambda F, H0, W0, Cn, H, W, **kw: lib.mf_resize_u8(
        kw.get("src", fake), F, H0, W0, Cn, H, W, kw.get("xb", fake), kw.get("xk", fake), kw.get("xks", 5), kw.get("yb", fake),
        kw.get("yk", fake), kw.get("yks", 5), kw.get("dst", fake), kw.get("scratch", fake), None)
    assert lib.mf_resize_u8_scratch_bytes(3, 37, 53, 4, 16, 20) == 3 * 37 * 20 * 4
    assert lib.mf_resize_u8_scratch_bytes(3, 37, 53, 4, 37, 20) == 0 and lib.mf_resize_u8_scratch_bytes(3, 37, 53, 4, 16, 53) == 0
    assert lib.mf_resize_u8_scratch_bytes(0, 37, 53, 3, 16, 20) == 0
    for Cn in (0, 2, 5, -1):
        assert lib.mf_resize_u8_scratch_bytes(1, 8, 8, Cn, 4, 4) == -1 and call(1, 8, 8, Cn, 4, 4) == -1 and b"C in {1, 3, 4}" in err()
    for bad in ((-1, 8, 8, 4, 4), (1, -8, 8, 4, 4), (1, 8, -8, 4, 4), (1, 8, 8, -4, 4), (1, 8, 8, 4, -4)):
        F, H0, W0, H, W = bad
        assert lib.mf_resize_u8_scratch_bytes(F, H0, W0, 3, H, W) == -1 and call(F, H0, W0, 3, H, W) == -1
    # 32-bit indexing: input, intermediate and output
    assert call(1, 1 << 15, 1 << 14, 4, 8, 8) == -1 and b"2^31" in err()
    assert call(1, 1 << 16, 8, 4, 8, 1 << 13) == -1 and b"2^31" in err()
    assert call(1 << 20, 8, 8, 4, 16, 32) == -1 and b"2^31" in err()
    assert lib.mf_resize_u8_scratch_bytes(1, 1 << 16, 8, 4, 8, 1 << 13) == -1
    # an output of no bytes launches nothing, whatever else is null; an empty input cannot fill an output
    assert call(0, 8, 8, 3, 4, 4, src=None, dst=None) == 0 and call(2, 8, 8, 3, 0, 4, src=None, dst=None) == 0
    assert call(2, 0, 0, 3, 0, 0, src=None, dst=None) == 0
    assert call(1, 0, 8, 3, 4, 4) == -1 and b"empty" in err()
    assert call(1, 8, 8, 3, 4, 4, src=None) == -1 and b"null" in err()
    assert call(1, 8, 8, 3, 4, 4, dst=None) == -1
    assert call(1, 8, 8, 3, 8, 4, xb=None) == -1 and b"width" in err()
    assert call(1, 8, 8, 3, 8, 4, xks=0) == -1 and call(1, 8, 8, 3, 8, 4, xk=None) == -1
    assert call(1, 8, 8, 3, 4, 8, yb=None) == -1 and b"height" in err()
    assert call(1, 8, 8, 3, 4, 8, yk=None) == -1 and call(1, 8, 8, 3, 4, 8, yks=0) == -1
    assert call(1, 8, 8, 3, 4, 4, scratch=None) == -1 and b"scratch" in err()
    for kw in (dict(src=odd), dict(dst=odd), dict(scratch=odd)):
        assert call(1, 8, 8, 4, 4, 4, **kw) == -1 and b"aligned" in err()


def test_composite_and_plate_refusals_before_any_launch():
    import moco_flow_amd._lib as L
    lib = L.lib()
    fake, odd = C.c_void_p(256), C.c_void_p(258)
    err = lambda: lib.mf_last_error()
    RGB, RGBA = L.MF_IMAGE_U8_RGB, L.MF_IMAGE_U8_RGBA
    comp = lambda image, kind, H, W, bg, bg_kind, out=fake: lib.mf_composite_rows(image, kind, H, W, bg, bg_kind, out, None)
    assert comp(fake, RGBA, -1, 4, fake, L.MF_BACKGROUND_ROWS) == -1 and comp(fake, RGBA, 4, -1, fake, L.MF_BACKGROUND_ROWS) == -1
    assert comp(fake, RGBA, 1 << 15, 1 << 14, fake, L.MF_BACKGROUND_ROWS) == -1 and b"2^31" in err()
    for kind in (L.MF_IMAGE_NONE, L.MF_IMAGE_ROWS, 4, -1):
        assert comp(fake, kind, 4, 4, fake, L.MF_BACKGROUND_ROWS) == -1 and b"image_kind" in err()
    for bg_kind in (L.MF_BACKGROUND_NONE, 4, -1):
        assert comp(fake, RGBA, 4, 4, fake, bg_kind) == -1 and b"needs a background" in err()
    for bg_kind in (L.MF_BACKGROUND_ROWS, L.MF_BACKGROUND_COLOUR, L.MF_BACKGROUND_U8):
        assert comp(fake, RGB, 4, 4, fake, bg_kind) == -1 and b"takes no background" in err()
        assert comp(fake, RGBA, 4, 4, None, bg_kind) == -1 and b"null background" in err()
        assert comp(None, RGBA, 4, 4, fake, bg_kind) == -1 and comp(fake, RGBA, 4, 4, fake, bg_kind, out=None) == -1
        assert comp(odd, RGBA, 4, 4, fake, bg_kind) == -1 and b"aligned" in err()
        assert comp(None, RGBA, 0, 4, None, bg_kind, out=None) == 0                  # no pixels: nothing is launched
    assert comp(None, RGB, 4, 4, None, L.MF_BACKGROUND_NONE) == -1 and comp(None, RGB, 4, 0, None, L.MF_BACKGROUND_NONE, out=None) == 0
    # mf_ray_batch still refuses the byte background: the new kind belongs to mf_composite_rows alone
    a = L.mf_ray_batch_args()
    a.H, a.W, a.focal, a.background_kind = 4, 4, 50.0, L.MF_BACKGROUND_U8
    assert lib.mf_ray_batch(C.byref(a), None) == -1 and b"background_kind" in err()

    plate = lambda F, H, W, Cn, k, path=L.MF_PLATE_AUTO, fr=fake, ms=fake, out=fake: lib.mf_background_plate(fr, ms, F, H, W, Cn, k, path, out, None)
    unit = open(os.path.join(ROOT, "moco_flow_amd", "csrc", "mf_frames.hip")).read()
    bound = int(re.search(r"\bkPlateLdsMaxFrames = (\d+)", unit).group(1))
    tile = int(re.search(r"\bkPlateTilePixels = (\d+)", unit).group(1))
    assert (bound + 3) // 4 * 4 * tile * 3 * 2 <= 160 * 1024 < (bound + 4) // 4 * 4 * tile * 3 * 2       # the largest F the LDS holds
    for F in (0, -1, 65536):
        assert plate(F, 4, 4, 3, 0) == -1 and b"F=" in err()
    for F, k in ((5, 5), (5, -1), (1, 1), (300, 300)):
        assert plate(F, 4, 4, 3, k) == -1 and b"k=" in err()
    for Cn in (1, 2, 5):
        assert plate(5, 4, 4, Cn, 2) == -1 and b"C in {3, 4}" in err()
    assert plate(5, -4, 4, 3, 2) == -1 and plate(5, 4, -4, 3, 2) == -1
    assert plate(5, 1 << 15, 1 << 14, 3, 2) == -1 and b"2^31" in err()
    assert plate(5, 4, 4, 3, 2, path=3) == -1 and plate(5, 4, 4, 3, 2, path=-1) == -1 and b"path" in err()
    assert plate(bound + 1, 4, 4, 3, 2, path=L.MF_PLATE_STAGED) == -1 and b"staged" in err()
    for kw in (dict(fr=None), dict(ms=None), dict(out=None)):
        assert plate(5, 4, 4, 4, 2, **kw) == -1 and b"null" in err()
    assert plate(5, 0, 4, 3, 2, fr=None, ms=None, out=None) == 0 and plate(5, 4, 0, 4, 4, fr=None, ms=None, out=None) == 0
