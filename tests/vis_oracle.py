"""TEST INFRASTRUCTURE ONLY -- numpy restatement of the reference's picture path, under the installed numpy:

  visualize_depth   utils/vis_utils.py:32-40 line for line (nan_to_num, min / max, normalise, 255 x, astype(uint8)), then the
                    colour table gather and ToTensor's / 255
  jet_lut           OPENCV RESTATED, UNPINNED AGAINST cv2 ITSELF: cv2 is not available here; OpenCV's Jet from its closed form
                    in float64, with applyColorMap's BGR order read as RGB as the reference does (column 0 is the b curve)
  quantise          torchvision.utils.save_image: mul(255).add_(0.5).clamp_(0, 255).to(uint8), each step in fp32
  sheet             torch.cat(panels, dim=-1) of trainer_moco_flow.py:614-621, 650-655 as (H, k W, 3) bytes and (3, H, k W) floats

Every array is float32 and every scalar np.float32, so each operation rounds once to fp32 (numpy 2 keeps a float32 array
or scalar float32 against a Python float; the 1e-8 of line 39 is written np.float32(1e-8) so that numpy 1 does the same).
mi / ma given by the caller are taken as np.float32: the device holds the range in fp32.

ONE DEVIATION, shared with the kernels and stated in include/mocoflow_hip.h: astype(np.uint8) of a value outside [0, 256) or
of NaN is undefined behaviour (numpy warns and returns what the C cast gives on the machine at hand), which happens with a
caller-given range narrower than the data and with infinities in the data; there the value is clamped to 0 .. 255 first,
NaN to 0.  Inside [0, 256) nothing changes: the cast truncates."""
import numpy as np


def jet_lut():
    x = np.arange(256, dtype=np.float64) / 255
    curve = lambda up, down: np.clip(np.minimum(4 * x + up, down - 4 * x), 0, 1)
    r, g, b = curve(-1.5, 4.5), curve(-0.5, 3.5), curve(0.5, 2.5)
    return np.rint(np.stack([b, g, r], axis=1) * 255).astype(np.uint8)         # rint: ties to even


def depth_index(depth, mi=None, ma=None):
    """vis_utils.py:32-40 -> the uint8 index plane."""
    x = np.asarray(depth, dtype=np.float32)
    with np.errstate(all="ignore"):
        if mi is not None and ma is not None:
            mi, ma = np.float32(mi), np.float32(ma)
            x = np.nan_to_num(x, nan=ma)
        else:
            x = np.nan_to_num(x)
            mi = np.min(x) if x.size else np.float32(0)
            ma = np.max(x) if x.size else np.float32(0)
        x = (x - mi) / (ma - mi + np.float32(1e-8))
        t = np.float32(255) * x
        assert x.dtype == np.float32 and t.dtype == np.float32
        t = np.where(np.isnan(t), np.float32(0), np.clip(t, np.float32(0), np.float32(255)))     # the one deviation (docstring)
        return t.astype(np.uint8)


def visualize_depth(depth, mi=None, ma=None, lut=None):
    """(H, W) -> (3, H, W) float32, as Image.fromarray(applyColorMap(x)) through ToTensor."""
    lut = jet_lut() if lut is None else np.asarray(lut)
    rgb = lut[depth_index(depth, mi, ma)]                                       # (H, W, 3) bytes
    return np.ascontiguousarray(np.moveaxis(rgb.astype(np.float32) / np.float32(255), -1, 0))


def quantise(v):
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(all="ignore"):
        t = np.clip(v * np.float32(255) + np.float32(0.5), np.float32(0), np.float32(255))
        assert t.dtype == np.float32
        return np.where(np.isnan(t), np.float32(0), t).astype(np.uint8)


def sheet(panels, H, W, lut=None):
    """panels: (H W, 3) float32 rows, or depth planes (H W,) / (H, W), or (depth, mi, ma) -> ((H, k W, 3) uint8, (3, H, k W)
    float32): a colour-mapped pixel keeps its table byte, an rgb pixel is quantised."""
    lut = jet_lut() if lut is None else np.asarray(lut)
    u8, fl = [], []
    for entry in panels:
        a, mi, ma = entry if isinstance(entry, tuple) else (entry, None, None)
        a = np.asarray(a, dtype=np.float32)
        if a.ndim == 2 and a.shape == (H * W, 3) and mi is None:
            rgb = a.reshape(H, W, 3)
            u8.append(quantise(rgb))
            fl.append(np.moveaxis(rgb, -1, 0))
        else:
            idx = depth_index(a.reshape(H, W), mi, ma)
            u8.append(lut[idx])
            fl.append(np.moveaxis(lut[idx].astype(np.float32) / np.float32(255), -1, 0))
    return np.concatenate(u8, axis=1), np.ascontiguousarray(np.concatenate(fl, axis=2))


def depth_plane(n, seed, sentinels=True):
    """The GPU tests' depths: seeded uniform in [2, 6], with mf_image_compose's sentinels 8 and 10 sprinkled in."""
    rng = np.random.default_rng(seed)
    d = rng.uniform(2.0, 6.0, n).astype(np.float32)
    if sentinels and n > 2:
        pick = rng.uniform(size=n)
        d[pick < 0.05] = 8.0
        d[pick > 0.95] = 10.0
    return d
