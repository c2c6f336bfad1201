#!/usr/bin/env python3
"""Frame ingest of a sequence on the device (moco_flow_amd.frames; datasets/moco_flow_dataset.py:45, 51-55, 169-176 and
scripts/data_utils.py:150-163): a stack of F RGBA frames at S0 x S0 with its masks ->
    resize            the whole stack to S x S (PIL's antialiased bilinear resample, bit for bit)
    composite         one S x S frame over the resized plate's rows
    background_plate  the S0 x S0 plate of the F frames and masks (both kernels: keys staged in LDS, and streamed)
    clean_mask        the F mattes from a synthetic alpha stack (one large blob with holes, plus speckle): threshold, largest
                      region, with and without fill_holes; mask_regions: labels and the table (scripts/data_utils.py:135-147)
Per row: device time per call from HIP events around each call, 5 warm-up calls, median of 20; beside it the algorithmic bytes
(every input byte read once, every output byte written once) over the time, as a fraction of the measured 4.69 TB/s copy rate
(README).  Then the host path in the same process: PIL per frame where it imports, and the reference's float64 np.sort on a
strip of rows small enough for host memory, labelled as a strip and scaled to the frame; scipy.ndimage.label + np.bincount per
frame where scipy imports.
Usage: time_frames.py [F S0 S] [--regions]  (default 300 1080 540; --regions: the matte rows alone)"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from moco_flow_amd import frames

REGIONS_ONLY = "--regions" in sys.argv
_args = [a for a in sys.argv[1:] if a != "--regions"]
F, S0, S = (int(_args[0]), int(_args[1]), int(_args[2])) if len(_args) > 2 else (300, 1080, 540)
COPY_RATE = 4.69e12                                      # bytes / s, the measured device copy rate
dev = torch.device("cuda")
gen = torch.Generator(device=dev).manual_seed(0)


def synthetic_matte():
    """(F, S0, S0) alpha bytes: one large blob (an ellipse that moves from frame to frame) with three holes and pin-holes (0.2 % of
    its pixels fall below the threshold), plus speckle outside (0.5 % of the pixels at 255)."""
    alpha = torch.empty((F, S0, S0), dtype=torch.uint8, device=dev)
    y, x = torch.meshgrid(torch.arange(S0, device=dev, dtype=torch.float32), torch.arange(S0, device=dev, dtype=torch.float32), indexing="ij")
    for f in range(F):
        cx, cy = S0 * (0.5 + 0.1 * np.sin(0.05 * f)), S0 * (0.5 + 0.05 * np.cos(0.03 * f))
        blob = ((x - cx) / (0.22 * S0)) ** 2 + ((y - cy) / (0.40 * S0)) ** 2 < 1.0
        for k in range(3):
            blob &= (x - cx - (k - 1) * 0.08 * S0) ** 2 + (y - cy - (k - 1) * 0.2 * S0) ** 2 > (0.03 * S0) ** 2
        noise = torch.rand((S0, S0), device=dev, generator=gen)
        alpha[f] = torch.where(blob, torch.where(noise < 0.002, 120, 255), torch.where(noise < 0.005, 255, 0)).to(torch.uint8)
    return alpha


def regions_rows():
    alpha = synthetic_matte()
    n = alpha.numel()
    print(f"matte clean-up, {F} frames {S0} x {S0} (chunks of {frames._region_chunk(F, S0, S0)} frames):")
    clean = row(f"frames.clean_mask, {F} frames", lambda: frames.clean_mask(alpha), 2 * n)
    filled = row(f"frames.clean_mask, {F} frames, fill_holes", lambda: frames.clean_mask(alpha, fill_holes=True), 2 * n)
    reg = row(f"frames.mask_regions, {F} frames (labels + table)", lambda: frames.mask_regions(alpha), 5 * n)
    row("frames.clean_mask, one frame, fill_holes", lambda: frames.clean_mask(alpha[0], fill_holes=True), 2 * S0 * S0)
    print(f"  regions per frame: {reg.counts.float().mean().item():.0f}; kept pixels per frame {clean.ne(0).sum().item() / F:.0f}, "
          f"with holes filled {filled.ne(0).sum().item() / F:.0f}")
    try:
        import scipy.ndimage as nd
    except ImportError:
        print("  scipy.ndimage does not import here: no host labelling timed")
        return
    ts = []
    for f in range(min(F, 5)):
        a = alpha[f].cpu().numpy()
        t0 = time.perf_counter()
        lab, _ = nd.label(a >= 196, structure=np.ones((3, 3)))
        area = np.bincount(lab.ravel())
        area[0] = 0
        host = (lab == area.argmax()).astype(np.uint8) * 255
        ts.append(time.perf_counter() - t0)
        assert np.array_equal(host, clean[f].cpu().numpy())
        assert np.array_equal(nd.binary_fill_holes(host).astype(np.uint8) * 255, filled[f].cpu().numpy())
    print(f"host path, same process (wall time): scipy.ndimage.label + np.bincount, one frame {statistics.median(ts) * 1e3:9.2f} ms "
          f"(x {F} frames = {statistics.median(ts) * F:7.2f} s); equal to the device's bytes, as is binary_fill_holes")


def timeit(f, warm=5, n=20):
    for _ in range(warm):
        out = f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = f()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts), max(ts), out


def row(name, f, nbytes):
    med, lo, hi, out = timeit(f)
    print(f"  {name:52s} {med:9.4f} / {lo:9.4f} / {hi:9.4f} ms   {nbytes / 1e6:9.1f} MB   {nbytes / (med * 1e-3) / COPY_RATE:6.3f} of the copy rate",
          flush=True)
    return out


if REGIONS_ONLY:
    print("ms per call (median of 20 / min / max), algorithmic bytes, fraction of 4.69 TB/s")
    regions_rows()
    sys.exit(0)
raw = torch.randint(0, 256, (F, S0, S0, 4), dtype=torch.uint8, device=dev, generator=gen)
masks = torch.randint(0, 256, (F, S0, S0), dtype=torch.uint8, device=dev, generator=gen)
print(f"{F} frames {S0} x {S0} RGBA -> {S} x {S}; ms per call (median of 20 / min / max), algorithmic bytes, fraction of 4.69 TB/s")
small = row(f"frames.resize, {F} frames", lambda: frames.resize(raw, (S, S)), F * 4 * (S0 * S0 + S * S))
row("frames.resize, one frame", lambda: frames.resize(raw[0], (S, S)), 4 * (S0 * S0 + S * S))
plate = row(f"frames.background_plate, {F} frames (auto)", lambda: frames.background_plate(raw, masks), F * S0 * S0 * 5 + S0 * S0 * 3)
streamed = row(f"frames.background_plate, {F} frames (streamed)", lambda: frames.background_plate(raw, masks, path="streamed"),
               F * S0 * S0 * 5 + S0 * S0 * 3)
assert torch.equal(plate, streamed)
bkgd = frames.to_rows(frames.resize(plate, (S, S)))
row("frames.composite, one frame over fp32 rows", lambda: frames.composite(small[0], bkgd), S * S * (4 + 12 + 12))
row("frames.to_rows, the plate", lambda: frames.to_rows(plate), S0 * S0 * (3 + 12))

print("host path, same process (wall time):")
frame0, mask_rows = raw[0].cpu().numpy(), None
try:
    from PIL import Image
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        ref = np.asarray(Image.fromarray(frame0).resize((S, S), Image.BILINEAR))
        ts.append(time.perf_counter() - t0)
    assert np.array_equal(ref, small[0].cpu().numpy())
    print(f"  PIL resize, one frame {statistics.median(ts) * 1e3:9.3f} ms (x {F} frames = {statistics.median(ts) * F:7.3f} s); equal to the device's bytes")
except ImportError:
    print("  PIL does not import here: no host resize timed")
strip = max(1, min(S0, (256 << 20) // (F * S0 * 3 * 8)))                   # rows whose float64 copy stays within 256 MB
img = raw[:, :strip].cpu().numpy()
msk = masks[:, :strip].cpu().numpy()
t0 = time.perf_counter()
host = np.sort(np.array([img[i, ..., :3] / 255. * (1 - (msk[i] / 255.)[:, :, np.newaxis]) for i in range(F)]), axis=0)[int(F * 0.8)]
dt = time.perf_counter() - t0
assert np.array_equal(np.floor(255.0 * host + 0.5).astype(np.uint8), plate[:strip].cpu().numpy())
print(f"  float64 np.sort, a STRIP of {strip} of {S0} rows {dt * 1e3:9.1f} ms (scaled to the frame: {dt * S0 / strip:7.2f} s; the whole "
      f"float64 stack would be {F * S0 * S0 * 3 * 8 / 1e9:.1f} GB); equal to the device's bytes")
del raw, masks, img, msk, host
regions_rows()
