#!/usr/bin/env python3
"""Frame sheets (visualize_frame / visualize_video, trainer_moco_flow.py:590-661): moco_flow_amd.vis.frame_sheet on a
540 x 540 five-panel sheet [gt | pred | depth | novel pred | novel depth] -- two mf_depth_range reductions and one
mf_frame_sheet launch, bytes and float planes -- beside the same result built from eager device ops on the same GPU
(per depth panel: nan_to_num, amin / amax, normalise, .to(uint8), table gather, / 255, permute; per rgb panel: view + permute;
then cat and save_image's mul(255).add(.5).clamp.to(uint8) and the permute to (H, 5 W, 3)).  The reference itself does the
colour map on the host (cv2), which this does not time.

Per row: device time per call from HIP events around each call, 5 warm-up calls, median of 20.  Also: the bytes the sheet
must move (panels read once, both outputs written once) over the HBM copy rate measured here (a 1 GiB device-to-device
copy, read + write counted).  A sheet is about 12 MB: both sides are launch-bound, no fraction of a peak is meant.
Usage: time_vis.py [H W]  (default 540 540)"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from moco_flow_amd import vis

H, W = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (540, 540)
dev = torch.device("cuda")
gen = torch.Generator().manual_seed(0)
y = torch.linspace(0, 1, H)[:, None, None]
x = torch.linspace(0, 1, W)[None, :, None]
gt = (0.5 + 0.5 * torch.sin(9 * x + 5 * y + torch.arange(3.0))).reshape(H * W, 3)
pred = (gt + 0.05 * torch.randn(gt.shape, generator=gen)).clamp(0, 1)
novel = pred.flip(0).contiguous()
depth = 2 + 4 * torch.rand(H * W, generator=gen)
depth[torch.rand(H * W, generator=gen) < 0.3] = 8.0            # mf_image_compose's sentinel outside the mask
novel_depth = depth.flip(0).contiguous()
gt, pred, novel, depth, novel_depth = (t.to(dev) for t in (gt, pred, novel, depth, novel_depth))
lut = vis.colormap_lut().to(dev)
lut_f = lut.float()


def eager_depth(d):
    v = torch.nan_to_num(d.view(H, W))
    mi, ma = v.amin(), v.amax()
    i = (255 * ((v - mi) / (ma - mi + 1e-8))).to(torch.uint8)
    return (lut_f[i.long()] / 255).permute(2, 0, 1)


def eager():
    img = lambda rows: rows.view(H, W, 3).permute(2, 0, 1)
    stack = torch.cat([img(gt), img(pred), eager_depth(depth), img(novel), eager_depth(novel_depth)], dim=-1)
    sheet = stack.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8)
    return sheet, stack


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


panels = [gt, pred, depth, novel, novel_depth]
print(f"sheet {H} x {5 * W} x 3 from five {H} x {W} panels (3 rgb, 2 depth); ms per call (median of 20 / min / max)")
results = {}
for name, f in (("frame_sheet (2 mf_depth_range + 1 mf_frame_sheet)", lambda: vis.frame_sheet(panels, H, W, planar=True)),
                ("frame_sheet, bytes only", lambda: (vis.frame_sheet(panels, H, W), None)),
                ("eager device ops", eager)):
    med, lo, hi, out = timeit(f)
    results[name] = (med, out)
    print(f"  {name:52s} {med:8.4f} / {lo:8.4f} / {hi:8.4f}", flush=True)
ours, theirs = results["frame_sheet (2 mf_depth_range + 1 mf_frame_sheet)"][1], results["eager device ops"][1]
# (torch divides a device tensor by a scalar as a multiplication by its reciprocal: the eager table values b / 255 may sit one ulp
#  from the fp32 quotient that ToTensor computes on the host and mf_depth_colormap on the device)
print(f"  bytes equal to the eager sheet: {torch.equal(ours[0], theirs[0])}; float planes: max |difference| "
      f"{(ours[1] - theirs[1]).abs().max().item():.2e}")

src = torch.empty(1 << 28, dtype=torch.float32, device=dev)
dst = torch.empty_like(src)
copy_ms = timeit(lambda: dst.copy_(src))[0]
rate = 2 * src.numel() * 4 / (copy_ms * 1e-3)
moved = (3 * 3 + 2) * H * W * 4 + 2 * H * W * 4 + 5 * H * W * 3 * (1 + 4)     # panels, the depth planes once more for the range, both outputs
med = results["frame_sheet (2 mf_depth_range + 1 mf_frame_sheet)"][0]
print(f"  HBM copy rate {rate / 1e12:.2f} TB/s (1 GiB device-to-device); the sheet moves {moved / 1e6:.1f} MB = "
      f"{moved / rate * 1e3:.4f} ms at that rate, {moved / rate * 1e3 / med:.3f} of the measured {med:.4f} ms")
