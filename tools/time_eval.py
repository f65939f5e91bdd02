#!/usr/bin/env python3
"""Time the frame evaluation on the GPU box (csrc/metrics.hip) for 1 and 16 frames of 640 x 512: SSIM (with and without the map store),
the masked squared sums, the five panels into one sheet, and EndoSurfRenderer.evaluate_rendered (= evaluate_frames without
render_frames: two sums, SSIM, panels, one read-back).  Beside them, for scale: the same SSIM formula in fp32 through
torch.nn.functional.conv2d on the device, and the host route the package had before (data.cal_psnr on device inputs: copy the stacks
to the host, reduce in numpy).  Events on the launch stream, one warm-up, median of 5.

    python tools/time_eval.py [--frames 1 16] [--size 512 640] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import torch
import torch.nn.functional as F

from endosurf_amd import data as D
from endosurf_amd.imaging import ssim_window

REPS = 5


def median_ms(fn, reps=REPS):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def ssim_conv2d(a, b, mask, window):
    """The reference's formula with stock ops, fp32: what a port without a kernel of its own would run."""
    a, b = (a * mask).permute(0, 3, 1, 2), (b * mask).permute(0, 3, 1, 2)
    c = a.shape[1]
    w = window.expand(c, 1, 11, 11).contiguous()
    mu1, mu2 = F.conv2d(a, w, groups=c), F.conv2d(b, w, groups=c)
    s1, s2, s12 = F.conv2d(a * a, w, groups=c) - mu1 * mu1, F.conv2d(b * b, w, groups=c) - mu2 * mu2, F.conv2d(a * b, w, groups=c) - mu1 * mu2
    return (((2 * mu1 * mu2 + 1e-4) * (2 * s12 + 9e-4)) / ((mu1 * mu1 + mu2 * mu2 + 1e-4) * (s1 + s2 + 9e-4))).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--size", type=int, nargs=2, default=[512, 640], metavar=("H", "W"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    from gpu_util import renderer_for_case
    from oracle_util import load_case
    r = renderer_for_case(load_case("trained_deform"))
    eng = r.engine
    H, W = args.size
    rows = []
    with torch.cuda.device(r.device):
        window = torch.from_numpy(ssim_window()).to(r.device)
        for n in args.frames:
            g = torch.Generator(device=r.device).manual_seed(n)
            rnd = lambda *s: torch.rand(*s, device=r.device, generator=g)
            gt, depth_gt = rnd(n, H, W, 3), rnd(n, H, W, 1) + 0.5
            col, dep, nrm = (gt + 0.05 * (rnd(n, H, W, 3) - 0.5)).contiguous(), depth_gt + 0.02 * rnd(n, H, W, 1), rnd(n, H, W, 3) - 0.5
            cmask, mask = (rnd(n, H, W, 1) > 0.1).float(), (rnd(n, H, W, 1) > 0.3).float()
            poses = torch.eye(4).repeat(n, 1, 1)
            out5, out2 = eng.empty(n + 1, dtype=torch.float64), eng.empty(2 * n + 2, dtype=torch.float64)
            row = {"frames": n, "height": H, "width": W, "reps": REPS}
            row["ssim_ms"] = median_ms(lambda: eng.ssim(gt, col, cmask, out=out5))
            row["ssim_with_map_ms"] = median_ms(lambda: eng.ssim(gt, col, cmask, full=True))
            row["sq_sums_ms"] = median_ms(lambda: eng.masked_sq_sums(gt, col, cmask, out=out2))
            row["panels_ms"] = median_ms(lambda: eng.eval_panels(gt, col, depth_gt, dep, nrm, poses, 1.5))
            rendered = {"color": col.view(-1, 3), "depth": dep.view(-1, 1), "normal": nrm.view(-1, 3)}
            row["evaluate_rendered_ms"] = median_ms(lambda: r.evaluate_rendered(rendered, gt, depth_gt, mask, cmask, poses, 1.5))
            row["ssim_fp64_fma_per_s"] = 605.0 * n * (H - 10) * (W - 10) * 3 / (row["ssim_ms"] * 1e-3)
            row["torch_conv2d_ssim_fp32_ms"] = median_ms(lambda: ssim_conv2d(gt, col, cmask, window))
            row["host_cal_psnr_ms"] = median_ms(lambda: D.cal_psnr(gt, col, cmask))
            row["ssim_value"] = float(out5[n])
            row["torch_conv2d_ssim_value"] = float(ssim_conv2d(gt, col, cmask, window))
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            json.dump(rows, fo, indent=1)


if __name__ == "__main__":
    main()
