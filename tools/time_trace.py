#!/usr/bin/env python3
"""Time surface tracing on the GPU box (csrc/trace.hip) on the seed-11 ``trained`` weights, next to the routes there were before it:
``trace_surface`` against ``ray_marching`` at 1 024 and 16 384 rays of the synthetic camera (``weightgen.make_rays``) and on one
640 x 512 frame of it, with the evaluations per ray, the iteration histogram, the mean over tiles of the slowest row -- what the launch
pays -- and |sdf| (the fp32 query) at both depths; ``render_surface_frames`` against ``render_frames`` for that frame; and the
tile-height table: 1 024, 16 384 and 327 680 rays on 32- and on 64-ray tiles.  Events on the launch stream, one warm-up, median of 5
(3 for the frame renders).  Numbers are recorded, not gated.

    python tools/time_trace.py [--out profiles/trace_time.json]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np
import torch

import weightgen
from endosurf_amd import tracing
from gpu_util import renderer_for

REPS = 5
H, W, FOCAL = 512, 640, 800.0


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


def frame_rays(t=0.5):
    """Every pixel of the camera ``weightgen.make_rays`` draws from: o = (0, 0, -1.5), pinhole 640 x 512, f = 800; [H, W, 9]."""
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    d = np.stack([(u - 319.5) / FOCAL, (v - 255.5) / FOCAL, np.ones_like(u)], -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    rays = np.zeros((H, W, 9), np.float32)
    rays[..., :3], rays[..., 3:6], rays[..., 8] = (0.0, 0.0, -1.5), d, t
    return torch.from_numpy(rays)


def slowest_row_mean(iters, tile):
    n = iters.numel()
    pad = torch.zeros((n + tile - 1) // tile * tile, dtype=iters.dtype, device=iters.device)
    pad[:n] = iters
    return float(pad.view(-1, tile).max(dim=1).values.float().mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "trace_time.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    r = renderer_for(11, "trained", True)
    eng = r.engine
    result = {"weights": "weightgen.make_state(11, 'trained', True)", "reps": REPS, "defaults": "tau 0, eps 1e-5, relax 1, min_step 1e-3, max_iters 128",
              "sizes": [], "tile_heights": [], "frame_render": {}}
    frame = frame_rays().to(r.device)
    sets = [("1024 rays", torch.from_numpy(weightgen.make_rays(91, 1024)).to(r.device)),
            ("16384 rays", torch.from_numpy(weightgen.make_rays(91, 16384)).to(r.device)), ("640x512 frame", frame.reshape(-1, 9))]
    with torch.cuda.device(r.device), torch.no_grad():
        weff, packed = r._weights()
        weff = weff.detach()
        for name, rays in sets:
            n = rays.shape[0]
            row = {"rays": name, "N": n}
            row["trace_surface_ms"] = median_ms(lambda: r.trace_surface(rays))
            row["ray_marching_ms"] = median_ms(lambda: r.ray_marching(rays))
            row["ray_marching_over_trace_surface"] = row["ray_marching_ms"] / row["trace_surface_ms"]
            tr, march = r.trace_surface(rays), r.ray_marching(rays).reshape(-1)
            it = tr["iters"]
            march_hit = torch.isfinite(march) & (march != 0)
            w = rays[:, 3:6] / (rays[:, 5:6] + 1e-6)
            at_march = r.sdf_observed(rays[:, :3] + torch.where(march_hit, march, torch.zeros_like(march))[:, None] * w, rays[:, 8]).reshape(-1).abs()
            at_trace = r.sdf_observed(tr["points"], rays[:, 8]).reshape(-1).abs()
            row.update(evaluations_per_ray=float(it.float().mean()), evaluations_per_ray_ray_marching=136, iters_max=int(it.max()),
                       iters_histogram=torch.bincount(it.long(), minlength=129).tolist(), tile_rows=32,
                       slowest_row_mean_over_tiles=slowest_row_mean(it, 32), slowest_row_mean_over_64_row_tiles=slowest_row_mean(it, 64),
                       status_counts={k: int((tr["status"] == v).sum()) for k, v in (("hit", tracing.HIT), ("miss", tracing.MISS),
                                                                                      ("occupied", tracing.OCCUPIED), ("not_converged", tracing.NOT_CONVERGED))},
                       hit_differs_from_ray_marching=int((tr["valid"] != march_hit).sum()),
                       abs_sdf_at_trace_depth={"median": float(at_trace[tr["valid"]].median()), "max": float(at_trace[tr["valid"]].max())},
                       abs_sdf_at_ray_marching_depth={"median": float(at_march[march_hit].median()), "max": float(at_march[march_hit].max())})
            result["sizes"].append(row)
            print(json.dumps({k: v for k, v in row.items() if k != "iters_histogram"}), flush=True)
        for n in (1024, 16384, H * W):
            rays = frame.reshape(-1, 9)[:n] if n == H * W else torch.from_numpy(weightgen.make_rays(91, n)).to(r.device)
            row = {"N": n}
            for tile in (32, 64):
                row[f"tile{tile}_ms"] = median_ms(lambda: eng.trace_surface(rays, weff, packed, True, tile_points=tile))
            result["tile_heights"].append(row)
            print(json.dumps(row), flush=True)
        fr = result["frame_render"]
        fr["render_surface_frames_ms"] = median_ms(lambda: r.render_surface_frames(frame), reps=3)
        fr["render_frames_ms"] = median_ms(lambda: r.render_frames(frame, iter_step=1, perturb_overwrite=False), reps=3)
        fr["render_frames_over_render_surface_frames"] = fr["render_frames_ms"] / fr["render_surface_frames_ms"]
        fr["valid_pixels"] = int(r.render_surface_frames(frame)["valid"].sum())
        print(json.dumps(fr), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            json.dump(result, fo, indent=1)


if __name__ == "__main__":
    main()
