#!/usr/bin/env python3
"""Time the pixel tracks on the GPU box (csrc/visible.hip, csrc/flow.hip) on the seed-11 ``trained`` weights:
``segment_visible`` against ``trace_surface`` -- the trace-based route to the same answer -- on the same 16 384 and 327 680 rows (rays of
the synthetic camera; the segments run from the camera to each ray's traced point, the rest to the far side of the unit ball);
``track_pixels`` for 1 024 pixels x 4 frames; ``frame_flow`` and ``stabilize_frames`` for one 640 x 512 frame to 4 frames; and how the
FREE share of frontally seen surface points moves with the margin.  Events on the launch stream, one warm-up, median of 5.  Numbers are
recorded, not gated.

    python tools/time_flow.py [--out profiles/flow_time.json]
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
from endosurf_amd import flow
from gpu_util import renderer_for

REPS = 5
H, W = 512, 640
K = np.array([[800.0, 0.0, 319.5], [0.0, 800.0, 255.5], [0.0, 0.0, 1.0]])
POSE = np.eye(4)
POSE[:3, 3] = (0.0, 0.0, -1.5)
T_FROM, TIMES = 0.3, [0.2, 0.4, 0.6, 0.8]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "flow_time.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    r = renderer_for(11, "trained", True)
    result = {"weights": "weightgen.make_state(11, 'trained', True)", "reps": REPS,
              "defaults": "margin 5e-3, tau 0, relax 1, min_step 1e-3, max_iters 128; trace eps 1e-5; track tol 1e-5", "segment_visible": [], "margins": []}
    with torch.cuda.device(r.device), torch.no_grad():
        for n in (16384, 327680):
            rays = torch.from_numpy(weightgen.make_rays(91, n)).to(r.device)
            tr = r.trace_surface(rays)
            far = rays[:, :3] + 3.0 * rays[:, 3:6]          # a ray that hits nothing: the segment through the whole ball
            ends = torch.where(tr["valid"][:, None], tr["points"], far).contiguous()
            o, t = rays[:, :3].contiguous(), rays[:, 8].contiguous()
            vis = r.segment_visible(o, ends, t)
            row = {"rows": n, "trace_surface_ms": median_ms(lambda: r.trace_surface(rays)),
                   "segment_visible_ms": median_ms(lambda: r.segment_visible(o, ends, t)),
                   "trace_evaluations_per_row": float(tr["iters"].float().mean()), "visible_evaluations_per_row": float(vis["iters"].float().mean()),
                   "trace_hits": int(tr["valid"].sum()), "free": int((vis["status"] == flow.FREE).sum()),
                   "occluded": int((vis["status"] == flow.OCCLUDED).sum()), "unknown": int((vis["status"] == flow.UNKNOWN).sum())}
            result["segment_visible"].append(row)
            print(row, flush=True)
            if n == 16384:
                hit = tr["valid"]
                for margin in (1e-3, 2e-3, 5e-3, 1e-2):
                    st = r.segment_visible(o, ends, t, margin=margin)["status"][hit]
                    m = {"margin": margin, "traced_points": int(hit.sum()), "free_share": float((st == flow.FREE).float().mean()),
                         "occluded": int((st == flow.OCCLUDED).sum()), "unknown": int((st == flow.UNKNOWN).sum())}
                    result["margins"].append(m)
                    print(m, flush=True)
        rng = np.random.default_rng(97)
        px = torch.from_numpy(np.stack([rng.uniform(0, W - 1, 1024), rng.uniform(0, H - 1, 1024)], -1).astype(np.float32)).to(r.device)
        tp = r.track_pixels(px, K, POSE, T_FROM, TIMES, H, W)
        result["track_pixels"] = {"pixels": 1024, "frames": len(TIMES), "ms": median_ms(lambda: r.track_pixels(px, K, POSE, T_FROM, TIMES, H, W)),
                                  "valid": int(tp["valid"].sum()), "visible": int(tp["visible"].sum()), "in_image": int(tp["in_image"].sum())}
        print(result["track_pixels"], flush=True)
        ff = r.frame_flow(K, POSE, T_FROM, TIMES, H, W)
        frames = torch.rand(len(TIMES), H, W, 3, device=r.device)
        result["frame"] = {"height": H, "width": W, "frames": len(TIMES), "frame_flow_ms": median_ms(lambda: r.frame_flow(K, POSE, T_FROM, TIMES, H, W)),
                           "stabilize_frames_ms": median_ms(lambda: r.stabilize_frames(frames, ff)),
                           "flow_to_rgb_ms": median_ms(lambda: r.flow_to_rgb(ff["flow"], 32.0)),
                           "valid_share": float(ff["valid"].float().mean()), "flow_abs_max_px": float(ff["flow"].abs().max())}
        print(result["frame"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
