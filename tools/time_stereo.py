#!/usr/bin/env python3
"""Time the stereo matcher on the GPU box (csrc/stereo.hip): census, cost, aggregation, selection and the speckle filter
each alone, and ``Engine.stereo_disparity`` as a whole, at 640 x 512 with D = 128 for 1 and 8 pairs and at 1280 x 1024 with D = 256 for
one pair, on a smooth value-noise texture whose rows are shifted by a disparity that grows down the image.  The aggregation's effective
bytes/s are its algorithmic traffic -- per path, C read once and S read and written once -- over its time, beside the 6.29 TB/s a float4
copy reaches on this chip.  The numpy twin is timed at 48 x 96 with D = 32 on the host clock.  Events on the launch stream, one warm-up,
median of 5.  Numbers are recorded, not gated.

    python tools/time_stereo.py [--out profiles/stereo_time.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np
import torch

import stereo_util as U
from endosurf_amd import stereo
from endosurf_amd._lib import check, ptr

REPS = 5
SHAPES = [(1, 512, 640, 128), (8, 512, 640, 128), (1, 1024, 1280, 256)]          # (pairs, H, W, D)
P1, P2, PATHS, UNIQUENESS, LR_MAX, SPECKLE_SIZE, SPECKLE_RANGE, POLL = 7, 60, 8, 10, 1, 100, 1, 8
COPY_BYTES_PER_S = 6.29e12          # float4 copy, MI355X


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


def pairs(n, H, W, D):
    """n pairs uint8 [n,H,W]: left = texture(x, y), right[y, x] = texture(x + d(y), y) with d(y) from D / 8 at the top to D / 2 at the
    bottom (a slanted floor), pair k shifted by k texture cells."""
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    d = D / 8.0 + (D / 2.0 - D / 8.0) * y / max(H - 1, 1)
    q = lambda t: np.minimum(np.floor(t * 256.0), 255).astype(np.uint8)
    left = np.stack([q(U.texture(0.25 * x + k, 0.25 * y, (1.0, 2.0, 4.0))) for k in range(n)])
    right = np.stack([q(U.texture(0.25 * (x + d) + k, 0.25 * y, (1.0, 2.0, 4.0))) for k in range(n)])
    return left, right, d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "stereo_time.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    from endosurf_amd.engine import Engine
    eng = Engine("cuda")
    lib = eng.lib
    result = {"reps": REPS, "p1": P1, "p2": P2, "paths": PATHS, "uniqueness": UNIQUENESS, "lr_max": LR_MAX, "speckle_size": SPECKLE_SIZE,
              "speckle_range": SPECKLE_RANGE, "poll": POLL, "copy_bytes_per_s": COPY_BYTES_PER_S, "shapes": []}
    with torch.cuda.device(eng.device), torch.no_grad():
        for n, H, W, D in SHAPES:
            left, right, truth = pairs(n, H, W, D)
            gl, gr = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
            st = eng.st()
            cl, cr = eng.empty(n, H, W, dtype=torch.int64), eng.empty(n, H, W, dtype=torch.int64)
            cost, S = eng.empty(n, H, W, D, dtype=torch.uint8), eng.empty(n, H, W, D, dtype=torch.uint16)
            out = eng._stereo_outputs(n, H, W)
            scratch = eng._stereo_scratch(n, H, W)

            def census():
                check(lib.es_stereo_census(ptr(gl), n, H, W, ptr(cl), st))
                check(lib.es_stereo_census(ptr(gr), n, H, W, ptr(cr), st))

            cost_fn = lambda: check(lib.es_sgm_cost(ptr(cl), ptr(cr), n, H, W, D, 0, ptr(cost), st))
            agg = lambda paths: check(lib.es_sgm_aggregate(ptr(cost), n, H, W, D, P1, P2, paths, ptr(S), st))
            select = lambda: eng._sgm_select_into(S, 0, UNIQUENESS, LR_MAX, True, out, scratch)

            def speckle():          # (the filter clears what it drops, so every repeat starts from the selection's outputs)
                work = {k: v.clone() for k, v in out.items()}
                eng._speckle_into(work, SPECKLE_SIZE, SPECKLE_RANGE, POLL, scratch)

            row = {"pairs": n, "height": H, "width": W, "max_disparity": D, "census_ms": median_ms(census), "cost_ms": median_ms(cost_fn),
                   "aggregate_4_paths_ms": median_ms(lambda: agg(4)), "aggregate_ms": median_ms(lambda: agg(PATHS)), "select_ms": median_ms(select)}
            row["speckle_ms"] = median_ms(speckle)
            row["speckle_clone_ms"] = median_ms(lambda: {k: v.clone() for k, v in out.items()})
            row["whole_call_ms"] = median_ms(lambda: eng.stereo_disparity(gl, gr, D, 0, P1, P2, PATHS, UNIQUENESS, LR_MAX, True, SPECKLE_SIZE,
                                                                          SPECKLE_RANGE, POLL))
            row["chunk_pairs"] = eng._stereo_chunk(n, H, W, D)
            cells = n * H * W * D
            row["aggregate_bytes"] = PATHS * (cells + 2 * 2 * cells)
            row["aggregate_bytes_per_s"] = row["aggregate_bytes"] / (row["aggregate_ms"] * 1e-3)
            row["aggregate_share_of_copy_rate"] = row["aggregate_bytes_per_s"] / COPY_BYTES_PER_S
            row["aggregate_lines_per_direction"] = {"rows": n * H, "columns": n * W, "diagonals": n * (H + W - 1)}
            r = eng.stereo_disparity(gl, gr, D, 0, P1, P2, PATHS, UNIQUENESS, LR_MAX, True, SPECKLE_SIZE, SPECKLE_RANGE, POLL)
            cols = np.zeros((n, H, W), bool)
            cols[:, :, D:] = True
            e = stereo.stereo_errors(r["disparity"].cpu().numpy(), r["valid"].cpu().numpy(), np.broadcast_to(truth, (n, H, W)), cols)
            row["density"], row["mean_abs_error_px"], row["within_1px"] = e["density"], e["mean_abs_error"], e["within"][1.0]
            result["shapes"].append(row)
            print(json.dumps(row), flush=True)
            del cl, cr, cost, S, out, scratch, r
            torch.cuda.empty_cache()
    s = U.scene("bump")
    t0 = time.perf_counter()
    stereo.stereo_disparity(s["left"], s["right"], U.SCENE_D, speckle_size=U.SPECKLE_SIZE)
    result["twin"] = {"height": U.SCENE_H, "width": U.SCENE_W, "max_disparity": U.SCENE_D, "host_ms": (time.perf_counter() - t0) * 1e3}
    print(json.dumps(result["twin"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
