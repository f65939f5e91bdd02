#!/usr/bin/env python3
"""Time the deformation-only kernels on the GPU box (csrc/deform.hip) on the seed-11 ``trained`` weights: es_deform_forward and
es_deform_inverse at M = 2 630, 65 536 and 1 048 576 rows, and at 16 384 and 16 385, the two sides of the tile-height threshold (points uniform in [-0.8, 0.8]^3, a random t_from / t_to per row, the
canonical points from es_deform_forward, y_0 = c, max_iters 64, tol 1e-5), with the mean and largest iteration count and the rate in
MMAC/s at 0.46 MMAC per row and evaluation (counted as what the launch executes: every tile rides until its last row has frozen) --
next to the only route there was before: ``tracking.inverse_deform`` over ``renderer.model.deform_network``, a full point evaluation,
a launch chain and a ``nonzero`` read-back per iteration.  Then the stopping length: tol = 1e-5, 3e-6, 1e-6, 3e-7 at 65 536 rows, with
the number of rows that end unconverged and the largest iteration count.  Events on the launch stream, one warm-up, median of 5.
Numbers are recorded, not gated.

    python tools/time_track.py [--rows 2630 16384 16385 65536 1048576] [--twin-max 1048576] [--out profiles/track_time.json]
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

from endosurf_amd import tracking
from gpu_util import renderer_for

REPS = 5
MMAC_PER_EVAL = 0.46
MAX_ITERS = 64
TOLS = (1e-5, 3e-6, 1e-6, 3e-7)


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


def tile_evaluations(iters):
    """Row evaluations the launch executes: each tile (32 rows up to 16 384 rows, 64 above: csrc/deform.hip) runs as many evaluations as
    its slowest row, on all of its rows."""
    M = iters.numel()
    T = 32 if M <= 16384 else 64
    pad = torch.zeros((M + T - 1) // T * T, dtype=iters.dtype, device=iters.device)
    pad[:M] = iters
    return int(pad.view(-1, T).max(dim=1).values.sum()) * T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[2630, 16384, 16385, 65536, 1048576])
    ap.add_argument("--twin-max", type=int, default=1048576, help="largest row count at which the host twin over deform_network is timed")
    ap.add_argument("--sweep-rows", type=int, default=65536)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "track_time.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    r = renderer_for(11, "trained", True)
    eng = r.engine
    result = {"weights": "weightgen.make_state(11, 'trained', True)", "reps": REPS, "max_iters": MAX_ITERS, "mmac_per_row_and_evaluation": MMAC_PER_EVAL,
              "sizes": [], "tol_sweep": []}

    def inputs(M):
        rng = np.random.default_rng(111)
        x = torch.from_numpy(rng.uniform(-0.8, 0.8, size=(M, 3)).astype(np.float32)).to(r.device)
        t_from, t_to = (torch.from_numpy(rng.uniform(size=(M,)).astype(np.float32)).to(r.device) for _ in range(2))
        return x, t_from, t_to

    with torch.cuda.device(r.device), torch.no_grad():
        weff, packed = r._weights()
        weff = weff.detach()
        for M in args.rows:
            x, t_from, t_to = inputs(M)
            c = eng.deform_forward(eng.points(x=x, t=t_from), weff, packed, want="xc")
            row = {"M": M}
            row["forward_ms"] = median_ms(lambda: eng.deform_forward(eng.points(x=x, t=t_from), weff, packed, want="both"))
            row["forward_mmac_per_s"] = M * MMAC_PER_EVAL / (row["forward_ms"] * 1e-3)
            solve = lambda tol=1e-5: eng.deform_inverse(eng.points(x=c, t=t_to), None, weff, packed, MAX_ITERS, tol)
            row["inverse_ms"] = median_ms(solve)
            y, step, iters = solve()
            ev = tile_evaluations(iters)
            row.update(tol=1e-5, iters_mean=float(iters.float().mean()), iters_max=int(iters.max()), unconverged=int((step > 1e-5).sum()),
                       row_evaluations_needed=int(iters.sum()), row_evaluations_executed=ev,
                       inverse_mmac_per_s=ev * MMAC_PER_EVAL / (row["inverse_ms"] * 1e-3))
            if M <= args.twin_max:
                twin = lambda: tracking.inverse_deform(r.model.deform_network, c, t_to, None, MAX_ITERS, 1e-5)
                row["twin_over_deform_network_ms"] = median_ms(twin)
                ty, ts, ti = twin()
                row.update(twin_iters_max=int(ti.max()), twin_unconverged=int((ts > 1e-5).sum()),
                           twin_max_distance=float(torch.linalg.norm(ty - y, dim=-1).max()))
            result["sizes"].append(row)
            print(json.dumps(row), flush=True)
        x, t_from, t_to = inputs(args.sweep_rows)
        c = eng.deform_forward(eng.points(x=x, t=t_from), weff, packed, want="xc")
        for tol in TOLS:
            ms = median_ms(lambda: eng.deform_inverse(eng.points(x=c, t=t_to), None, weff, packed, MAX_ITERS, tol))
            y, step, iters = eng.deform_inverse(eng.points(x=c, t=t_to), None, weff, packed, MAX_ITERS, tol)
            row = {"M": args.sweep_rows, "tol": tol, "inverse_ms": ms, "unconverged": int((step > tol).sum()), "iters_max": int(iters.max()),
                   "iters_mean": float(iters.float().mean())}
            result["tol_sweep"].append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            json.dump(result, fo, indent=1)


if __name__ == "__main__":
    main()
