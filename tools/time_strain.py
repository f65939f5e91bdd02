#!/usr/bin/env python3
"""Time the strain kernels on the GPU box (csrc/deform_jet.hip, csrc/strain.hip) on the seed-11 ``trained`` weights: es_deform_jacobian
-- the value and the three forward tangents of every point in one launch, 4 MLP rows per point -- against the route there was before,
``model.get_deform_grad_from_observed_space``: three launches of the point forward chain, one per unit direction, 6 rows per point
plus the mask and u_l workspace streams, on the same rows (points uniform in [-0.8, 0.8]^3, a random time per row) at M = 2 630,
65 536 and 1 048 576 points, and at 4 096 and 4 097, the two sides of the tile-height threshold; es_strain_rows with and without
normals at the same sizes; and ``renderer.mesh_strain`` on the 2 630-vertex mesh of DESIGN.md 7h (24^3 lattice at t = 0.3) tracked
through t, t + 0.01, t + 0.02, 0.9.  Events on the launch stream, one warm-up each, the candidates interleaved repetition by
repetition, median of 5.  Numbers are recorded, not gated.

    python tools/time_strain.py [--points 2630 4096 4097 65536 1048576] [--out profiles/strain_time.json]
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

from gpu_util import renderer_for

REPS = 5
MMAC_PER_ROW = 0.46


def interleaved_ms(fns, reps=REPS):
    """Median milliseconds of each of ``fns`` (name -> callable): one warm-up each, then ``reps`` rounds, every round running each
    candidate once, so that clock and cache drift fall on all of them alike."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            out[k].append(a.elapsed_time(b))
    return {k: statistics.median(v) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, nargs="+", default=[2630, 4096, 4097, 65536, 1048576])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "strain_time.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    r = renderer_for(11, "trained", True)
    eng = r.engine
    result = {"weights": "weightgen.make_state(11, 'trained', True)", "reps": REPS, "mmac_per_mlp_row": MMAC_PER_ROW, "sizes": [], "mesh": None}
    with torch.cuda.device(r.device), torch.no_grad():
        weff, packed = r._weights()
        weff = weff.detach()
        for M in args.points:
            rng = np.random.default_rng(111)
            x = torch.from_numpy(rng.uniform(-0.8, 0.8, size=(M, 3)).astype(np.float32)).to(r.device)
            t, t2 = (torch.from_numpy(rng.uniform(size=(M,)).astype(np.float32)).to(r.device) for _ in range(2))
            n = torch.from_numpy(rng.normal(size=(M, 3)).astype(np.float32)).to(r.device)
            ms = interleaved_ms({"one_launch": lambda: eng.deform_jacobian(eng.points(x=x, t=t), weff, packed),
                                 "three_launches": lambda: r.model.get_deform_grad_from_observed_space(x, t)})
            ja, jb = eng.deform_jacobian(eng.points(x=x, t=t), weff, packed), eng.deform_jacobian(eng.points(x=x, t=t2), weff, packed)
            diff = float((ja - r.model.get_deform_grad_from_observed_space(x, t)).abs().max())
            sm = interleaved_ms({"with_normals": lambda: eng.strain_rows(ja, jb, n), "without": lambda: eng.strain_rows(ja, jb)})
            row = {"M": M, "jacobian_ms": ms["one_launch"], "three_launch_ms": ms["three_launches"],
                   "speedup": ms["three_launches"] / ms["one_launch"], "max_abs_difference": diff,
                   "jacobian_mmac_per_s": 4 * M * MMAC_PER_ROW / (ms["one_launch"] * 1e-3),
                   "strain_rows_ms": sm["with_normals"], "strain_rows_without_normals_ms": sm["without"]}
            result["sizes"].append(row)
            print(json.dumps(row), flush=True)
        mesh = r.extract_observation_mesh(0.3, [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0], 24)
        times = [0.3, 0.31, 0.32, 0.9]
        track = r.track_mesh(mesh, t=0.3, times=times)
        ms = interleaved_ms({"mesh_strain": lambda: r.mesh_strain(track, times), "canonical": lambda: r.mesh_strain(track, times, "canonical")})
        out = r.mesh_strain(track, times)
        last = out["valid"][-1]
        result["mesh"] = {"vertices": int(mesh["vertices"].shape[0]), "triangles": int(mesh["triangles"].shape[0]), "times": times,
                          "mesh_strain_ms": ms["mesh_strain"], "mesh_strain_canonical_ms": ms["canonical"],
                          "valid": int(out["valid"].sum()), "rows": int(out["valid"].numel()),
                          "area_ratio_last_frame_min_max": [float(out["area"][-1][last].min()), float(out["area"][-1][last].max())],
                          "stretch_last_frame_min_max": [float(out["stretch"][-1][last].min()), float(out["stretch"][-1][last].max())]}
        print(json.dumps(result["mesh"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            json.dump(result, fo, indent=1)


if __name__ == "__main__":
    main()
