#!/usr/bin/env python3
"""Time the curvature kernels on the GPU box (csrc/sdf_hess.hip, csrc/curvature.hip) on the seed-11 ``trained`` weights: es_sdf_hessian
-- value, gradient and Hessian of the SDF network in one launch, 10 MLP rows per point -- on both tile heights, against the route there
was before: three Hessian-vector products, each a saving point forward, a full point backward (weight-gradient GEMMs included) and
``Engine.point_input_adjoint``, on the same canonical points (uniform in [-0.8, 0.8]^3) at M = 1 024, 2 630, 65 536 and 1 048 576;
es_curvature_rows at the same sizes; both tile heights at nine sizes around the tile-height threshold (median of 9); and ``renderer.mesh_curvature`` on the 2 630-vertex mesh of DESIGN.md 7h (24^3 lattice at
t = 0.3) tracked through t, t + 0.01, t + 0.02, 0.9.  Events on the launch stream, one warm-up each, the candidates interleaved
repetition by repetition, median of 5.  Numbers are recorded, not gated.

    python tools/time_curvature.py [--points 1024 2630 65536 1048576] [--out profiles/curvature_time.json]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))
import numpy as np
import torch

from gpu_util import renderer_for
from time_strain import MMAC_PER_ROW, REPS, interleaved_ms

HVP_CHUNK = 131072          # points per Hessian-vector product: the saving forward keeps ~103 KB per point


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, nargs="+", default=[1024, 2630, 65536, 1048576])
    ap.add_argument("--tile-sweep", type=int, nargs="*", default=[128, 256, 512, 768, 1024, 1280, 1536, 1638, 2048],
                    help="sizes around the tile-height threshold, both heights, median of 9")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "curvature_time.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    from endosurf_amd import _lib
    r = renderer_for(11, "trained", True)
    eng = r.engine
    result = {"weights": "weightgen.make_state(11, 'trained', True)", "reps": REPS, "mmac_per_mlp_row": MMAC_PER_ROW, "hvp_chunk": HVP_CHUNK,
              "sizes": [], "mesh": None}
    with torch.cuda.device(r.device), torch.no_grad():
        weff, packed = r._weights()
        weff = weff.detach()
        eye = torch.eye(3, device=r.device)

        def three_hvps(x, t):
            """H by the route of the parent commit: per unit direction a saving forward of the SDF network (no deformation: canonical
            points), the full backward and the point adjoint, in chunks that fit the workspace."""
            cols = []
            for j in range(3):
                parts = []
                for i in range(0, x.shape[0], HVP_CHUNK):
                    xs = x[i:i + HVP_CHUNK]
                    w = eye[j][None].expand(xs.shape[0], 3).contiguous()
                    ctx = eng.point_forward(eng.points(x=xs, t=t[i:i + HVP_CHUNK]), weff, packed, _lib.PF_SAVE, fp32_only=True)
                    eng.point_backward(ctx, weff, packed, None, w)
                    parts.append(eng.point_input_adjoint(ctx, weff, packed, None, w))
                cols.append(torch.cat(parts))
            return torch.stack(cols, -1)

        for M in args.points:
            rng = np.random.default_rng(111)
            x = torch.from_numpy(rng.uniform(-0.8, 0.8, size=(M, 3)).astype(np.float32)).to(r.device)
            t = torch.from_numpy(rng.uniform(size=(M,)).astype(np.float32)).to(r.device)
            ms = interleaved_ms({"tile32": lambda: eng.sdf_hessian(x, weff, packed, tile_rows=32),
                                 "tile64": lambda: eng.sdf_hessian(x, weff, packed, tile_rows=64),
                                 "chosen": lambda: eng.sdf_hessian(x, weff, packed),
                                 "three_hvps": lambda: three_hvps(x, t)})
            _, g, H = eng.sdf_hessian(x, weff, packed)
            diff = float((H - three_hvps(x, t)).abs().max())
            jac = eng.deform_jacobian(eng.points(x=x, t=t), weff, packed)
            rm = interleaved_ms({"composed": lambda: eng.curvature_rows(g, H, jac, g), "plain": lambda: eng.curvature_rows(g, H)})
            row = {"M": M, "hessian_tile32_ms": ms["tile32"], "hessian_tile64_ms": ms["tile64"], "hessian_ms": ms["chosen"],
                   "three_hvp_ms": ms["three_hvps"], "speedup": ms["three_hvps"] / ms["chosen"], "max_abs_difference": diff,
                   "max_abs_hessian": float(H.abs().max()), "hessian_mmac_per_s": 10 * M * MMAC_PER_ROW / (ms["chosen"] * 1e-3),
                   "curvature_rows_ms": rm["composed"], "curvature_rows_without_jac_ms": rm["plain"]}
            result["sizes"].append(row)
            print(json.dumps(row), flush=True)
            del x, t, g, H, jac
            torch.cuda.empty_cache()
        result["tile_sweep"] = []
        for M in args.tile_sweep:
            x = torch.from_numpy(np.random.default_rng(111).uniform(-0.8, 0.8, size=(M, 3)).astype(np.float32)).to(r.device)
            ms = interleaved_ms({"tile32": lambda: eng.sdf_hessian(x, weff, packed, tile_rows=32),
                                 "tile64": lambda: eng.sdf_hessian(x, weff, packed, tile_rows=64)}, reps=9)
            result["tile_sweep"].append({"M": M, "hessian_tile32_ms": ms["tile32"], "hessian_tile64_ms": ms["tile64"]})
            print(json.dumps(result["tile_sweep"][-1]), flush=True)
        mesh = r.extract_observation_mesh(0.3, [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0], 24)
        times = [0.3, 0.31, 0.32, 0.9]
        track = r.track_mesh(mesh, t=0.3, times=times)
        ms = interleaved_ms({"mesh_curvature": lambda: r.mesh_curvature(track, times=times), "one_frame": lambda: r.mesh_curvature(mesh, t=0.3)})
        out = r.mesh_curvature(track, times=times)
        first = out["valid"][0]
        result["mesh"] = {"vertices": int(mesh["vertices"].shape[0]), "triangles": int(mesh["triangles"].shape[0]), "times": times,
                          "mesh_curvature_ms": ms["mesh_curvature"], "mesh_curvature_one_frame_ms": ms["one_frame"],
                          "valid": int(out["valid"].sum()), "rows": int(out["valid"].numel()),
                          "mean_first_frame_min_max": [float(out["mean"][0][first].min()), float(out["mean"][0][first].max())],
                          "gauss_first_frame_min_max": [float(out["gauss"][0][first].min()), float(out["gauss"][0][first].max())]}
        print(json.dumps(result["mesh"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            json.dump(result, fo, indent=1)


if __name__ == "__main__":
    main()
