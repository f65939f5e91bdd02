#!/usr/bin/env python3
"""Time the depth fusion on the GPU box (csrc/fuse.hip): ``Engine.tsdf_integrate`` alone at 128^3 and 256^3 voxels with 16
frames of 640 x 512 (an analytic sphere seen from 16 poses), beside the same rule written in stock torch ops, a gather per frame, in
fp64; ``fuse_depth`` in canonical space on the seed-11 ``trained`` weights at 64^3 and 128^3 with 4 frames, and the share of it spent in
``to_observed`` (the same solves timed alone); and ``mesh_coverage`` on the 2 630-vertex mesh of DESIGN.md 7h.  Events on the launch
stream, one warm-up, median of 5.  Numbers are recorded, not gated.

    python tools/time_fuse.py [--out profiles/fuse_time.json]
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

import fuse_util as U
from endosurf_amd import flow, fusion
from flow_util import rotated_pose
from gpu_util import renderer_for

REPS = 5
H, W = 512, 640
K = np.array([[800.0, 0.0, 319.5], [0.0, 800.0, 255.5], [0.0, 0.0, 1.0]])
FRAMES = 16
BOUNDS = ((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5))
CANONICAL_TIMES = [0.2, 0.4, 0.6, 0.8]


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


def poses(n):
    P = np.stack([rotated_pose(0.0731 * np.cos(1.7 * k), 0.0417 + 0.011 * k) for k in range(n)])
    P[:, 1, 3] = 0.0171 - 0.004 * np.arange(n)
    return P


def torch_integrate(state, pts, depth, cams, trunc):
    """``fusion.integrate`` (one lattice, no colour, no mask) in stock torch ops on the device: fp64, one gather per frame."""
    ts, wt = state
    x = pts.double()
    Hh, Ww = depth.shape[1:]
    for f in range(depth.shape[0]):
        c = cams[f]
        d = [x[:, k] - c[9 + k] for k in range(3)]
        q = [(c[k] * d[0] + c[3 + k] * d[1]) + c[6 + k] * d[2] for k in range(3)]
        z = q[2]
        u = (c[12] * q[0] + c[13] * q[1]) / z + c[14]
        v = c[15] * q[1] / z + c[16]
        fj, fi = torch.floor(u + 0.5), torch.floor(v + 0.5)
        ok = (z > 0) & (fj >= 0) & (fj <= Ww - 1) & (fi >= 0) & (fi <= Hh - 1)
        pix = torch.where(ok, fi * Ww + fj, torch.zeros_like(fj)).long()
        dd = depth[f].reshape(-1)[pix]
        s = dd.double() - z
        ok &= torch.isfinite(dd) & (dd > 0) & ~(s < -trunc)
        term = torch.clamp(s / trunc, max=1.0).float()
        ts += torch.where(ok, term, torch.zeros_like(term))
        wt += ok.float()
    return ts, wt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "fuse_time.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    r = renderer_for(11, "trained", True)
    eng = r.engine
    result = {"weights": "weightgen.make_state(11, 'trained', True)", "reps": REPS, "integrate": [], "canonical": []}
    with torch.cuda.device(r.device), torch.no_grad():
        P = poses(FRAMES)
        depth = torch.from_numpy(np.stack([U.sphere_depth(K, p, H, W) for p in P])).to(r.device)
        color = torch.rand(FRAMES, H, W, 3, device=r.device)
        table = flow.camera_table(K, P)[0]
        cams = eng.flow_cameras(table)
        for R in (128, 256):
            pts = fusion.lattice_points(fusion.lattice_axes(*BOUNDS, R, r.device))
            N = pts.shape[0]
            trunc = fusion.default_trunc(*BOUNDS, R)
            bare, full = eng.tsdf_state(N, False), eng.tsdf_state(N, True)
            stock = (torch.zeros(N, device=r.device), torch.zeros(N, device=r.device))
            row = {"resolution": R, "voxels": N, "frames": FRAMES, "height": H, "width": W, "gathers": N * FRAMES,
                   "integrate_ms": median_ms(lambda: eng.tsdf_integrate(bare, pts, depth, cams, trunc=trunc)),
                   "integrate_color_ms": median_ms(lambda: eng.tsdf_integrate(full, pts, depth, cams, color, trunc=trunc)),
                   "torch_fp64_ms": median_ms(lambda: torch_integrate(stock, pts, depth, cams, trunc)),
                   "finalize_ms": median_ms(lambda: eng.tsdf_finalize(full))}
            row["gathers_per_s"] = row["gathers"] / (row["integrate_ms"] * 1e-3)
            # the six calls (one warm-up, five timed) of each state added the same frames: weights agree voxel by voxel
            row["torch_weight_differs_on"] = int((stock[1] != bare["weight"]).sum())
            row["observed_share"] = float((bare["weight"] > 0).float().mean())
            result["integrate"].append(row)
            print(json.dumps(row), flush=True)
            del pts, bare, full, stock
        Pc = P[:len(CANONICAL_TIMES)]
        dc, cc = depth[:len(CANONICAL_TIMES)].contiguous(), color[:len(CANONICAL_TIMES)].contiguous()
        tt = torch.tensor(CANONICAL_TIMES, device=r.device)
        for R in (64, 128):
            N = R ** 3
            fuse = lambda: r.fuse_depth(dc, K, Pc, CANONICAL_TIMES, *BOUNDS, R, colors=cc)
            axes = fusion.lattice_axes(*BOUNDS, R, r.device)

            def solves():
                for n0 in range(0, N, 1 << 18):
                    pts = fusion.lattice_points(axes, n0, n0 + (1 << 18))
                    r.to_observed(pts.repeat(len(CANONICAL_TIMES), 1), tt.repeat_interleave(pts.shape[0]))

            vol = fuse()
            ob = r.to_observed(fusion.lattice_points(axes, 0, 1 << 18).repeat(len(CANONICAL_TIMES), 1),
                               tt.repeat_interleave(min(N, 1 << 18)))
            row = {"resolution": R, "voxels": N, "frames": len(CANONICAL_TIMES), "solves": N * len(CANONICAL_TIMES), "fuse_depth_ms": median_ms(fuse),
                   "to_observed_ms": median_ms(solves), "static_ms": median_ms(lambda: r.fuse_depth(dc, K, Pc, CANONICAL_TIMES, *BOUNDS, R, colors=cc, space="static")),
                   "observed_share": float((vol["weight"] > 0).float().mean()), "converged_share_first_chunk": float(ob["converged"].float().mean()),
                   "iters_per_row_first_chunk": float(ob["iters"].float().mean())}
            row["to_observed_share"] = row["to_observed_ms"] / row["fuse_depth_ms"]
            result["canonical"].append(row)
            print(json.dumps(row), flush=True)
        mesh = r.extract_observation_mesh(0.3, [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0], 24)
        track = r.track_mesh(mesh, t=0.3, times=[0.3, 0.31, 0.32, 0.9])
        cov = r.mesh_coverage(mesh, vol, t=0.3)
        result["mesh_coverage"] = {"vertices": int(mesh["vertices"].shape[0]), "volume_resolution": 128,
                                   "from_vertices_ms": median_ms(lambda: r.mesh_coverage(mesh, vol, t=0.3)),
                                   "from_track_ms": median_ms(lambda: r.mesh_coverage(track, vol)),
                                   "inside": int(cov["inside"].sum()), "covered": int((cov["coverage"] >= 1.0).sum())}
        print(json.dumps(result["mesh_coverage"]), flush=True)
        fm = r.fused_mesh(vol)
        result["fused_mesh"] = {"volume_resolution": 128, "ms": median_ms(lambda: r.fused_mesh(vol)), "vertices": int(fm["vertices"].shape[0]),
                                "triangles": int(fm["triangles"].shape[0])}
        print(json.dumps(result["fused_mesh"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
