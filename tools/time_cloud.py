#!/usr/bin/env python3
"""Time the scene normalisation on the GPU box (csrc/cloud.hip, data.scene_normalization) on a synthetic sequence of the EndoNeRF
format: 63 frames of 640 x 512, a fixed camera (f = 570), a smooth moving surface at depth 60 .. 100, a tool mask over a sixth of
the image and one isolated wrong depth per thousand pixels.  Two densities: ``down_sample`` 0.005 (what the reference keeps, because
its two neighbour searches run on the host) and 1.0 (every pixel).

Per density, on the first frame's cloud and on the merged cloud (the frames' kept points): es_nn_build, es_cloud_self_nearest,
es_cloud_radius_count without a cap and with the outlier filter's cap of 6, at the filter's own radius (20 x the mean neighbour
distance; the uncapped count over the merged cloud at full density, whose balls hold thousands of points each, only with --all) --
events on the launch stream, one warm-up, median of ``reps`` -- and the whole ``data.scene_normalization`` on the host clock,
read-backs included (one warm-up call on two frames, then one timed call).  Beside them scipy's cKDTree on the host (build, query
k = 2, query_ball_point(return_length=True), 16 workers) as the stand-in for Open3D, which this project does not have: on both clouds
at 0.005, on the frame cloud only at 1.0 (the merged cloud of 16.6 M points is left out: the count alone visits 10^10 pairs or more).

    python tools/time_cloud.py [--frames 63] [--all] [--out profiles/cloud_time.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch

from endosurf_amd import data as D
from endosurf_amd._lib import check, ptr

H, W, F = 512, 640, 570.0
NB, FACTOR = 5, 20.0


def sequence(n, dev):
    """depths [n,H,W], intrinsics, poses [n,4,4], masks [n,H,W] on ``dev``, from one seed."""
    g = torch.Generator(device=dev).manual_seed(7)
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    t = torch.arange(n, device=dev, dtype=torch.float32)[:, None, None]
    depth = 80 + 14 * torch.sin(xs / 90 + 0.05 * t) * torch.cos(ys / 70 - 0.03 * t) + 6 * torch.sin((xs + ys) / 40 + 0.1 * t)
    depth = depth + 0.05 * torch.randn(n, H, W, device=dev, generator=g)
    wrong = torch.rand(n, H, W, device=dev, generator=g) < 1e-3
    depth = torch.where(wrong, 30 + 120 * torch.rand(n, H, W, device=dev, generator=g), depth)
    masks = ~((xs > 0.55 * W) & (ys > 0.62 * H)).expand(n, H, W)          # the tool: a corner of the image
    K = torch.tensor([[F, 0, (W - 1) / 2, 0], [0, F, (H - 1) / 2, 0], [0, 0, 1, 0], [0, 0, 0, 1]], device=dev)
    return depth.contiguous(), K.expand(n, 4, 4).contiguous(), torch.eye(4, device=dev).expand(n, 4, 4).contiguous(), masks.float()


def median_ms(fn, reps):
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


def device_row(eng, pts, reps, uncapped):
    lib, st, P = eng.lib, eng.st(), int(pts.shape[0])
    scratch = eng._scratch("es_nn_scratch_bytes", P)
    dist, index, count = eng.empty(P), eng.empty(P, dtype=torch.int32), eng.empty(P, dtype=torch.int32)
    row = {"points": P, "reps": reps}
    row["grid_build_ms"] = median_ms(lambda: check(lib.es_nn_build(ptr(pts), P, ptr(scratch), st), "es_nn_build"), reps)
    row["self_nearest_ms"] = median_ms(lambda: check(lib.es_cloud_self_nearest(ptr(pts), P, ptr(scratch), ptr(dist), ptr(index), st), "es_cloud_self_nearest"), reps)
    fin = torch.isfinite(dist)
    radius = FACTOR * (torch.where(fin, dist, torch.zeros_like(dist)).double().sum() / fin.sum())
    r2 = (radius.float() * radius.float()).reshape(1)
    for name, cap in (("radius_count_ms", 0), ("radius_count_cap6_ms", NB + 1))[0 if uncapped else 1:]:
        row[name] = median_ms(lambda: check(lib.es_cloud_radius_count(ptr(pts), P, P, ptr(scratch), ptr(r2), cap, ptr(count), st), "es_cloud_radius_count"), reps)
        if cap == 0:
            row["neighbours_mean"], row["neighbours_max"] = float(count.double().mean()), int(count.max())
    row["radius"], row["kept"] = float(radius), int((count > NB).sum())
    return row


def host_row(pts):
    from scipy.spatial import cKDTree
    p = pts.cpu().numpy().astype(np.float64)
    row = {"points": len(p), "workers": 16}
    t0 = time.perf_counter()
    tree = cKDTree(p)
    t1 = time.perf_counter()
    d = tree.query(p, k=2, workers=16)[0][:, 1]
    t2 = time.perf_counter()
    n = tree.query_ball_point(p, FACTOR * d.mean(), return_length=True, workers=16)
    t3 = time.perf_counter()
    row.update(ckdtree_build_ms=1e3 * (t1 - t0), ckdtree_query_k2_ms=1e3 * (t2 - t1), ckdtree_ball_count_ms=1e3 * (t3 - t2), kept=int((n > NB).sum()))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=63)
    ap.add_argument("--all", action="store_true", help="also the uncapped count over the merged cloud at full density (slow)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cloud_time.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    from endosurf_amd.engine import Engine
    dev = torch.device("cuda", torch.cuda.current_device())
    eng = Engine(dev)
    depths, K, poses, masks = sequence(args.frames, dev)
    u = torch.rand(depths.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(8))
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    with torch.cuda.device(dev):
        for ratio in (0.005, 1.0):
            kw = dict(masks=masks, down_sample=ratio, u=u, nb_points=NB, radius_factor=FACTOR, engine=eng)
            D.scene_normalization(depths[:2], K[:2], poses[:2], **{**kw, "masks": masks[:2], "u": u[:2]})          # warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = D.scene_normalization(depths, K, poses, **kw)
            torch.cuda.synchronize()
            c = out["counts"]
            emit({"what": "scene_normalization", "down_sample": ratio, "frames": args.frames, "wall_ms": 1e3 * (time.perf_counter() - t0),
                  "valid": sum(c["valid"]), "sampled": sum(c["sampled"]), "kept": sum(c["kept"]), "merged": c["merged"],
                  "depth_norm_scale": out["depth_norm_scale"]})
            d0 = depths[0] * masks[0]          # the first frame's cloud as its outlier pass sees it: masked, clipped, sampled
            d0 = torch.where((d0 >= out["close_depth"]) & (d0 <= out["inf_depth"]) & ((u[0] < ratio) | (ratio >= 1.0)), d0, torch.zeros_like(d0))
            frame = D.depth_points(d0, K[0], poses[0], out["inf_depth"]).contiguous()
            merged = (out["points"].double() * out["depth_norm_scale"] + out["scale_mat"][:3, 3].double()).float().contiguous()
            for name, pts in (("frame", frame), ("merged", merged)):
                small = ratio < 1.0 or name == "frame"
                emit({"what": "device", "cloud": name, "down_sample": ratio, **device_row(eng, pts, 5 if small else 1, small or args.all)})
                if small:
                    emit({"what": "host cKDTree", "cloud": name, "down_sample": ratio, **host_row(pts)})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fo:
        json.dump(rows, fo, indent=1)


if __name__ == "__main__":
    main()
