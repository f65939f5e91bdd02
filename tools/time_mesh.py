#!/usr/bin/env python3
"""Time the mesh clean-up and the geometric error on the GPU box (csrc/mesh.hip), per resolution, on the trained golden case with two
planted floaters (tiny spheres appended to the extracted mesh): connected components (Engine.mesh_components: time and rounds), the
whole filter (Engine.keep_components: components + compaction), and Engine.nearest for one 640 x 512 frame of synthetic depth points
(327 680 points around the kept vertices, in a scan-line-like order) against the kept vertices -- next to a chunked
torch.cdist(...).min on the device and, on a subset of the queries, the numpy twin on the host.  Events on the launch stream (host
clock for the host twin), one warm-up, median of 5.

    python tools/time_mesh.py [--res 128 256 512] [--queries 327680] [--host-queries 512] [--compare-max 256] [--out FILE.json]
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

from endosurf_amd import meshing
from gpu_util import renderer_for_case
from oracle_util import load_case

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


def cdist_min(q, p):
    rows = max(1, (1 << 27) // max(p.shape[0], 1))          # 512 MB of distances per chunk
    d, i = [], []
    for q0 in range(0, q.shape[0], rows):
        m = torch.cdist(q[q0:q0 + rows], p).min(dim=1)
        d.append(m.values)
        i.append(m.indices)
    return torch.cat(d), torch.cat(i)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[128, 256, 512])
    ap.add_argument("--queries", type=int, default=640 * 512)
    ap.add_argument("--host-queries", type=int, default=512, help="queries the numpy twin is timed on (its time is scaled to --queries)")
    ap.add_argument("--compare-max", type=int, default=256, help="largest resolution at which torch.cdist and the host twin are timed")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    r = renderer_for_case(load_case("trained_deform"))
    eng = r.engine
    bmin, bmax, t = [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0], torch.tensor([0.37])
    rows = []
    with torch.cuda.device(r.device):
        tiny_v, tiny_f, _ = eng.iso_surface(torch.from_numpy(np.fromfunction(
            lambda i, j, k: np.sqrt((i - 4.0) ** 2 + (j - 4.0) ** 2 + (k - 4.0) ** 2) - 2.7, (9, 9, 9)).astype(np.float32)).cuda(), 0.0)
        for R in args.res:
            v, f = r._mesh_on_device(t, bmin, bmax, R, 0.0, 1 << 22)
            n0 = v.shape[0]
            for c in ((0.9, 0.9, 0.9), (-0.9, 0.85, -0.9)):          # two floaters in the corners of the box
                f = torch.cat([f, tiny_f + v.shape[0]])
                v = torch.cat([v, tiny_v * 0.004 + torch.tensor(c, device=v.device)])
            row = {"R": R, "reps": REPS, "V": v.shape[0], "T": f.shape[0]}
            row["components_ms"] = median_ms(lambda: eng.mesh_components(f, v.shape[0]))
            row["filter_ms"] = median_ms(lambda: eng.keep_components(v, f, 0.9))
            kv, kf, vmap, st = eng.keep_components(v, f, 0.9)
            row.update(st, kept_vertices=kv.shape[0], floaters_removed=bool(kv.shape[0] <= n0))
            # one frame of depth points: vertices picked along the vertex order (scan-line like), moved by a few cells
            g = torch.Generator(device=v.device).manual_seed(R)
            pick = torch.linspace(0, kv.shape[0] - 1, args.queries, device=v.device).long()
            q = kv[pick] + torch.randn(args.queries, 3, device=v.device, generator=g) * (4.0 / R)
            row["queries"] = args.queries
            row["nearest_ms"] = median_ms(lambda: eng.nearest(q, kv))
            d, i = eng.nearest(q, kv)
            row["geometric_error"] = float(d.double().mean())
            if R > args.compare_max:
                rows.append(row)
                print(json.dumps(row), flush=True)
                continue
            row["cdist_min_ms"] = median_ms(lambda: cdist_min(q, kv), reps=3)
            cd, ci = cdist_min(q, kv)
            row["cdist_max_abs_diff"] = float((cd - d).abs().max())
            nq = min(args.host_queries, args.queries)
            qn, pn = q[:nq].cpu().numpy(), kv.cpu().numpy()
            t0 = time.perf_counter()
            hd, hi = meshing.nearest(qn, pn)
            row["host_twin_ms_scaled"] = 1e3 * (time.perf_counter() - t0) * args.queries / nq
            row["host_twin_index_equal"] = float((hi == i[:nq].cpu().numpy()).mean())
            row["host_twin_max_rel_diff"] = float(np.max(np.abs(hd - d[:nq].cpu().numpy()) / np.maximum(hd, 1e-30)))
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            json.dump(rows, fo, indent=1)


if __name__ == "__main__":
    main()
