#!/usr/bin/env python3
"""Time the point-to-surface distance on the GPU box (csrc/surface.hip), per resolution, on the trained golden case: the mesh of
EndoSurfRenderer.extract_observation_mesh after the component filter, and the same after ``simplify="grid"``.  Queries: one 640 x 512
frame of synthetic depth points (327 680 points around the filtered mesh's vertices, in a scan-line-like order; the same cloud for
both meshes, made as tools/time_mesh.py makes it).  Reported per mesh: es_surf_build (centroids, radii and the grid) and, timed on its
own over the same centroids, es_nn_build (the grid alone; the prepare kernel is the difference), es_surf_query, the whole
Engine.point_to_mesh, Engine.nearest on the same queries for scale, the mean number of cell shells read and of triangles measured per
query, and both metrics (mean distance to the nearest vertex, mean distance to the surface).  Events on the launch stream, one warm-up,
median of 5.

    python tools/time_surface.py [--res 128 256] [--queries 327680] [--out FILE.json]
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

from endosurf_amd._lib import check, ptr
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


def measure(eng, name, R, v, f, q):
    lib, st = eng.lib, eng.st()
    V, T, Q = v.shape[0], f.shape[0], q.shape[0]
    f32 = f.to(torch.int32).contiguous()
    scratch = eng._scratch("es_surf_scratch_bytes", V, T)
    nn_scratch = eng._scratch("es_nn_scratch_bytes", T)
    cent = v[f32.long()].double().mean(1).float().contiguous()
    dist, tri, closest = eng.empty(Q), eng.empty(Q, dtype=torch.int32), eng.empty(Q, 3)
    row = {"R": R, "mesh": name, "reps": REPS, "V": V, "T": T, "queries": Q}
    row["build_ms"] = median_ms(lambda: check(lib.es_surf_build(ptr(v), ptr(f32), V, T, ptr(scratch), st), "es_surf_build"))
    row["grid_ms"] = median_ms(lambda: check(lib.es_nn_build(ptr(cent), T, ptr(nn_scratch), st), "es_nn_build"))
    row["prepare_ms_by_difference"] = row["build_ms"] - row["grid_ms"]
    row["query_ms"] = median_ms(lambda: check(lib.es_surf_query(ptr(q), Q, ptr(v), ptr(f32), V, T, ptr(scratch), ptr(dist), ptr(tri),
                                                                ptr(closest), None, st), "es_surf_query"))
    row["point_to_mesh_ms"] = median_ms(lambda: eng.point_to_mesh(q, v, f))
    row["nearest_ms"] = median_ms(lambda: eng.nearest(q, v))
    d, _, _, work = eng.point_to_mesh(q, v, f, return_work=True)
    row["shells_mean"], row["triangles_mean"] = (float(x) for x in work.double().mean(0).tolist())
    row["shells_max"], row["triangles_max"] = (int(x) for x in work.max(0).values.tolist())
    row["surface_error"] = float(d.double().mean())
    row["geometric_error"] = float(eng.nearest(q, v)[0].double().mean())
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--queries", type=int, default=640 * 512)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    r = renderer_for_case(load_case("trained_deform"))
    eng = r.engine
    bmin, bmax, t = [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0], torch.tensor([0.37])
    rows = []
    with torch.cuda.device(r.device):
        for R in args.res:
            kept = r.extract_observation_mesh(t, bmin, bmax, R, components=0.9)
            grid = r.extract_observation_mesh(t, bmin, bmax, R, components=0.9, simplify="grid")
            kv = kept["vertices"]
            # one frame of depth points: vertices picked along the vertex order (scan-line like), moved by a few cells
            g = torch.Generator(device=kv.device).manual_seed(R)
            pick = torch.linspace(0, kv.shape[0] - 1, args.queries, device=kv.device).long()
            q = (kv[pick] + torch.randn(args.queries, 3, device=kv.device, generator=g) * (4.0 / R)).contiguous()
            for name, m in (("filtered", kept), ("filtered, simplify=grid", grid)):
                row = measure(eng, name, R, m["vertices"].contiguous(), m["triangles"], q)
                rows.append(row)
                print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            json.dump(rows, fo, indent=1)


if __name__ == "__main__":
    main()
