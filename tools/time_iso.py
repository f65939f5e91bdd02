#!/usr/bin/env python3
"""Time a mesh extraction stage by stage on the GPU box, on the trained golden case: field sampling (the SDF query over the grid),
the on-device iso-surface (Engine.iso_surface: classify + scans, the read of the two counts, emit) and, next to it, today's host step
(the device-to-host copy of the field + meshing.marching_tetrahedra).  Events on the launch stream, one warm-up, median of 5.
``--band`` adds the narrow-band path (Engine.band_field, csrc/band.hip): the field assembled from queries near the surface only
(band_field_ms), field + iso-surface (band_total_ms, next to dense_total_ms), its counts, and whether the mesh is the dense one.
``--cubes`` adds the cube triangulation (Engine.iso_surface(method="cubes"), csrc/cubes.hip) beside the tetrahedra one, timed the same
way (cubes_iso_ms, cubes_V, cubes_T), and what the smaller mesh saves behind the extractor: the vertex attributes of
extract_observation_mesh (renderonpts' colours and normals + the SDF at the vertices: attrs_ms / cubes_attrs_ms) and, up to
``--host-max``, the bytes of export_observation_mesh's three PLY files (ply_bytes / cubes_ply_bytes).

    python tools/time_iso.py [--res 128 256 512] [--host-max 256] [--band] [--cubes] [--block 8] [--lipschitz 1.0] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import torch

from endosurf_amd.meshing import marching_tetrahedra
from gpu_util import renderer_for_case
from oracle_util import load_case


def median_ms(fn, reps=5):
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
    ap.add_argument("--res", type=int, nargs="+", default=[128, 256, 512])
    ap.add_argument("--host-max", type=int, default=256, help="largest resolution at which the host extractor is timed")
    ap.add_argument("--band", action="store_true", help="also time the narrow-band extraction and compare its mesh with the dense one")
    ap.add_argument("--cubes", action="store_true", help="also time the cube triangulation, and the vertex attributes and PLY sizes of both methods")
    ap.add_argument("--block", type=int, default=8)
    ap.add_argument("--lipschitz", type=float, default=1.0)
    ap.add_argument("--out", default=None, help="also write the rows to this JSON file (one JSON line per resolution is always printed)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    r = renderer_for_case(load_case("trained_deform"))
    bmin, bmax, t = [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0], torch.tensor([0.37])
    rows = []
    view = torch.tensor([0.1, -0.2, -1.5])

    def attributes(verts, R):          # what extract_observation_mesh evaluates at the vertices of a mesh (index coordinates in)
        x = verts / (R - 1.0) * 2.0 - 1.0
        dirs = x - view.to(x.device)[None]
        dirs = dirs / torch.linalg.norm(dirs, ord=2, dim=-1, keepdim=True)
        tt = t.to(x.device)
        r.renderonpts(x, dirs, tt, net_chunk=1 << 17, cpu=False)
        with torch.no_grad():
            for i in range(0, x.shape[0], 1 << 17):
                r._point_eval(x[i:i + (1 << 17)], tt)

    with torch.cuda.device(r.device):
        for R in args.res:
            row = {"R": R, "field_ms": median_ms(lambda: r._field_on_device(bmin, bmax, R, t))}
            u = r._field_on_device(bmin, bmax, R, t)
            row["iso_ms"] = median_ms(lambda: r.engine.iso_surface(u, 0.0))
            v, f, _ = r.engine.iso_surface(u, 0.0)
            row["V"], row["T"] = v.shape[0], f.shape[0]
            if R <= args.host_max:
                host = []
                for _ in range(3):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    un = u.cpu().numpy()
                    t1 = time.perf_counter()
                    marching_tetrahedra(un, 0.0)
                    host.append((time.perf_counter() - t0, t1 - t0))
                row["host_copy_ms"] = 1e3 * statistics.median(h[1] for h in host)
                row["host_total_ms"] = 1e3 * statistics.median(h[0] for h in host)
            if args.cubes:
                row["cubes_iso_ms"] = median_ms(lambda: r.engine.iso_surface(u, 0.0, "cubes"))
                cv, cf, _ = r.engine.iso_surface(u, 0.0, "cubes")
                row["cubes_V"], row["cubes_T"] = cv.shape[0], cf.shape[0]
                row["attrs_ms"] = median_ms(lambda: attributes(v, R))
                row["cubes_attrs_ms"] = median_ms(lambda: attributes(cv, R))
                if R <= args.host_max:
                    with tempfile.TemporaryDirectory() as tmp:
                        for key, method in (("ply_bytes", "tetrahedra"), ("cubes_ply_bytes", "cubes")):
                            m = r.export_observation_mesh(os.path.join(tmp, method), t, bmin, bmax, R, view_point=view, components=None, method=method)
                            row[key] = sum(os.path.getsize(q) for q in m["paths"].values())
                            del m
                del cv, cf
            if args.band:
                band = dict(block=args.block, lipschitz=args.lipschitz)
                field = lambda: r._band_field_on_device(bmin, bmax, R, t, 0.0, 1 << 22, band)
                row["band_field_ms"] = median_ms(field)
                row["band_total_ms"] = median_ms(lambda: r.engine.iso_surface(field()[0], 0.0))
                row["dense_total_ms"] = median_ms(lambda: r.engine.iso_surface(r._field_on_device(bmin, bmax, R, t), 0.0))
                ub, stats = field()
                bv, bf, _ = r.engine.iso_surface(ub, 0.0)
                row.update(band, **stats, evaluated_fraction=stats["evaluated_points"] / stats["dense_points"],
                           mesh_equal=bool(torch.equal(bv, v) and torch.equal(bf, f)), speedup_total=row["dense_total_ms"] / row["band_total_ms"])
                del ub, bv, bf
            rows.append(row)
            print(json.dumps(row))
            del u, v, f
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            json.dump(rows, fo, indent=1)


if __name__ == "__main__":
    main()
