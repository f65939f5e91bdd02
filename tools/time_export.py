#!/usr/bin/env python3
"""Time the mesh export on the GPU box (csrc/export.hip, the clean-up of csrc/mesh.hip), per resolution, on the trained golden case's
extracted mesh: Engine.mesh_clean, Engine.vertex_normals, Engine.cluster_vertices with one lattice cell (what ``simplify="grid"``
runs, with six attribute channels) and Engine.ply_pack with colours and normals plus its copy to the host -- each next to its numpy
twin on the host (meshing.mesh_clean / vertex_normals / cluster_vertices, data.ply_body), and the triangle counts before and after
the clustering.  Events on the launch stream (host clock for the twins and for the copy), one warm-up, median of 5; the twins once.

    python tools/time_export.py [--res 256] [--out profiles/export_time.json]
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

from endosurf_amd import data, meshing
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


def host_ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t0), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[256])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    r = renderer_for_case(load_case("trained_deform"))
    eng = r.engine
    bmin, bmax, t = [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0], torch.tensor([0.37])
    rows = []
    with torch.cuda.device(r.device):
        for R in args.res:
            v, f = r._mesh_on_device(t, bmin, bmax, R, 0.0, 1 << 22)
            vn_, fn_ = v.cpu().numpy(), f.cpu().numpy()
            cell, origin = r._simplify_arg("grid", bmin, bmax, R)
            row = {"R": R, "reps": REPS, "V": v.shape[0], "T": f.shape[0], "cell": cell}
            row["clean_ms"] = median_ms(lambda: eng.mesh_clean(v, f, compact=True))
            row["clean_twin_ms"], tw = host_ms(lambda: meshing.mesh_clean(vn_, fn_, compact=True))
            cv, cf, _, st = eng.mesh_clean(v, f, compact=True)
            row["clean_equal"] = bool(np.array_equal(cf.cpu().numpy(), tw[1]) and st == tw[3])
            row.update({f"clean_{k}": x for k, x in st.items()})
            row["normals_ms"] = median_ms(lambda: eng.vertex_normals(v, f))
            row["normals_twin_ms"], tw = host_ms(lambda: meshing.vertex_normals(vn_, fn_))
            normals = eng.vertex_normals(v, f)
            row["normals_equal"] = bool(np.array_equal(normals.cpu().numpy(), tw))
            att = torch.cat([normals, torch.rand(v.shape[0], 3, device=v.device)], -1)
            row["cluster_ms"] = median_ms(lambda: eng.cluster_vertices(v, f, cell, origin, att))
            row["cluster_twin_ms"], tw = host_ms(lambda: meshing.cluster_vertices(vn_, fn_, cell, origin, att.cpu().numpy()))
            sv, sf, sa, _, sst = eng.cluster_vertices(v, f, cell, origin, att)
            row["cluster_equal"] = bool(np.array_equal(sv.cpu().numpy(), tw[0]) and np.array_equal(sf.cpu().numpy(), tw[1])
                                        and np.array_equal(sa.cpu().numpy(), tw[2]) and sst == tw[4])
            row.update({f"cluster_{k}": x for k, x in sst.items()}, triangles_before=f.shape[0], triangles_after=sf.shape[0])
            colors = att[:, 3:].contiguous()
            row["ply_pack_ms"] = median_ms(lambda: eng.ply_pack(v, f, colors, normals))
            body = eng.ply_pack(v, f, colors, normals)
            torch.cuda.synchronize()
            row["ply_copy_ms"], host_body = host_ms(lambda: body.cpu().numpy())
            row["ply_twin_ms"], tw = host_ms(lambda: data.ply_body(vn_, fn_, colors.cpu().numpy(), normals.cpu().numpy()))
            row["ply_equal"] = bool(np.array_equal(host_body, tw))
            row["ply_bytes"] = int(body.numel())
            row["ply_bytes_after_simplify"] = int(eng.ply_pack(sv, sf, sa[:, 3:].contiguous(), sa[:, :3].contiguous()).numel())
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            json.dump(rows, fo, indent=1)


if __name__ == "__main__":
    main()
