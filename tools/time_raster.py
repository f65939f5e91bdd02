#!/usr/bin/env python3
"""Time the mesh rasteriser on the GPU box (csrc/raster.hip), stage by stage, on the trained golden case: the mesh extracted at each
resolution (narrow band, largest component) drawn to a 640 x 512 image from a camera in front of the scene with six attributes per
vertex (colours and normals) -- projection, counting (set-up, scan, clearing the keys), filling, resolving, the whole
Engine.rasterize (with its two read-backs) and EndoSurfRenderer.render_mesh (rasterise once, shade three times) -- plus one
screen-filling two-triangle quad.  Events on the launch stream, one warm-up, median of 5.

    python tools/time_raster.py [--res 128 256 512] [--size 512 640] [--out FILE.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import torch

from endosurf_amd.meshing import camera_params
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


def stages(eng, verts, tris, attrs, K, pose, H, W):
    """Per-stage times of one image through the C ABI, on buffers allocated once."""
    lib, st = eng.lib, eng.st()
    p = lambda t: C.c_void_p(t.data_ptr())
    V, T, Cn = verts.shape[0], tris.shape[0], attrs.shape[1]
    cam = (C.c_double * 17)(*camera_params(K, pose).tolist())
    xy, zc = eng.empty(V, 2, dtype=torch.int32), eng.empty(V)
    scratch = eng.empty(int(lib.es_rast_scratch_bytes(V, T, H, W)), dtype=torch.uint8)
    totals = eng.empty(8, dtype=torch.int64)
    depth, tri, bary, out = eng.empty(H, W), eng.empty(H, W, dtype=torch.int32), eng.empty(H, W, 3), eng.empty(H, W, Cn)
    view = (H, W, 1e-6, 0, p(scratch))

    def ok(status):
        assert status == 0, lib.es_last_error()

    row = {"project_ms": median_ms(lambda: ok(lib.es_rast_project(p(verts), V, cam, p(xy), p(zc), st)))}
    row["count_ms"] = median_ms(lambda: ok(lib.es_rast_count(p(tris), V, T, p(xy), p(zc), *view, p(totals), st)))
    n_work = int(totals[0])

    def count_and_fill():          # (a fill on keys that already hold the picture skips its atomics: time it behind a clearing count)
        ok(lib.es_rast_count(p(tris), V, T, p(xy), p(zc), *view, p(totals), st))
        ok(lib.es_rast_fill(p(tris), V, T, p(xy), p(zc), *view, n_work, st))

    row["fill_ms"] = median_ms(count_and_fill) - row["count_ms"]
    row["resolve_ms"] = median_ms(lambda: ok(lib.es_rast_resolve(p(tris), V, T, p(xy), p(zc), p(attrs), Cn, H, W, 1e-6, 0, p(scratch), p(depth), p(tri),
                                                                 p(bary), p(out), p(totals), st)))
    row["kernels_ms"] = row["project_ms"] + row["count_ms"] + row["fill_ms"] + row["resolve_ms"]
    tt = totals.tolist()
    row.update(work_items=n_work, covered_pixels=int(tt[6]), offscreen=int(tt[5]), zero_area=int(tt[3]))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[128, 256, 512])
    ap.add_argument("--size", type=int, nargs=2, default=[512, 640], metavar=("H", "W"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    r = renderer_for_case(load_case("trained_deform"))
    eng = r.engine
    H, W = args.size
    bmin, bmax, t, view = [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0], torch.tensor([0.37]), [0.0, 0.0, -1.5]
    K = torch.tensor([[0.8 * W, 0, (W - 1) / 2.0, 0], [0, 0.8 * W, (H - 1) / 2.0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    pose = torch.eye(4)
    pose[:3, 3] = torch.tensor(view)
    rows = []
    with torch.cuda.device(r.device):
        for R in args.res:
            mesh = r.extract_observation_mesh(t, bmin, bmax, R, view_point=view, band=True, components=0.9)
            v, f = mesh["vertices"], mesh["triangles"]
            attrs = torch.cat([mesh["colors"], mesh["normals"]], -1).contiguous()
            row = {"case": "trained_deform", "R": R, "height": H, "width": W, "reps": REPS, "V": v.shape[0], "T": f.shape[0], "attributes": 6}
            row.update(stages(eng, v, f, attrs, K, pose, H, W))
            row["rasterize_ms"] = median_ms(lambda: eng.rasterize(v, f, K, pose, H, W, attributes=attrs))
            row["render_mesh_ms"] = median_ms(lambda: r.render_mesh(mesh, K, pose, H, W, view_point=view))
            rows.append(row)
            print(json.dumps(row), flush=True)
        quad = torch.tensor([[-9.0, -9, 1], [9, -9, 1.5], [9, 9, 2], [-9, 9, 1.5]], device=r.device)
        qf = torch.tensor([[0, 2, 1], [0, 3, 2]], dtype=torch.int32, device=r.device)
        qa = torch.cat([quad, quad], -1).contiguous()
        row = {"case": "screen-filling quad", "height": H, "width": W, "reps": REPS, "V": 4, "T": 2, "attributes": 6}
        row.update(stages(eng, quad, qf, qa, K, torch.eye(4), H, W))
        row["rasterize_ms"] = median_ms(lambda: eng.rasterize(quad, qf, K, torch.eye(4), H, W, attributes=qa))
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            json.dump(rows, fo, indent=1)


if __name__ == "__main__":
    main()
