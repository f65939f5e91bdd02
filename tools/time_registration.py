#!/usr/bin/env python3
"""Time rigid registration on the GPU box (csrc/register.hip through ``Engine.track_rigid`` and ``Engine.icp``) against its host twin
(``registration``) on the seed-11 ``trained`` weights:

* ``track_rigid`` on the 2 630-vertex mesh of DESIGN.md 7h (24^3 lattice at t = 0.3) tracked through four frames, whole call, and the
  twin's wall time on the same vertices;
* ``register_points`` (point-to-plane ICP) of a 65 536-point cloud -- centroids of triangles spread evenly over the mesh, taken out of
  place by a rotation vector (0.02, -0.03, 0.04) and a translation (0.02, -0.015, 0.01) -- against the mesh of the 256^3 extraction:
  the whole call at ``poll`` = 1, 4 and 16, its iteration count and status, the one-off grid build, and one iteration split into its
  four launches (apply, query, accumulate, update; 16 launches of each back to back at the final transform, no read-back).  The
  twin's closest-triangle search is brute force over all triangles: one iteration of it is timed on ``--twin-points`` rows and scaled
  to the cloud (recorded as extrapolated, with the rows it was measured on).

Events on the launch stream, one warm-up each, the candidates interleaved repetition by repetition, median of 5.  Numbers are
recorded, not gated.

    python tools/time_registration.py [--big 256] [--points 65536] [--twin-points 64] [--out profiles/registration_time.json]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))
import numpy as np
import torch

from gpu_util import renderer_for
from time_strain import REPS, interleaved_ms

POLLS = (1, 4, 16)
BATCH = 16
ROTVEC, SHIFT = (0.02, -0.03, 0.04), (0.02, -0.015, 0.01)


def track_case(eng, v):
    from endosurf_amd import registration
    ms = interleaved_ms({"track_rigid": lambda: eng.track_rigid(v)})["track_rigid"]
    hv = v.cpu().numpy()
    t0 = time.perf_counter()
    want = registration.track_rigid(hv)
    twin_ms = (time.perf_counter() - t0) * 1e3
    got = eng.track_rigid(v)
    row = {"case": "track_rigid, tracked mesh, 4 frames", "frames": int(v.shape[0]), "vertices": int(v.shape[1]), "device_ms": ms,
           "twin_ms": twin_ms, "twin_over_device": twin_ms / ms, "rmse": got["rmse"].cpu().numpy().tolist(),
           "rotation_minus_twin": float(np.abs(got["rotation"].cpu().numpy() - want["rotation"]).max()),
           "translation_minus_twin": float(np.abs(got["translation"].cpu().numpy() - want["translation"]).max())}
    print(json.dumps(row), flush=True)
    return row


def icp_case(eng, v, tri, n_points, twin_points):
    from endosurf_amd import meshing, registration
    from endosurf_amd._lib import check, ptr
    V, T = int(v.shape[0]), int(tri.shape[0])
    t32 = tri.to(torch.int32).contiguous()
    pick = torch.linspace(0, T - 1, n_points, device=v.device).long()
    cloud = v[t32[pick].long()].double().mean(1)
    R0, t0 = registration.rodrigues(ROTVEC), np.asarray(SHIFT)
    pts = ((cloud - torch.from_numpy(t0).to(v.device)) @ torch.from_numpy(R0).to(v.device)).float().contiguous()
    total = interleaved_ms({f"poll{p}": (lambda p=p: eng.icp(pts, v, t32, poll=p)) for p in POLLS})
    out = eng.icp(pts, v, t32)
    angle = registration.rotation_angle(out["rotation"].cpu().numpy() @ R0.T)
    shift = float(np.linalg.norm(out["translation"].cpu().numpy() - t0))
    # one iteration, launch by launch, at the final transform
    lib, st, N = eng.lib, eng.st(), n_points
    grid = eng._scratch("es_surf_scratch_bytes", V, T)
    scratch = eng._scratch("es_rigid_scratch_bytes", 1, N)
    state = torch.zeros(16, device=v.device, dtype=torch.float64)
    state[:9], state[9:12] = out["rotation"].reshape(9), out["translation"]
    state.view(torch.int32)[26:29] = torch.tensor([registration.MAX_ITERS, 0, 0], device=v.device, dtype=torch.int32)
    x, dist, near, closest = eng.empty(N, 3), eng.empty(N), eng.empty(N, dtype=torch.int32), eng.empty(N, 3)
    sums = eng.empty(registration.NORMAL_SUMS, dtype=torch.float64)

    def many(fn):
        def run():
            for _ in range(BATCH):
                fn()
        return run
    build = lambda: check(lib.es_surf_build(ptr(v), ptr(t32), V, T, ptr(grid), st), "es_surf_build")
    apply_ = lambda: check(lib.es_rigid_apply(ptr(state), ptr(state[9:]), ptr(pts), 1, N, 3 * N, ptr(x), None, None, None, st), "es_rigid_apply")
    query = lambda: check(lib.es_surf_query(ptr(x), N, ptr(v), ptr(t32), V, T, ptr(grid), ptr(dist), ptr(near), ptr(closest), None, st), "es_surf_query")
    accumulate = lambda: check(lib.es_icp_normal_equations(ptr(x), ptr(closest), ptr(near), ptr(dist), ptr(v), ptr(t32), V, T, N, -1.0, ptr(scratch),
                                                           ptr(sums), st), "es_icp_normal_equations")
    update = lambda: check(lib.es_icp_update(ptr(sums), registration.METHODS["plane"], 0.0, ptr(state), st), "es_icp_update")
    build(), apply_(), query(), accumulate()
    parts = interleaved_ms({"build": build, "apply": many(apply_), "query": many(query), "accumulate": many(accumulate), "update": many(update)})
    per = {k: parts[k] / BATCH for k in ("apply", "query", "accumulate", "update")}
    row = {"case": f"register_points, {n_points} points against the extraction", "points": n_points, "vertices": V, "triangles": T,
           "iterations": out["iterations"], "status": registration.STATUS_NAMES[out["status"]], "rmse": out["rmse"], "inliers": out["inliers"],
           "angle_error_rad": angle, "translation_error": shift, "total_ms_by_poll": {str(p): total[f"poll{p}"] for p in POLLS},
           "grid_build_ms": parts["build"], "iteration_ms": per, "iteration_ms_sum": sum(per.values())}
    if twin_points > 0:
        rows = pts[:: max(1, n_points // twin_points)][:twin_points].cpu().numpy()
        hv, ht = v.cpu().numpy(), tri.cpu().numpy()
        t1 = time.perf_counter()
        xs = registration.rigid_apply(np.eye(3), np.zeros(3), rows)
        d, near_h, c = meshing.point_to_mesh(xs, hv, ht)
        registration.icp_update(np.eye(3), np.zeros(3), registration.normal_equations(xs, c, near_h, d, hv, ht), "plane")
        twin_ms = (time.perf_counter() - t1) * 1e3
        row.update(twin_iteration_rows=len(rows), twin_iteration_ms_on_those_rows=twin_ms,
                   twin_iteration_ms_extrapolated=twin_ms * n_points / len(rows),
                   twin_extrapolated_over_device_iteration=twin_ms * n_points / len(rows) / sum(per.values()))
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--big", type=int, default=256)
    ap.add_argument("--points", type=int, default=65536)
    ap.add_argument("--twin-points", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "registration_time.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    r = renderer_for(11, "trained", True)
    eng = r.engine
    result = {"weights": "weightgen.make_state(11, 'trained', True)", "reps": REPS, "launch_batch": BATCH, "cases": []}
    box = ([-1.0, -1.0, -1.0], [1.0, 1.0, 1.0])
    with torch.cuda.device(r.device), torch.no_grad():
        mesh = r.extract_observation_mesh(0.3, *box, 24)
        track = r.track_mesh(mesh, t=0.3, times=[0.3, 0.31, 0.32, 0.9])
        result["cases"].append(track_case(eng, track["vertices"].contiguous()))
        big = r.extract_observation_mesh(0.3, *box, args.big)
        result["cases"].append(icp_case(eng, big["vertices"].contiguous(), big["triangles"], args.points, args.twin_points))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            json.dump(result, fo, indent=1)


if __name__ == "__main__":
    main()
