#!/usr/bin/env python3
"""Time the kinematics kernels on the GPU box (csrc/deform_jet.hip, csrc/kinematics.hip) on the seed-11 ``trained`` weights:
es_deform_derivatives -- value, three tangents, the time tangent and three second tangents of every point in one launch, 8 MLP rows per
point -- against es_deform_jacobian on the same points (4 rows per point, the four-row instance of the same kernel: about half the
time is the expectation) at M = 2 630, 4 096, 65 536 and 1 048 576 points (uniform in [-0.8, 0.8]^3, a random
time per row), and around the tile-height threshold; the finite-difference route it replaces, two ``track_points`` solves to t +- h
from a shared time; es_kinematics_rows with and without normals at the same sizes; and ``renderer.mesh_kinematics`` on the 2 630-vertex
mesh of DESIGN.md 7h (24^3 lattice at t = 0.3) tracked through t, t + 0.01, t + 0.02, 0.9.  Events on the launch stream, one warm-up
each, the candidates interleaved repetition by repetition, median of 5.  Numbers are recorded, not gated.

``--tile-libs SHORT TALL``: two more builds of the library that differ from the product in one constant, KINEMATICS_HALF_MAX_POINTS of
csrc/deform_jet.hip (INT_MAX: always the 32-row tile; 0: always the 64-row tile).  With them the tool times both tile heights at the
same point counts, interleaved, which is the table the constant is chosen from.

    python tools/time_kinematics.py [--points 2630 4096 65536 1048576] [--tile-libs short.so tall.so] [--out profiles/kinematics_time.json]
"""
import argparse
import ctypes as C
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

FD_STEP = 1e-3          # fp32 tracks: far above the solver's stopping length (1e-5), which a step of 1e-6 would drown in
TILE_POINTS = [512, 1024, 1536, 2048, 2560, 2630, 3072, 4096, 6144, 8192]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, nargs="+", default=[2630, 4096, 65536, 1048576])
    ap.add_argument("--tile-libs", nargs=2, metavar=("SHORT", "TALL"), default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "kinematics_time.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    from endosurf_amd import _lib
    r = renderer_for(11, "trained", True)
    eng = r.engine
    result = {"weights": "weightgen.make_state(11, 'trained', True)", "reps": REPS, "mmac_per_mlp_row": MMAC_PER_ROW, "fd_step": FD_STEP,
              "sizes": [], "tiles": None, "mesh": None}
    with torch.cuda.device(r.device), torch.no_grad():
        weff, packed = r._weights()
        weff = weff.detach()

        def inputs(M):
            rng = np.random.default_rng(111)
            x = torch.from_numpy(rng.uniform(-0.8, 0.8, size=(M, 3)).astype(np.float32)).to(r.device)
            t = torch.from_numpy(rng.uniform(size=(M,)).astype(np.float32)).to(r.device)
            n = torch.from_numpy(rng.normal(size=(M, 3)).astype(np.float32)).to(r.device)
            return x, t, n
        for M in args.points:
            x, t, n = inputs(M)
            ms = interleaved_ms({"derivatives": lambda: eng.deform_derivatives(eng.points(x=x, t=t), weff, packed),
                                 "jacobian": lambda: eng.deform_jacobian(eng.points(x=x, t=t), weff, packed),
                                 "two_solves": lambda: (r.track_points(x, 0.5, [0.5 + FD_STEP]), r.track_points(x, 0.5, [0.5 - FD_STEP]))})
            d = eng.deform_derivatives(eng.points(x=x, t=t), weff, packed)
            same = bool(torch.equal(d["jac"], eng.deform_jacobian(eng.points(x=x, t=t), weff, packed)))
            km = interleaved_ms({"with_normals": lambda: eng.kinematics_rows(d["jac"], d["d_t"], d["dd"], n),
                                 "without": lambda: eng.kinematics_rows(d["jac"], d["d_t"], d["dd"])})
            row = {"M": M, "derivatives_ms": ms["derivatives"], "jacobian_ms": ms["jacobian"],
                   "derivatives_over_jacobian": ms["derivatives"] / ms["jacobian"], "two_track_points_solves_ms": ms["two_solves"],
                   "speedup_over_two_solves": ms["two_solves"] / ms["derivatives"], "jac_bit_equal": same,
                   "derivatives_mmac_per_s": 8 * M * MMAC_PER_ROW / (ms["derivatives"] * 1e-3),
                   "kinematics_rows_ms": km["with_normals"], "kinematics_rows_without_normals_ms": km["without"]}
            result["sizes"].append(row)
            print(json.dumps(row), flush=True)
        if args.tile_libs:
            libs = {}
            for name, path in zip(("rows32", "rows64"), args.tile_libs):
                lib = C.CDLL(os.path.abspath(path))
                lib.es_deform_derivatives.restype = C.c_int
                lib.es_deform_derivatives.argtypes = _lib.PROTOTYPES["es_deform_derivatives"][1]
                assert lib.es_init() == 0
                libs[name] = lib
            result["tiles"] = []
            for M in TILE_POINTS:
                x, t, _ = inputs(M)
                out = [eng.empty(M, 3, 3), eng.empty(M, 3), eng.empty(M, 3, 3)]
                pts = eng.points(x=x, t=t)

                def call(lib, keep=None):
                    bufs = out if keep is None else keep
                    assert lib.es_deform_derivatives(C.byref(pts), _lib.ptr(packed), _lib.ptr(weff), _lib.ptr(bufs[0]), _lib.ptr(bufs[1]),
                                                     _lib.ptr(bufs[2]), None, eng.st()) == 0
                ms = interleaved_ms({k: (lambda lib=lib: call(lib)) for k, lib in libs.items()})
                a, b = ([torch.empty_like(o) for o in out] for _ in range(2))
                call(libs["rows32"], a)
                call(libs["rows64"], b)
                row = {"M": M, "rows32_ms": ms["rows32"], "rows64_ms": ms["rows64"], "same_bits": all(torch.equal(p, q) for p, q in zip(a, b))}
                result["tiles"].append(row)
                print(json.dumps(row), flush=True)
        mesh = r.extract_observation_mesh(0.3, [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0], 24)
        times = [0.3, 0.31, 0.32, 0.9]
        track = r.track_mesh(mesh, t=0.3, times=times)
        normals = torch.stack([eng.vertex_normals(track["vertices"][f].contiguous(), mesh["triangles"]) for f in range(len(times))])
        ms = interleaved_ms({"mesh_kinematics": lambda: r.mesh_kinematics(track, times),
                             "given_normals": lambda: r.mesh_kinematics(track, times, normals)})
        out = r.mesh_kinematics(track, times)
        ok = out["valid"]
        result["mesh"] = {"vertices": int(mesh["vertices"].shape[0]), "triangles": int(mesh["triangles"].shape[0]), "times": times,
                          "mesh_kinematics_ms": ms["mesh_kinematics"], "mesh_kinematics_given_normals_ms": ms["given_normals"],
                          "valid": int(ok.sum()), "rows": int(ok.numel()),
                          "speed_min_max": [float(out["speed"][ok].min()), float(out["speed"][ok].max())],
                          "area_rate_min_max": [float(out["area_rate"][ok].min()), float(out["area_rate"][ok].max())],
                          "divergence_min_max": [float(out["divergence"][ok].min()), float(out["divergence"][ok].max())]}
        print(json.dumps(result["mesh"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            json.dump(result, fo, indent=1)


if __name__ == "__main__":
    main()
