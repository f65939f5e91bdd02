#!/usr/bin/env python3
"""Time the geodesic solver on the GPU box (csrc/geodesic.hip through ``Engine.geodesic``) against its host twin
(``geodesic.mesh_geodesic``) on the seed-11 ``trained`` weights: the 2 630-vertex mesh of DESIGN.md 7h (24^3 lattice at t = 0.3)
tracked through four frames, with 1 and with 16 vertex sources (4 and 64 fields in one launch per sweep), and the 256^3 extraction
with one source.  Per case: the sweep count, the whole call at ``poll`` = 1, 8 and 32 (one word read back per ``poll`` sweeps), the
time of one sweep launch at the fixed point (every triangle computes; 64 launches back to back, no read-back), what is left per
read-back once the sweeps are taken out, and the twin's wall time on the same inputs.  (``cached_geometry`` in
profiles/geodesic_time.json is the same run's figures for a variant that read g11, g12, g22 of every corner from a per-(frame,
triangle) cache; it lost on the large mesh and is not in the library: DESIGN.md 7m.)  Events on the launch stream, one warm-up
each, the candidates interleaved repetition by repetition, median of 5.  Numbers are recorded, not gated.

    python tools/time_geodesic.py [--big 256] [--no-big-twin] [--out profiles/geodesic_time.json]
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

POLLS = (1, 8, 32)
SWEEP_BATCH = 64


def sweep_ms(eng, v, tri, S):
    """Milliseconds of one sweep launch at the fixed point of S vertex sources (ids spread over the mesh)."""
    from endosurf_amd._lib import check, ptr
    F, V, T = int(v.shape[0]), int(v.shape[1]), int(tri.shape[0])
    t32 = tri.to(torch.int32).contiguous()
    src = torch.linspace(0, V - 1, S, device=v.device).long()
    done = eng.geodesic(v, tri, src)["distance"].double().reshape(F * S, V).contiguous()
    cur = done.view(torch.int64).clone()
    nxt = cur.clone()
    state = {"cur": cur, "nxt": nxt}

    def run():
        for _ in range(SWEEP_BATCH):
            check(eng.lib.es_geodesic_sweep(ptr(v), ptr(t32), F, V, T, S, ptr(state["cur"]), ptr(state["nxt"]), None, eng.st()),
                  "es_geodesic_sweep")
            state["cur"], state["nxt"] = state["nxt"], state["cur"]
    return run


def case(eng, name, v, tri, S, twin=True):
    from endosurf_amd import geodesic
    F, V, T = int(v.shape[0]), int(v.shape[1]), int(tri.shape[0])
    src = torch.linspace(0, V - 1, S, device=v.device).long()
    calls = {f"poll{p}": (lambda p=p: eng.geodesic(v, tri, src, poll=p)) for p in POLLS}
    total = interleaved_ms(calls)
    sweeps = {p: eng.geodesic(v, tri, src, poll=p)["sweeps"] for p in POLLS}
    per = interleaved_ms({"sweep": sweep_ms(eng, v, tri, S)})["sweep"] / SWEEP_BATCH
    row = {"case": name, "frames": F, "sources": S, "fields": F * S, "vertices": V, "triangles": T,
           "sweeps_by_poll": {str(p): sweeps[p] for p in POLLS}, "total_ms_by_poll": {str(p): total[f"poll{p}"] for p in POLLS},
           "sweep_ms": per, "left_per_readback_ms": {str(p): (total[f"poll{p}"] - sweeps[p] * per) / (sweeps[p] / p) for p in POLLS}}
    if twin:
        hv, ht, hs = v.cpu().numpy(), tri.cpu().numpy(), src.cpu().numpy()
        t0 = time.perf_counter()
        want = geodesic.mesh_geodesic(hv, ht, hs)
        row["twin_ms"] = (time.perf_counter() - t0) * 1e3
        row["twin_sweeps"] = want["sweeps"]
        row["twin_over_device_poll8"] = row["twin_ms"] / total["poll8"]
        got = eng.geodesic(v, tri, src)["distance"].cpu().numpy()
        d = np.abs(got.view(np.int32).astype(np.int64) - want["distance"].view(np.int32).astype(np.int64))
        row["entries_differing_from_twin"], row["max_ulp_from_twin"] = int((d > 0).sum()), int(d.max())
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--big", type=int, default=256)
    ap.add_argument("--no-big-twin", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "geodesic_time.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    r = renderer_for(11, "trained", True)
    eng = r.engine
    result = {"weights": "weightgen.make_state(11, 'trained', True)", "reps": REPS, "sweep_batch": SWEEP_BATCH, "cases": []}
    box = ([-1.0, -1.0, -1.0], [1.0, 1.0, 1.0])
    with torch.cuda.device(r.device), torch.no_grad():
        mesh = r.extract_observation_mesh(0.3, *box, 24)
        track = r.track_mesh(mesh, t=0.3, times=[0.3, 0.31, 0.32, 0.9])
        v, tri = track["vertices"].contiguous(), mesh["triangles"]
        for S in (1, 16):
            result["cases"].append(case(eng, f"tracked mesh, 4 frames, {S} source(s)", v, tri, S))
        big = r.extract_observation_mesh(0.3, *box, args.big)
        result["cases"].append(case(eng, f"{args.big}^3 extraction, 1 source", big["vertices"][None].contiguous(), big["triangles"], 1,
                                    twin=not args.no_big_twin))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            json.dump(result, fo, indent=1)


if __name__ == "__main__":
    main()
