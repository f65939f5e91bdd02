"""Geodesic distance on the device (csrc/geodesic.hip: the C ABI, Engine.geodesic, EndoSurfRenderer.mesh_geodesic / track_geodesic)
against the numpy twin endosurf_amd.geodesic, which tests/test_geodesic_host.py checks on its own.  The device promises the same bits
from call to call and for any ``poll``, and the twin's values to one fp32 ulp after rounding (the fp64 fields differ by rounding
only, tests/test_geodesic_host.py measures 1e-12, so only a rounding-boundary flip can show): not the twin's fp64 bits."""
import numpy as np
import pytest
import torch

from endosurf_amd import _lib
from endosurf_amd import geodesic as G
from endosurf_amd._lib import EndoSurfHipError, check, ptr
from geodesic_util import NAN, bumpy, check_exact, exact_cases, grid_mesh, rigid_track, sphere_mesh, twin_sphere, ulps

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from endosurf_amd.engine import Engine
    return Engine("cuda")


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def engine_solve(eng, **kw):
    def solve(v, f, src):
        out = eng.geodesic(dev(v), dev(f), dev(src), **kw)
        assert out["distance"].dtype == torch.float32 and out["distance"].is_cuda
        return out["distance"].cpu().numpy(), out["sweeps"]
    return solve


def abi_solve(v, f, src):
    """The four entries called one by one: seeds, a sweep and a read-back at a time, the rounding."""
    lib = _lib.load()
    st = _lib.stream_ptr()
    vt, tt = dev(v, torch.float32), dev(f, torch.int32).reshape(-1, 3)
    V, T, S = len(v), len(f), len(src)
    cur, nxt = (torch.empty(S, V, device="cuda", dtype=torch.int64) for _ in range(2))
    field, vertex = torch.arange(S, device="cuda", dtype=torch.int32), dev(src, torch.int32)
    value = torch.zeros(S, device="cuda", dtype=torch.float64)
    check(lib.es_geodesic_seed(ptr(vt), ptr(tt), 1, V, T, S, ptr(field), ptr(vertex), ptr(value), S, ptr(cur), ptr(nxt), st), "seed")
    changed = torch.ones(1, device="cuda", dtype=torch.int32)
    sweeps = 0
    while True:
        check(lib.es_geodesic_sweep(ptr(vt), ptr(tt), 1, V, T, S, ptr(cur), ptr(nxt), ptr(changed), st), "sweep")
        cur, nxt = nxt, cur
        sweeps += 1
        if not int(changed.item()):
            break
        assert sweeps <= V + 1
    assert torch.equal(cur, nxt)          # the sweep that changed nothing left both buffers at the fixed point
    out = torch.empty(S, V, device="cuda")
    check(lib.es_geodesic_finish(ptr(cur), S * V, ptr(out), st), "finish")
    return out.cpu().numpy(), sweeps


@pytest.mark.parametrize("name", list(exact_cases()))
def test_exact_cases(eng, name):
    """Dyadic coordinates: the checked values are exact in the rule, so the device gives them to the last bit -- through the C ABI
    (whose sweep count is the twin's) and through Engine.geodesic."""
    check_exact(name, abi_solve)
    v, f, src = exact_cases()[name]
    assert abi_solve(v, f, np.asarray(src))[1] == G.mesh_geodesic(v, f, np.asarray(src))["sweeps"]
    check_exact(name, engine_solve(eng))
    check_exact(name, engine_solve(eng, poll=3))


def against_twin(got, want, what):
    """Within one fp32 ulp everywhere, the same +inf pattern; prints how many entries differ at all."""
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float32, what
    assert np.array_equal(np.isinf(got), np.isinf(want)) and not np.isnan(got).any(), what
    d = ulps(got, want)
    print(f"GEODESIC_MEASURED {what}: {int((d > 0).sum())} of {d.size} fp32 entries differ from the twin, at most {int(d.max()) if d.size else 0} ulp")
    assert (d <= 1).all(), what


@pytest.mark.parametrize("n,method", [(17, "tetrahedra"), (17, "cubes"), (33, "tetrahedra"), (33, "cubes")])
def test_sphere_probes_against_the_twin(eng, n, method):
    v, f, top = sphere_mesh(n, method)
    want = twin_sphere(n, method)
    poll = 8
    out = eng.geodesic(dev(v), dev(f), dev(np.array([top])), poll=poll)
    against_twin(out["distance"], want["distance"], f"sphere {method} {n}^3")
    assert out["sweeps"] == -(-want["sweeps"] // poll) * poll


def test_same_bits_from_call_to_call_and_for_any_poll(eng):
    v, f, top = sphere_mesh(33)
    dv, df, src = dev(v), dev(f.astype(np.int32)), dev(np.array([top, 7, 1000]))
    first = eng.geodesic(dv, df, src)
    runs = [eng.geodesic(dv, df, src)] + [eng.geodesic(dv, df, src, poll=p) for p in (1, 8, 32)]
    assert all(torch.equal(r["distance"], first["distance"]) for r in runs)
    want = G.mesh_geodesic(v, f, np.array([top, 7, 1000]))["sweeps"]
    assert [r["sweeps"] for r in runs] == [-(-want // p) * p for p in (8, 1, 8, 32)]


@pytest.mark.parametrize("nx,ny", [(19, 15), (4, 3)])
def test_many_fields_in_one_launch(eng, nx, ny):
    """F = 3 frames x S = 5 sources: each [f, s] slice is the single-field call on that frame, to the bit (a wrong frame index b / S or
    a wrong stride shows here).  V = 285, T = 504: no multiples of the block; and T = 12, below one wavefront."""
    v, f = bumpy(nx, ny)
    track = rigid_track(v, f, scaled=True)
    src = np.array([0, len(v) - 1, len(v) // 2, 5, len(v) - 3])
    dv, df = dev(track["vertices"]), dev(f)
    out = eng.geodesic(dv, df, dev(src))
    assert out["distance"].shape == (3, 5, len(v))
    for fr in range(3):
        for s in range(5):
            one = eng.geodesic(dv[fr].contiguous(), df, dev(src[s:s + 1]))
            assert one["distance"].shape == (1, len(v)) and torch.equal(out["distance"][fr, s], one["distance"][0]), (fr, s)
    want = G.mesh_geodesic(track["vertices"], f, src)
    against_twin(out["distance"], want["distance"], f"track {nx} x {ny}")
    assert out["sweeps"] == -(-want["sweeps"] // 8) * 8
    assert torch.equal(out["distance"][2], 2.0 * out["distance"][0])          # the scaled frame: every operation scales exactly


def two_components():
    """The 5 x 5 dyadic grid in the plane z = 0 and, out of reach, one more triangle at z = 4: projections onto it are exact."""
    v, f = grid_mesh(5)
    return np.concatenate([v, v[[0, 5, 6]] + [0, 0, 4.0]]).astype(np.float32), np.concatenate([f, [[25, 26, 27]]])


def test_point_sources_and_targets_against_the_twin(eng):
    """Points in a triangle, on an edge, on a vertex, above the plane, and a non-finite one; targets in the source's triangle, elsewhere,
    in the component out of reach, and non-finite -- over three rigidly moved frames, with frame 1 as the reference."""
    v, f = two_components()
    track = rigid_track(v, f)
    ref = track["vertices"][1].astype(np.float64)
    local = np.array([[0.3125, 0.0625, 0.0], [0.5, 0.375, 0.0], [0.25, 0.75, 0.0], [0.6875, 0.4375, 0.5], [NAN, 0.0, 0.0]])
    local_q = np.array([[0.4375, 0.125, 0.0], [0.9375, 0.875, 0.0], [0.5, 0.5, 0.0], [0.0625, 0.03125, 4.0], [0.0, NAN, 0.0], [0.625, 0.375, 0.0]])
    move = lambda p: (p @ np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]).T + [0.25, -0.5, 0.125]).astype(np.float32)
    assert np.array_equal(move(v.astype(np.float64)), track["vertices"][1])
    p, q = move(local), move(local_q)
    want = G.mesh_geodesic(track["vertices"], f, p, targets=q, reference=1)
    out = eng.geodesic(dev(track["vertices"]), dev(f), dev(p), dev(q), reference=1)
    against_twin(out["distance"], want["distance"], "point sources")
    against_twin(out["target_distance"], want["target_distance"], "targets")
    td = out["target_distance"].cpu().numpy()
    assert td.shape == (3, 5, 6) and np.isinf(td[:, 4]).all() and np.isinf(td[:, :, 3:5]).all() and np.isfinite(td[:, :4][:, :, [0, 1, 2, 5]]).all()
    same = np.float32(np.hypot(0.125, 0.0625))          # source 0 and target 0 share a triangle: the straight distance, in every frame
    assert (ulps(td[:, 0, 0], np.full(3, same)) <= 1).all()
    again = eng.geodesic(dev(track["vertices"]), dev(f), dev(p), dev(q), reference=1, poll=1)
    assert torch.equal(again["distance"], out["distance"]) and torch.equal(again["target_distance"], out["target_distance"])
    single = eng.geodesic(dev(track["vertices"][1]), dev(f), dev(p), dev(q))
    assert single["distance"].shape == (5, 28) and torch.equal(single["distance"], out["distance"][1])
    assert single["target_distance"].shape == (5, 6) and torch.equal(single["target_distance"], out["target_distance"][1])


def test_sweep_cap_raises(eng):
    v, f = grid_mesh(5)
    with pytest.raises(EndoSurfHipError, match="fixed point"):
        eng.geodesic(dev(v), dev(f), dev(np.array([0])), max_sweeps=1)
    assert eng.geodesic(dev(v), dev(f), dev(np.array([0])), max_sweeps=5, poll=32)["sweeps"] == 5          # the twin's count: just enough


def test_engine_argument_errors(eng):
    v, f = (dev(x) for x in grid_mesh(3))
    src = dev(np.array([0]))
    for bad in (dict(vertices=v.cpu()), dict(vertices=v[:, :2]), dict(triangles=f.cpu()), dict(triangles=f.float()), dict(sources=src.cpu()),
                dict(sources=src.reshape(1, 1)), dict(sources=v[:1, :2]), dict(sources=src[:0]), dict(reference=1), dict(poll=0),
                dict(targets=v.cpu())):
        kw = dict(vertices=v, triangles=f, sources=src)
        kw.update(bad)
        with pytest.raises(EndoSurfHipError):
            eng.geodesic(**kw)


def test_bad_arguments_return_error_codes():
    """Status 1 with a message that names the argument, before anything is launched (host addresses, never dereferenced); empty meshes
    are status 0."""
    lib = _lib.load()
    buf = np.zeros(64, np.float64)
    b = buf.ctypes.data
    b2 = b + 256

    def seed(v=b, t=b, F=1, V=4, T=2, S=1, sf=b, sv=b, sx=b, n=1, cur=b, nxt=b2):
        return lib.es_geodesic_seed(v, t, F, V, T, S, sf, sv, sx, n, cur, nxt, None)

    def sweep(v=b, t=b, F=1, V=4, T=2, S=1, cur=b, nxt=b2):
        return lib.es_geodesic_sweep(v, t, F, V, T, S, cur, nxt, None, None)

    def read(field=b, v=b, t=b, F=1, V=4, T=2, S=1, qt=b, qp=b, Q=1, st=None, sp=None, out=b):
        return lib.es_geodesic_read(field, v, t, F, V, T, S, qt, qp, Q, st, sp, out, None)
    for call in (seed, sweep, read):
        assert call(v=None) == 1 and b"vertices" in lib.es_last_error()
        assert call(t=None) == 1 and b"triangles" in lib.es_last_error()
        assert call(S=0) == 1 and b"S must" in lib.es_last_error()
        for neg in ("F", "V", "T"):
            assert call(**{neg: -1}) == 1 and b"negative" in lib.es_last_error()
        assert call(V=1 << 31) == 1 and b"2^31" in lib.es_last_error()
    assert seed(cur=None) == 1 and b"cur" in lib.es_last_error()
    assert seed(nxt=b) == 1 and b"two buffers" in lib.es_last_error()
    assert seed(sv=None) == 1 and b"seed_vertex" in lib.es_last_error()
    assert seed(n=-1) == 1 and b"n_seeds" in lib.es_last_error()
    assert sweep(nxt=None) == 1 and b"next" in lib.es_last_error()
    assert sweep(nxt=b) == 1 and b"two buffers" in lib.es_last_error()
    assert read(qt=None) == 1 and b"target_triangle" in lib.es_last_error()
    assert read(out=None) == 1 and b"out" in lib.es_last_error()
    assert read(field=None) == 1 and b"field" in lib.es_last_error()
    assert read(st=b) == 1 and b"source_point" in lib.es_last_error()
    assert read(Q=-1) == 1 and b"Q" in lib.es_last_error()
    assert lib.es_geodesic_finish(None, 4, b, None) == 1 and b"field" in lib.es_last_error()
    assert lib.es_geodesic_finish(b, -1, b, None) == 1 and b"negative" in lib.es_last_error()
    # nothing to do: status 0 with null buffers
    assert seed(v=None, F=0, cur=None, nxt=None) == 0 and seed(v=None, V=0, cur=None, nxt=None) == 0
    assert sweep(v=None, F=0, cur=None, nxt=None) == 0 and sweep(v=None, t=None, V=0, T=0, cur=None, nxt=None) == 0
    assert read(Q=0, qt=None, qp=None, out=None) == 0 and lib.es_geodesic_finish(None, 0, None, None) == 0


@pytest.fixture(scope="module")
def R():
    from gpu_util import renderer_for
    return renderer_for(11, "trained", True)


def test_renderer_calls(R):
    """The small test renderer's tracked mesh: keys, shapes, device residency, equality with Engine.geodesic on the same tensors; a
    mesh dict, a (vertices, triangles) pair and host inputs are accepted."""
    n = 17
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    verts = (np.array([-0.2, -0.25, 0.1])[None] + i.reshape(-1, 1) * np.array([0.02, 0.004, -0.006])[None]
             + j.reshape(-1, 1) * np.array([-0.002, 0.018, 0.008])[None]).astype(np.float32)
    tris = grid_mesh(n)[1]
    track = R.track_mesh(dev(verts), dev(tris), t=0.3, times=[0.3, 0.5, 0.9])
    assert bool(track["converged"].all())
    src, q = np.array([0, 150]), (0.5 * verts[[40, 200]] + 0.5 * verts[[41, 217]]).astype(np.float32)
    out = R.mesh_geodesic(track, src, targets=q)
    assert set(out) == {"distance", "sweeps", "target_distance"} and out["distance"].is_cuda and out["target_distance"].is_cuda
    assert out["distance"].shape == (3, 2, 289) and out["target_distance"].shape == (3, 2, 2) and out["sweeps"] % 8 == 0
    assert bool(torch.isfinite(out["distance"]).all()) and bool((out["distance"][:, 0, 1:] > 0).all())
    direct = R.engine.geodesic(track["vertices"], dev(tris), dev(src), dev(q))
    assert torch.equal(direct["distance"], out["distance"]) and torch.equal(direct["target_distance"], out["target_distance"])
    mesh = R.mesh_geodesic({"vertices": dev(verts), "triangles": dev(tris)}, src)
    pair = R.mesh_geodesic((verts, tris), src.tolist())
    assert set(mesh) == {"distance", "sweeps"} and mesh["distance"].shape == (2, 289) and torch.equal(mesh["distance"], pair["distance"])
    assert torch.equal(mesh["distance"], R.engine.geodesic(dev(verts), dev(tris), dev(src))["distance"])
    a, b = verts[[0, 150]], q
    lengths = R.track_geodesic(track, a, b)
    paired = R.mesh_geodesic(track, a, targets=b)["target_distance"]
    assert lengths.shape == (3, 2) and lengths.is_cuda and torch.equal(lengths, torch.stack([paired[:, 0, 0], paired[:, 1, 1]], 1))
    host = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in track.items()}
    assert torch.equal(R.track_geodesic(host, a.tolist(), b.tolist()), lengths)
    print(f"GEODESIC_MEASURED tracked patch: lengths over the frames {lengths.cpu().numpy().round(5).tolist()}, sweeps {out['sweeps']}")
