"""Point-to-surface distance on the device (csrc/surface.hip: Engine.point_to_mesh, data.cal_surface_error,
EndoSurfRenderer.surface_error) against the numpy twin endosurf_amd.meshing.point_to_mesh, which tests/test_surface_host.py checks
against an independent formulation.  The library is built with -ffp-contract=fast, so the device's fp64 d2 is not the twin's to the last
bit; three bounds hold everywhere (coordinates in [-1, 1]^3, L^2 <= 12: the fp64 error of ~20 operations is below 2^-44 L^2, its square
root at d near 0 is 2^-22 L, and both get a 16 x margin):
  |dist_dev - dist_twin| <= 2^-20 + one fp32 ulp of dist_twin;
  d2_twin[triangle_dev] - min d2_twin <= 2^-40 (the twin's value for the device's triangle);
  |closest_dev - closest_twin| <= 2^-19 wherever the twin's best two distinct d2 differ by more than 2^-36."""
import math

import numpy as np
import pytest
import torch

from endosurf_amd import data as D
from endosurf_amd._lib import EndoSurfHipError
from mesh_util import FIELD_CASES, hand_meshes, mt_mesh
from surface_util import D2_TOL, check_exact, exact_cases, soup, sphere_probe, twin_bounds

pytestmark = pytest.mark.gpu

HAND = hand_meshes()


@pytest.fixture(scope="module")
def eng():
    from endosurf_amd.engine import Engine
    return Engine("cuda")


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def run(eng, q, v, f):
    out = eng.point_to_mesh(dev(q), dev(v), dev(f))
    assert out[0].dtype == torch.float32 and out[1].dtype == torch.int32 and out[2].dtype == torch.float32
    assert out[0].shape == (len(q),) and out[1].shape == (len(q),) and out[2].shape == (len(q), 3)
    return tuple(x.cpu().numpy() for x in out)


def check_against_twin(eng, q, v, f, what):
    """The three bounds of the module's docstring; returns (device outputs, twin_bounds) for further checks."""
    ref = twin_bounds(q, v, f)
    dist, tri, at = got = run(eng, q, v, f)
    none = ref["triangle"] < 0
    assert np.array_equal(tri < 0, none) and (tri[none] == -1).all(), what
    assert np.isinf(dist[none]).all() and np.isnan(at[none]).all(), what
    ok = ~none
    assert ((tri[ok] >= 0) & (tri[ok] < len(f))).all(), what
    want = ref["dist"][ok].astype(np.float64)
    e1 = np.abs(dist[ok].astype(np.float64) - want) - np.spacing(ref["dist"][ok]).astype(np.float64)
    e2 = ref["d2"][np.nonzero(ok)[0], tri[ok]] - ref["best"][ok]
    clear = ref["clear"] & ok
    e3 = np.abs(at[clear].astype(np.float64) - ref["closest"][clear].astype(np.float64))
    worst = [float(e.max()) if e.size else 0.0 for e in (e1, e2, e3)]
    print(f"SURFACE_MEASURED {what}: V={len(v)} T={len(f)} Q={len(q)} |dist - twin| - ulp <= {worst[0]:.3e} (2^-20), d2[tri] - min <= {worst[1]:.3e} "
          f"(2^-40), |closest - twin| <= {worst[2]:.3e} (2^-19) on {int(clear.sum())} clear rows; same triangle {float((tri == ref['triangle']).mean()):.4f}")
    assert worst[0] <= 2.0 ** -20, what
    assert worst[1] <= D2_TOL, what
    assert worst[2] <= 2.0 ** -19, what
    return got, ref


def into_box(v):
    """Index-space or unbounded test vertices moved into [-1, 1]^3 (where the bounds are derived)."""
    v = np.asarray(v, np.float64)
    if len(v) == 0:
        return v.astype(np.float32)
    lo, hi = v.min(0), v.max(0)
    return ((v - 0.5 * (lo + hi)) * (1.8 / max(float((hi - lo).max()), 1e-30))).astype(np.float32)


def jittered(v, n, seed, sigma):
    rng = np.random.default_rng(seed)
    if len(v) == 0:
        return rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    q = v[rng.integers(0, len(v), n)].astype(np.float64) + rng.normal(size=(n, 3)) * sigma
    q[: n // 10] = v[rng.integers(0, len(v), n // 10)]                      # some exactly on vertices
    return np.clip(q, -1.0, 1.0).astype(np.float32)


def test_random_soup(eng):
    v, f, q = soup(300, 600, seed=11)
    (dist, tri, at), ref = check_against_twin(eng, q, v, f, "soup")
    assert dist[140:230].max() <= 2.0 ** -20                                # on vertices, in edges, in faces


@pytest.mark.parametrize("name", list(HAND))
def test_hand_made_meshes(eng, name):
    v, f = HAND[name]
    v = into_box(v)
    check_against_twin(eng, jittered(v, 500, 1, 0.05), v, f, name)


@pytest.mark.parametrize("name,shape,thr", FIELD_CASES)
def test_host_extracted_meshes(eng, name, shape, thr):
    v, f = mt_mesh(name, shape, thr)
    v = into_box(v)
    check_against_twin(eng, jittered(v, 500, 2, 0.03), v, f, name)


@pytest.fixture(scope="module")
def probe():
    return sphere_probe()


def test_sphere_probe_and_dominance(eng, probe):
    """The probe of the host file on the device, and dominance: every vertex of this mesh is referenced, the surface contains its
    vertices, so dist_surface <= dist_vertex (1 + 2^-20): the slack covers the fp32 rounding of ``nearest``'s sum of squares."""
    v, f, q, h = probe
    assert len(np.unique(f)) == len(v)
    (dist, tri, at), ref = check_against_twin(eng, q, v, f, "sphere 33^3")
    near = eng.nearest(dev(q), dev(v))[0].cpu().numpy()
    assert (dist.astype(np.float64) <= near.astype(np.float64) * (1 + 2.0 ** -20)).all()
    surf, vert = float(dist.astype(np.float64).mean()), float(near.astype(np.float64).mean())
    print(f"SURFACE_MEASURED sphere probe on the device: vertex {vert:.5f} surface {surf:.5f}")
    assert surf < 0.2 * vert
    assert abs(D.cal_surface_error(dev(q), dev(v), dev(f), 2.5, engine=eng) - 2.5 * surf) <= 1e-12
    assert abs(D.cal_surface_error(dev(q), dev(v), dev(f), 2.5) - 2.5 * float(ref["dist"].astype(np.float64).mean())) <= 2.5 * 2.0 ** -19


def test_dominance_on_jittered_queries(eng, probe):
    v, f, _, h = probe
    q = jittered(v, 2000, 5, 2 * h)
    dist = eng.point_to_mesh(dev(q), dev(v), dev(f))[0].double()
    near = eng.nearest(dev(q), dev(v))[0].double()
    assert bool((dist <= near * (1 + 2.0 ** -20)).all())


def test_one_huge_triangle_among_small_ones(eng):
    """The large-R path: 500 small triangles and one that spans the box, so that no query can stop before it has read most of the grid."""
    rng = np.random.default_rng(4)
    c = rng.uniform(-0.9, 0.9, (500, 1, 3))
    small = (c + rng.uniform(-0.02, 0.02, (500, 3, 3))).reshape(-1, 3)
    v = np.concatenate([small, [[-1, -1, -1], [1, 1, -0.5], [-1, 1, 1]]]).astype(np.float32)
    f = np.concatenate([np.arange(1500).reshape(500, 3), [[1500, 1501, 1502]]]).astype(np.int64)
    f = f[rng.permutation(501)]
    w = rng.dirichlet(np.ones(3), 100)
    on_huge = (w @ v[1500:].astype(np.float64) + rng.normal(size=(100, 3)) * 0.01).clip(-1, 1).astype(np.float32)
    q = np.concatenate([jittered(v, 400, 6, 0.05), on_huge, rng.uniform(-1, 1, (100, 3)).astype(np.float32)])
    (dist, tri, at), ref = check_against_twin(eng, q, v, f, "huge triangle")
    huge = int(np.nonzero((f == 1500).any(1))[0][0])
    assert (tri == huge).sum() > 20                                           # it is the answer for queries far from its centroid
    # work: with the huge triangle no walk can stop before the grid ends; without it most stop after a few shells
    work = eng.point_to_mesh(dev(q), dev(v), dev(f), return_work=True)[3].cpu().numpy()
    small_only = f[(f != 1500).all(1)]
    work_small = eng.point_to_mesh(dev(q), dev(v), dev(small_only), return_work=True)[3].cpu().numpy()
    assert work.shape == work_small.shape == (600, 2) and work.dtype == np.int32
    assert (work[:, 1] >= 1).all() and (work[:, 1] <= 501).all() and (work_small[:, 1] >= 1).all() and (work_small[:, 1] <= 500).all()
    assert (work[:, 0] >= work_small[:, 0]).all() and work[:, 0].mean() > work_small[:, 0].mean()


def test_flat_single_and_tiny(eng):
    rng = np.random.default_rng(8)
    # a flat mesh: all z equal (the grid has one cell along z)
    n = 12
    gx, gy = np.meshgrid(np.linspace(-0.8, 0.8, n), np.linspace(-0.8, 0.8, n), indexing="ij")
    v = np.stack([gx, gy, np.full_like(gx, 0.25)], -1).reshape(-1, 3).astype(np.float32)
    i = (np.arange(n - 1)[:, None] * n + np.arange(n - 1)[None]).reshape(-1)
    f = np.concatenate([np.stack([i, i + 1, i + n], 1), np.stack([i + 1, i + n + 1, i + n], 1)])
    q = np.concatenate([jittered(v, 300, 9, 0.1), rng.uniform(-1, 1, (100, 3)).astype(np.float32)])
    check_against_twin(eng, q, v, f, "flat")
    # a single triangle
    v1 = np.array([[-0.5, -0.25, 0.1], [0.7, -0.3, -0.2], [0.1, 0.6, 0.3]], np.float32)
    f1 = np.array([[0, 1, 2]])
    check_against_twin(eng, rng.uniform(-1, 1, (300, 3)).astype(np.float32), v1, f1, "single triangle")
    check_against_twin(eng, np.array([[0.3, 0.9, -0.7]], np.float32), v1, f1, "T = 1, Q = 1")
    check_against_twin(eng, np.array([[0.3, 0.9, -0.7]], np.float32), v1, f1.astype(np.int32), "int32 triangles")


@pytest.mark.parametrize("name", list(exact_cases()))
def test_exact_cases(eng, name):
    """Dyadic coordinates: every operation of the rule is exact, fused or not, so the device must give the known answer to the last
    bit -- the smallest index on a shared edge, at a fan's centre and among duplicates; NaN rows and empty inputs."""
    v, f, q = exact_cases()[name][:3]
    check_exact(name, run(eng, q, v, f))
    check_exact(name, run(eng, q, v, f.astype(np.int32)))


def test_indices_beyond_int32_stay_out_of_range(eng):
    v, f, q = exact_cases()["duplicates"][:3]
    f = np.concatenate([[[(1 << 32), (1 << 32) + 1, (1 << 32) + 2]], f])     # would wrap to (0, 1, 2)
    dist, tri, at = run(eng, q, v, f)
    assert tri.tolist() == [1] and dist.tolist() == [0.5]


def test_argument_errors(eng):
    v, f, q = (dev(x) for x in exact_cases()["duplicates"][:3])
    for bad in (dict(points=q[:, :2]), dict(points=q.reshape(-1)), dict(points=q.cpu()), dict(vertices=v.cpu()), dict(vertices=v[:, :2]),
                dict(triangles=f.cpu()), dict(triangles=f[:, :2]), dict(triangles=f.float()), dict(triangles=f.to(torch.int16)),
                dict(triangles=f.reshape(-1))):
        kw = dict(points=q, vertices=v, triangles=f)
        kw.update(bad)
        with pytest.raises(EndoSurfHipError):
            eng.point_to_mesh(**kw)


def test_two_calls_give_the_same_bits_whatever_the_scratch_held(eng, probe, monkeypatch):
    v, f, q, _ = probe
    q = np.concatenate([q[:500], [[np.nan, 0, 0]]]).astype(np.float32)
    dq, dv, df = dev(q), dev(v), dev(f)
    first = eng.point_to_mesh(dq, dv, df)
    again = eng.point_to_mesh(dq, dv, df)
    # the same call with its scratch filled with garbage before the build
    plain = eng._scratch

    def dirty(fn_name, *dims):
        s = plain(fn_name, *dims)
        s.copy_(torch.randint(0, 256, s.shape, device=s.device, dtype=torch.uint8, generator=torch.Generator(s.device).manual_seed(3)))
        return s
    monkeypatch.setattr(eng, "_scratch", dirty)
    third = eng.point_to_mesh(dq, dv, df)
    for a, b, c in zip(first, again, third):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() == c.cpu().numpy().tobytes()


# ---- the metric on a trained scene (the fixture of tests/test_gpu_mesh.py::test_geometric_error_of_a_rendered_depth_map) ----------------
BMIN, BMAX = [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]


@pytest.fixture(scope="module")
def scene():
    from gpu_util import renderer_for_case
    from oracle_util import load_case
    return renderer_for_case(load_case("trained_deform")), torch.tensor([0.37])


def test_surface_error_of_a_rendered_depth_map(scene):
    r, t = scene
    h, w = 40, 48
    K = torch.tensor([[60.0, 0, 23.5, 0], [0, 60.0, 19.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    pose = torch.eye(4)
    pose[:3, 3] = torch.tensor([0.0, 0.0, -1.5])
    rays = D.assemble_rays(D.get_rays(K[None].cuda(), pose[None].cuda(), w, h), torch.zeros(1, 2, device="cuda"))
    rays[..., 8] = float(t)
    out = r.render_frames(rays, iter_step=1, ray_chunk=512, perturb_overwrite=False, use_graph=False)
    depth = out["depth"].reshape(h, w)
    trunc = float(depth.median())          # drops about half of the pixels
    mesh = r.extract_observation_mesh(t, BMIN, BMAX, 97, components=0.9)
    taus = (0.001, 0.01, 0.05, 0.5, 100.0)
    got = r.surface_error(mesh, depth, K, pose, trunc, depth_scale=2.5, thresholds=taus)
    assert {"mean", "rmse", "max", "vertex_mean", "within"} <= set(got)
    assert got["vertex_mean"] == r.geometric_error(mesh, depth, K, pose, trunc, depth_scale=2.5)
    assert math.isfinite(got["mean"]) and 0.0 <= got["mean"] <= got["vertex_mean"]
    assert got["mean"] <= got["rmse"] * (1 + 1e-12) and got["rmse"] <= got["max"] * (1 + 1e-12)
    assert len(got["within"]) == len(taus) and all(a <= b for a, b in zip(got["within"], got["within"][1:]))
    assert 0.0 <= got["within"][0] and got["within"][-1] == 1.0
    pts = D.depth_points(depth, K, pose, trunc)
    assert got["points"] == pts.shape[0] > 0
    assert got["mean"] == D.cal_surface_error(pts, mesh["vertices"], mesh["triangles"], 2.5, engine=r.engine)
    pair = r.surface_error((mesh["vertices"].cpu().numpy(), mesh["triangles"].cpu().numpy()), depth.cpu().numpy(), K, pose, trunc, 2.5, taus)
    assert pair == got
    # against the twin on the host, on a part of the cloud (the whole of it would take the twin a minute)
    sub = pts[:: max(1, pts.shape[0] // 50)]
    want = D.cal_surface_error(sub.cpu(), mesh["vertices"].cpu(), mesh["triangles"].cpu(), 2.5)
    assert abs(D.cal_surface_error(sub, mesh["vertices"], mesh["triangles"], 2.5) - want) <= 2.5 * 2.0 ** -19
    empty = r.surface_error(mesh, depth, K, pose, 0.0, thresholds=(0.1,))
    assert empty["points"] == 0 and math.isnan(empty["mean"]) and math.isnan(empty["within"][0])
    print(f"SURFACE_MEASURED trained R=97: {got['points']} points, V={mesh['vertices'].shape[0]} T={mesh['triangles'].shape[0]}: {got}")
