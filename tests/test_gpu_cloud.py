"""Point-cloud clean-up queries on the device (csrc/cloud.hip: Engine.self_nearest / radius_count / radius_outlier_mask) against their
numpy twins in endosurf_amd.meshing, which tests/test_cloud_host.py checks against scipy's cKDTree: every output bit-equal, because both
sides evaluate the same fp32 expression; and data.scene_normalization on device tensors against the same call on host arrays."""
import ctypes as C

import numpy as np
import pytest
import torch

from cloud_util import SCENE_ARGS, analytic_scene, collinear_cloud, lattice_cloud, planar_cloud, random_cloud, with_bad_rows
from endosurf_amd import data as D
from endosurf_amd import meshing as M
from endosurf_amd._lib import EndoSurfHipError, ptr

pytestmark = pytest.mark.gpu

# P = 0, 1, 2, 3; 7 (one cell); 257 (two workgroups); 5000 (many cells, 20 workgroups); axes of one cell; non-finite rows
CLOUDS = {
    "P0": lambda: np.zeros((0, 3), np.float32),
    "P1": lambda: random_cloud(1, seed=21),
    "P2": lambda: random_cloud(2, seed=22),
    "P3": lambda: random_cloud(3, seed=23),
    "P7": lambda: random_cloud(7, seed=24),
    "P257": lambda: random_cloud(257, seed=25, scale=3.0),
    "lattice5000": lambda: lattice_cloud(5000),
    "random5000": lambda: random_cloud(5000, seed=26, scale=40.0) + np.float32(100),
    "planar": planar_cloud,
    "collinear": collinear_cloud,
    "identical": lambda: np.tile(np.array([[0.5, -1.25, 3.0]], np.float32), (40, 1)),
    "bad_rows": lambda: with_bad_rows(lattice_cloud(1000, seed=9)),
    "only_bad_rows": lambda: np.full((5, 3), np.nan, np.float32),
}
_TWIN = {}          # name -> (points, twin self_nearest): computed once, never changed


def cloud(name):
    if name not in _TWIN:
        p = CLOUDS[name]()
        _TWIN[name] = (p, M.self_nearest(p))
    return _TWIN[name]


@pytest.fixture(scope="module")
def eng():
    from endosurf_amd.engine import Engine
    return Engine("cuda")


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@pytest.mark.parametrize("name", list(CLOUDS))
def test_self_nearest_is_the_twin(eng, name):
    p, (want_d, want_i) = cloud(name)
    dist, idx = eng.self_nearest(dev(p))
    assert dist.dtype == torch.float32 and idx.dtype == torch.int32 and dist.shape == idx.shape == (len(p),)
    assert np.array_equal(bits(dist.cpu().numpy()), bits(want_d)) and np.array_equal(idx.cpu().numpy(), want_i), name
    again = eng.self_nearest(dev(p))
    assert torch.equal(again[0].view(torch.int32), dist.view(torch.int32)) and torch.equal(again[1], idx)


def queries_for(p):
    """The first rows of the cloud (at most 1000), rows between the points, rows far outside the box and non-finite rows: Q is no multiple
    of 256."""
    fin = p[np.isfinite(p).all(1)]
    lo, hi = (fin.min(0), fin.max(0)) if len(fin) else (np.zeros(3, np.float32), np.ones(3, np.float32))
    rng = np.random.default_rng(31)
    between = (lo + rng.random((150, 3)) * (hi - lo)).astype(np.float32)
    far = np.array([hi + 1e6, lo - 1e6, [hi[0] + 3e4, lo[1], lo[2]], [1e30, -1e30, 1e30]], np.float32)
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]], np.float32)
    q = np.concatenate([p[:1000], between, far, bad]).astype(np.float32)
    assert len(q) % 256 != 0
    return q, float(((hi - lo).astype(np.float64) ** 2).sum())


@pytest.mark.parametrize("name", list(CLOUDS))
def test_radius_count_is_the_twin(eng, name):
    p, _ = cloud(name)
    q, diag2 = queries_for(p)
    pd, qd = dev(p), dev(q)
    for r2 in (0.0, 1e-30, 0.01 * diag2, diag2, np.inf, np.nan, -1.0):
        want = M.radius_count(q, p, radius_sq=r2)
        for cap in (0, 1, 6):
            got = eng.radius_count(qd, pd, radius_sq=r2, cap=cap)
            assert got.dtype == torch.int32 and got.shape == (len(q),)
            assert np.array_equal(got.cpu().numpy(), np.minimum(want, cap) if cap else want), (name, r2, cap)
    r = float(np.sqrt(0.01 * diag2)) if diag2 > 0 else 0.5
    want = M.radius_count(q, p, radius=r)
    as_float = eng.radius_count(qd, pd, r)
    as_tensor = eng.radius_count(qd, pd, torch.tensor(r, dtype=torch.float64, device="cuda"))          # squared in fp32 on the device
    assert np.array_equal(as_float.cpu().numpy(), want) and torch.equal(as_float, as_tensor), name
    assert torch.equal(eng.radius_count(qd, pd, r), as_float)                                         # two calls, the same bits
    mask = eng.radius_outlier_mask(pd, 5, r)
    assert mask.dtype == torch.bool and np.array_equal(mask.cpu().numpy(), M.radius_outlier_mask(p, 5, r)), name


def test_radius_count_reads_the_radius_on_the_device(eng):
    """20 x the mean neighbour distance, computed and used without leaving the device."""
    p, (dist, _) = cloud("random5000")
    pd = dev(p)
    d = eng.self_nearest(pd)[0]
    radius = 2.0 * d.double().mean()
    assert radius.is_cuda and radius.dim() == 0
    want = M.radius_outlier_mask(p, 5, np.float32(2.0 * dist.astype(np.float64).mean()))
    got = eng.radius_outlier_mask(pd, 5, radius.float())          # (the fp64 means may differ in their last bits; their fp32 roundings here do not)
    assert float(radius.float()) == float(np.float32(2.0 * dist.astype(np.float64).mean()))
    assert 0 < want.sum() < len(p) and np.array_equal(got.cpu().numpy(), want)


def test_unbuilt_scratch_answers_nothing(eng):
    """A scratch that was never built gives inf / -1 / 0, not a fault; a built one the twin's answer, whatever it held before."""
    lib, st = eng.lib, eng.st()
    p, (want_d, want_i) = cloud("P257")
    pd, P = dev(p), len(p)
    r2 = torch.tensor([4.0], device="cuda")
    for fill in (0xFF, 0x00):
        scr = torch.full((lib.es_nn_scratch_bytes(P),), fill, dtype=torch.uint8, device="cuda")
        dist, idx = torch.full((P,), -1.0, device="cuda"), torch.full((P,), -9, dtype=torch.int32, device="cuda")
        cnt = torch.full((P,), -9, dtype=torch.int32, device="cuda")
        assert lib.es_cloud_self_nearest(ptr(pd), P, ptr(scr), ptr(dist), ptr(idx), st) == 0
        assert lib.es_cloud_radius_count(ptr(pd), P, P, ptr(scr), ptr(r2), 0, ptr(cnt), st) == 0
        assert bool(dist.isinf().all()) and bool((idx == -1).all()) and bool((cnt == 0).all())
        assert lib.es_nn_build(ptr(pd), P, ptr(scr), st) == 0
        assert lib.es_cloud_self_nearest(ptr(pd), P, ptr(scr), ptr(dist), ptr(idx), st) == 0
        assert lib.es_cloud_radius_count(ptr(pd), P, P, ptr(scr), ptr(r2), 0, ptr(cnt), st) == 0
        assert np.array_equal(bits(dist.cpu().numpy()), bits(want_d)) and np.array_equal(idx.cpu().numpy(), want_i)
        assert np.array_equal(cnt.cpu().numpy(), M.radius_count(p, p, radius_sq=4.0))


def test_bad_arguments(eng):
    v = torch.rand(10, 3, device="cuda")
    with pytest.raises(EndoSurfHipError):
        eng.self_nearest(torch.zeros(4, 2, device="cuda"))
    with pytest.raises(EndoSurfHipError):
        eng.self_nearest(v.cpu())
    with pytest.raises(EndoSurfHipError):
        eng.radius_count(v, v, 1.0, cap=-1)
    with pytest.raises(EndoSurfHipError):
        eng.radius_count(v, v)
    with pytest.raises(EndoSurfHipError):
        eng.radius_count(v, v, torch.ones(2, device="cuda"))
    with pytest.raises(EndoSurfHipError):
        eng.radius_outlier_mask(v, -1, 1.0)
    lib = eng.lib
    dummy = torch.zeros(4096, device="cuda")
    p, odd = C.c_void_p(dummy.data_ptr()), C.c_void_p(dummy.data_ptr() + 4)

    def fails(status, word):
        assert status == 1 and word in lib.es_last_error(), (status, lib.es_last_error())

    fails(lib.es_cloud_self_nearest(None, 4, p, p, p, None), b"points")
    fails(lib.es_cloud_self_nearest(p, 4, p, None, p, None), b"dist")
    fails(lib.es_cloud_self_nearest(p, 4, p, p, None, None), b"index")
    fails(lib.es_cloud_self_nearest(p, 4, None, p, p, None), b"scratch")
    fails(lib.es_cloud_self_nearest(p, 4, odd, p, p, None), b"aligned")
    fails(lib.es_cloud_self_nearest(p, -4, p, p, p, None), b"negative")
    fails(lib.es_cloud_self_nearest(p, 1 << 31, p, p, p, None), b"2^31")
    assert lib.es_cloud_self_nearest(None, 0, None, None, None, None) == 0          # P == 0 writes nothing
    fails(lib.es_cloud_radius_count(None, 3, 4, p, p, 0, p, None), b"query")
    fails(lib.es_cloud_radius_count(p, 3, 4, p, None, 0, p, None), b"radius_sq")
    fails(lib.es_cloud_radius_count(p, 3, 4, p, p, 0, None, None), b"count")
    fails(lib.es_cloud_radius_count(p, 3, 4, None, p, 0, p, None), b"scratch")
    fails(lib.es_cloud_radius_count(p, 3, 4, odd, p, 0, p, None), b"aligned")
    fails(lib.es_cloud_radius_count(p, 3, 4, p, p, -1, p, None), b"cap")
    fails(lib.es_cloud_radius_count(p, -3, 4, p, p, 0, p, None), b"negative")
    fails(lib.es_cloud_radius_count(p, 3, -4, p, p, 0, p, None), b"negative")
    fails(lib.es_cloud_radius_count(p, 1 << 31, 4, p, p, 0, p, None), b"2^31")
    fails(lib.es_cloud_radius_count(p, 3, 1 << 31, p, p, 0, p, None), b"2^31")
    assert lib.es_cloud_radius_count(None, 0, 4, None, None, 0, None, None) == 0          # Q == 0 writes nothing


# ---- scene_normalization: device tensors against host arrays --------------------------------------------------------------------------------
def radius_is_not_critical(pts):
    """No point's capped count changes between radius (1 - 1e-3) and radius (1 + 1e-3): the last bits of the mean cannot matter.
    Returns the rows the pass keeps."""
    dist, _ = M.self_nearest(pts)
    nb, r = SCENE_ARGS["nb_points"], SCENE_ARGS["radius_factor"] * dist[np.isfinite(dist)].astype(np.float64).mean()
    below, above = (M.radius_count(pts, pts, r * s, cap=nb + 1) for s in (1 - 1e-3, 1 + 1e-3))
    assert np.array_equal(below, above)
    return pts[below > nb]


def test_scene_normalization_on_the_device_is_the_host_result(eng):
    depths, K, poses, planted = analytic_scene()
    # the condition, on the twin alone: every outlier pass of this scene (three frames, then the merged cloud) is far from a tie
    kept = [radius_is_not_critical(D.depth_points(torch.from_numpy(depths[i]), torch.from_numpy(K[i]), torch.from_numpy(poses[i]), np.inf).numpy())
            for i in range(len(depths))]
    radius_is_not_critical(np.concatenate(kept))
    host = D.scene_normalization(depths, K, poses, **SCENE_ARGS)
    got = D.scene_normalization(dev(depths), dev(K), dev(poses), engine=eng, **SCENE_ARGS)
    assert got["kept_mask"].is_cuda and torch.equal(got["kept_mask"].cpu(), host["kept_mask"])
    assert got["counts"] == host["counts"] and not (got["kept_mask"].cpu().numpy() & planted).any()
    assert got["close_depth"] == host["close_depth"] and got["inf_depth"] == host["inf_depth"]
    assert abs(got["depth_norm_scale"] - host["depth_norm_scale"]) <= 1e-6 * host["depth_norm_scale"]
    for key in ("scale_mat", "bbox_minmax"):
        a, b = got[key].cpu().double(), host[key].double()
        assert got[key].is_cuda and got[key].dtype == host[key].dtype and bool(((a - b).abs() <= 1e-6 * b.abs()).all()), key
    assert (got["points"].cpu() - host["points"]).abs().max() <= 1e-6
    again = D.scene_normalization(dev(depths), dev(K), dev(poses), engine=eng, **SCENE_ARGS)
    assert all(torch.equal(again[key], got[key]) for key in ("scale_mat", "bbox_minmax", "points", "kept_mask"))
