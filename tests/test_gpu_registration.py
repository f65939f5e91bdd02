"""Rigid registration on the device (csrc/register.hip: the C ABI, Engine.rigid_moments / rigid_fit / rigid_apply / track_rigid / icp,
EndoSurfRenderer.track_rigid / register_points / register_mesh) against the numpy twin endosurf_amd.registration, which
tests/test_registration_host.py checks on its own.  The device promises the same bits from call to call and for any ``poll``; the
twin's bits where every sum is exact; otherwise the twin's values within the bounds worked out at each test."""
import numpy as np
import pytest
import torch

from endosurf_amd import _lib
from endosurf_amd import registration as REG
from endosurf_amd._lib import EndoSurfHipError, check, ptr
from geodesic_util import bumpy, grid_mesh, rigid_track
from registration_util import (ICP_CASES, INVALID_CASES, RECOVERY, icp_case, is_rotation, measured_tolerance, mirrored_plane, motion_error,
                               permutation_spread, random_cloud, twin_icp)

pytestmark = pytest.mark.gpu

CHUNK = REG.MOMENT_CHUNK
EDGE_SIZES = [1, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5]          # thread / workgroup / second-stage edges


@pytest.fixture(scope="module")
def eng():
    from endosurf_amd.engine import Engine
    return Engine("cuda")


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def abi_moments(p, q, w, scratch_fill=None):
    """es_rigid_moments called directly: p, q [B,N,3] fp32, w None / [N] / [B,N] -> [B,17] fp64 numpy."""
    lib, st = _lib.load(), _lib.stream_ptr()
    B, N = p.shape[:2]
    nbytes = lib.es_rigid_scratch_bytes(B, N)
    assert nbytes > 0 and nbytes % 16 == 0
    scratch = torch.empty(nbytes, device="cuda", dtype=torch.uint8)
    if scratch_fill is not None:
        scratch.view(torch.float64).fill_(scratch_fill)
    out = torch.full((B, 17), float("nan"), device="cuda", dtype=torch.float64)
    tp, tq, tw = dev(p, torch.float32), dev(q, torch.float32), None if w is None else dev(w, torch.float32)
    check(lib.es_rigid_moments(ptr(tp), ptr(tq), ptr(tw), B, N, int(w is not None and w.ndim == 2), ptr(scratch), ptr(out), st), "es_rigid_moments")
    return out.cpu().numpy()


def dyadic(B, N, seed):
    rng = np.random.default_rng(seed)
    p, q = (rng.integers(-256, 257, (2, B, N, 3)) / 64.0).astype(np.float32)          # multiples of 1/64, |x| <= 4
    w = (rng.integers(0, 9, (B, N)) / 4.0).astype(np.float32)                           # 0 .. 2 in quarters; some rows weigh nothing
    return p, q, w


def test_scratch_size_follows_the_chunk():
    lib = _lib.load()
    one = lib.es_rigid_scratch_bytes(1, CHUNK)
    assert lib.es_rigid_scratch_bytes(1, 1) == one and lib.es_rigid_scratch_bytes(1, CHUNK + 1) > one
    assert lib.es_rigid_scratch_bytes(3, 3 * CHUNK + 5) >= 8 * 17 * 3 * 4


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N", EDGE_SIZES)
def test_moments_exact(N, B):
    """Dyadic coordinates and weights: every partial sum is exact in fp64, so any order of summation gives the twin's bits."""
    p, q, w = dyadic(B, N, 100 * B + N)
    for weights in (w, w[0], None):
        got, want = abi_moments(p, q, weights), REG.rigid_moments(p, q, weights)
        assert got.shape == (B, 17) and np.array_equal(got, want), (N, B, None if weights is None else weights.shape, np.abs(got - want).max())


@pytest.mark.parametrize("B,N", [(1, 1000), (2, 3 * CHUNK + 5)])
def test_moments_random(B, N):
    """fp32 data: each entry within 2 N 2^-53 sum |w a b| of the twin, the bound for two orders of summation."""
    rng = np.random.default_rng(N)
    p, q = rng.normal(size=(2, B, N, 3)).astype(np.float32)
    w = rng.uniform(0.1, 2.0, (B, N)).astype(np.float32)
    got, want = abi_moments(p, q, w), REG.rigid_moments(p, q, w)
    size = REG.rigid_moments(np.abs(p), np.abs(q), w)
    size[:, 16] = want[:, 16]          # its terms are not negative
    bound = 2.0 * N * 2.0 ** -53 * size
    print(f"REGISTRATION_MEASURED moments {B} x {N}: largest |device - twin| / bound = {np.max(np.abs(got - want) / bound):.3g}")
    assert (np.abs(got - want) <= bound).all()


def test_moments_skip_rows_and_repeat_bit_for_bit(eng):
    rng = np.random.default_rng(7)
    B, N = 2, 2 * CHUNK + 77
    p, q = rng.normal(size=(2, B, N, 3)).astype(np.float32)
    w = rng.uniform(0.5, 1.5, (B, N)).astype(np.float32)
    skip = rng.choice(N, 60, replace=False)
    w[0, skip[:10]], w[1, skip[10:20]], w[0, skip[20:25]], w[1, skip[25:30]] = 0.0, -1.0, np.nan, np.inf
    p[0, skip[30:40], 1], q[1, skip[40:50], 2], p[1, skip[50:60], 0] = np.nan, np.inf, -np.inf
    first = abi_moments(p, q, w)
    keep = np.isfinite(w) & (w > 0) & np.isfinite(p).all(-1) & np.isfinite(q).all(-1)
    assert first[0, 0] == pytest.approx(w[0][keep[0]].astype(np.float64).sum(), rel=1e-13) and keep.sum() == 2 * N - 60
    clean = REG.rigid_moments(np.where(keep[..., None], p, 0), np.where(keep[..., None], q, 0), np.where(keep, w, 0))
    assert np.array_equal(REG.rigid_moments(p, q, w), clean) and np.isfinite(first).all()
    assert np.allclose(first, clean, rtol=0, atol=2.0 * N * 2.0 ** -53 * np.abs(clean).max() * 8)
    assert np.array_equal(abi_moments(p, q, w), first)
    assert np.array_equal(abi_moments(p, q, w, scratch_fill=float("nan")), first) and np.array_equal(abi_moments(p, q, w, scratch_fill=1e300), first)
    through = eng.rigid_moments(dev(p), dev(q), dev(w))
    assert through.dtype == torch.float64 and through.is_cuda and np.array_equal(through.cpu().numpy(), first)
    assert np.array_equal(eng.rigid_moments(dev(p[0]), dev(q[0]), dev(w[0])).cpu().numpy(), first[0])
    empty = eng.rigid_moments(dev(p[:, :0]), dev(q[:, :0]))
    assert empty.shape == (2, 17) and not bool(empty.any())


# ---- rigid_fit and track_rigid ---------------------------------------------------------------------------------------------------------
def within_ulp(got, want, floor=0.0):
    """|got - want| <= one fp32 unit in the last place of the larger of the two (or ``floor``, where given)."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    tol = np.maximum(np.spacing(np.maximum(np.abs(got), np.abs(want))).astype(np.float64), floor)
    return bool((np.abs(got.astype(np.float64) - want.astype(np.float64)) <= tol).all())


def fit_against_twin(eng, p, q, w, what):
    """Engine.rigid_fit against the twin within 16 max(s, 2^-50), s = the twin's own spread over 8 orders of its rows."""
    out = eng.rigid_fit(dev(p), dev(q), None if w is None else dev(w))
    want = REG.rigid_fit(p, q, w)
    sel = lambda a, perm: a[..., perm, :] if a.ndim == 3 else a[perm]
    spread = permutation_spread(lambda perm: REG.rigid_fit(sel(p, perm), sel(q, perm), None if w is None else w[..., perm]), p.shape[-2],
                                ("rotation", "translation"))
    dist = max(float(np.abs(out[k].cpu().numpy() - want[k]).max()) for k in ("rotation", "translation"))
    print(f"REGISTRATION_MEASURED {what}: twin spread over 8 row orders {spread:.3g}, device - twin {dist:.3g}, bound {measured_tolerance(spread):.3g}")
    assert dist <= measured_tolerance(spread), what
    assert all(out[k].dtype == torch.float64 and out[k].is_cuda for k in ("rotation", "translation", "rmse", "weight")) and out["valid"].dtype == torch.bool
    assert np.array_equal(out["valid"].cpu().numpy(), want["valid"]) and np.array_equal(out["weight"].cpu().numpy(), want["weight"])
    assert is_rotation(out["rotation"].cpu().numpy())
    rmse, rmse_twin = out["rmse"].cpu().numpy(), want["rmse"]
    assert np.allclose(rmse, rmse_twin, rtol=1e-6, atol=2.0 ** -24)          # of fp32 rows: a flipped rounding of one moves it this little
    return out, want


def test_rigid_fit_against_the_twin(eng):
    p, q, R0, t0 = random_cloud(1500, 11, batches=3)
    q = q.astype(np.float32)
    w = np.random.default_rng(12).uniform(0.25, 2.0, (3, 1500)).astype(np.float32)
    out, _ = fit_against_twin(eng, np.broadcast_to(p, (3, 1500, 3)), q, w, "rigid_fit of a 3 x 1500 cloud")
    for b in range(3):
        assert max(motion_error(out["rotation"][b].cpu().numpy(), out["translation"][b].cpu().numpy(), R0[b], t0[b])) < 1e-7
    single, _ = fit_against_twin(eng, p, q[1], None, "rigid_fit, unbatched")
    assert single["rotation"].shape == (3, 3) and single["rmse"].shape == ()
    shared = eng.rigid_fit(dev(p), dev(q), dev(w))          # one [N,3] p against three q
    assert torch.equal(shared["rotation"], out["rotation"]) and torch.equal(shared["translation"], out["translation"])
    again = eng.rigid_fit(dev(p), dev(q), dev(w))
    assert all(torch.equal(again[k], shared[k]) for k in shared)


def test_rigid_fit_reflection_and_invalid_cases(eng):
    p, q = mirrored_plane()
    out, want = fit_against_twin(eng, p, q, None, "rigid_fit of a mirrored planar set")
    R = out["rotation"].cpu().numpy()
    assert bool(out["valid"]) and np.linalg.det(R) > 0.999999 and float(out["rmse"]) < 1e-6
    p3 = random_cloud(80, 6)[0]
    solid, _ = fit_against_twin(eng, p3, p3 * np.float32([-1.0, 1.0, 1.0]), None, "rigid_fit of a mirrored cloud")
    assert bool(solid["valid"]) and np.linalg.det(solid["rotation"].cpu().numpy()) > 0.999999 and float(solid["rmse"]) > 0.1
    for name, (a, b, w) in INVALID_CASES.items():
        got = eng.rigid_fit(dev(a), dev(b), None if w is None else dev(w))
        twin = REG.rigid_fit(a, b, w)
        assert not bool(got["valid"]) and torch.equal(got["rotation"].cpu(), torch.eye(3, dtype=torch.float64)), name
        assert np.allclose(got["translation"].cpu().numpy(), twin["translation"], rtol=0, atol=2.0 ** -50), name
        assert float(got["weight"]) == twin["weight"] and float(got["rmse"]) == pytest.approx(float(twin["rmse"]), rel=1e-6, abs=2.0 ** -24), name


@pytest.mark.parametrize("weighted", [False, True])
def test_track_rigid_against_the_twin(eng, weighted):
    v, f = bumpy(19, 15)          # V = 285: no multiple of the block
    track = rigid_track(v, f, scaled=True)
    w = np.linspace(0.5, 1.5, len(v)).astype(np.float32) if weighted else None
    want = REG.track_rigid(track, weights=w)
    out = eng.track_rigid(dev(track["vertices"]), weights=None if w is None else dev(w))
    assert set(out) == {"rotation", "translation", "rmse", "valid", "residual", "residual_norm"}
    x = track["vertices"]
    spread = permutation_spread(lambda perm: REG.track_rigid(x[:, perm], weights=None if w is None else w[perm]), len(v), ("rotation", "translation"))
    dist = max(float(np.abs(out[k].cpu().numpy() - want[k]).max()) for k in ("rotation", "translation"))
    print(f"REGISTRATION_MEASURED track_rigid (weighted: {weighted}): twin spread over 8 row orders {spread:.3g}, device - twin {dist:.3g}, "
          f"bound {measured_tolerance(spread):.3g}")
    assert dist <= measured_tolerance(spread)
    assert bool(out["valid"].all()) and is_rotation(out["rotation"].cpu().numpy())
    # the residual is a difference of O(1) fp64 values that agree to a few 2^-53: below 2^-48 it is rounding in either implementation
    assert within_ulp(out["residual_norm"].cpu().numpy(), want["residual_norm"], floor=2.0 ** -48)
    assert within_ulp(out["residual"].cpu().numpy(), want["residual"], floor=2.0 ** -48)
    assert out["residual"].dtype == torch.float32 and out["residual"].shape == (3, 285, 3) and out["residual_norm"].shape == (3, 285)
    assert float(out["residual_norm"][:2].max()) < 1e-14 and float(out["residual_norm"][2].max()) > 0.1
    assert np.allclose(out["rmse"].cpu().numpy(), want["rmse"], rtol=1e-6, atol=2.0 ** -24)
    other = eng.track_rigid(dev(track["vertices"]), reference=-1, weights=None if w is None else dev(w))
    twin_other = REG.track_rigid(track, reference=2, weights=w)
    assert np.abs(other["rotation"].cpu().numpy() - twin_other["rotation"]).max() <= measured_tolerance(spread)
    again = eng.track_rigid(dev(track["vertices"]), weights=None if w is None else dev(w))
    assert all(torch.equal(again[k], out[k]) for k in out)


def test_rigid_apply_against_the_twin(eng):
    p, _, R0, t0 = random_cloud(777, 21, batches=3)
    got = eng.rigid_apply(dev(R0), dev(t0), dev(p))          # one p, three motions
    want = REG.rigid_apply(R0, t0, p)
    assert got.shape == (3, 777, 3) and got.dtype == torch.float32 and within_ulp(got.cpu().numpy(), want)
    print(f"REGISTRATION_MEASURED rigid_apply: {int((got.cpu().numpy() != want).sum())} of {want.size} fp32 coordinates differ from the twin")
    each = eng.rigid_apply(dev(R0), dev(t0), dev(want))      # three sets of rows
    assert within_ulp(each.cpu().numpy(), REG.rigid_apply(R0, t0, want))
    one = eng.rigid_apply(dev(R0[1]), dev(t0[1]), dev(p))
    assert one.shape == (777, 3) and torch.equal(one, got[1])
    assert eng.rigid_apply(dev(R0), dev(t0), dev(p[:0])).shape == (3, 0, 3)
    for bad in ((dev(R0[:, :2]), dev(t0), dev(p)), (dev(R0), dev(t0[:2]), dev(p)), (dev(R0), dev(t0), dev(p[:, :2])), (dev(R0).cpu(), dev(t0), dev(p)),
                (dev(R0), dev(t0), dev(np.zeros((2, 5, 3), np.float32)))):
        with pytest.raises(EndoSurfHipError):
            eng.rigid_apply(*bad)


# ---- ICP -----------------------------------------------------------------------------------------------------------------------------------
def run_icp(eng, name, **kw):
    p, v, f, _, _, _ = icp_case(name)
    args = dict(tol=1e-6, max_distance=ICP_CASES[name][3])
    args.update(kw)
    return eng.icp(dev(p), dev(v), dev(f), **args)


@pytest.mark.parametrize("name", list(ICP_CASES))
def test_icp_plane(eng, name):
    p, v, f, R0, t0, kept = icp_case(name)
    want = twin_icp(name, tol=1e-6)
    out = run_icp(eng, name)
    angle, shift = motion_error(out["rotation"].cpu().numpy(), out["translation"].cpu().numpy(), R0, t0)
    print(f"REGISTRATION_MEASURED icp plane {name}: {out['iterations']} iterations (twin {want['iterations']}), angle error {angle:.3g} rad, "
          f"translation error {shift:.3g}, rmse {out['rmse']:.3g}, inliers {out['inliers']}")
    assert out["status"] == want["status"] == REG.CONVERGED and out["iterations"] <= want["iterations"] + 1 and out["step"] < 1e-6
    assert out["inliers"] == want["inliers"] == int(kept.sum())
    assert angle <= RECOVERY and shift <= RECOVERY
    assert out["rotation"].dtype == torch.float64 and out["rotation"].is_cuda and out["points"].dtype == torch.float32 and out["triangle"].dtype == torch.int32
    assert np.array_equal(out["distance"].cpu().numpy() > 0.25, ~kept) and np.array_equal(want["distance"] > 0.25, ~kept)
    assert bool((out["triangle"] >= 0).all())
    assert out["rmse"] == pytest.approx(want["rmse"], rel=0.5, abs=1e-7)          # both are rounding of fp32 rows: the same size
    for poll in (1, 3, 4):
        again = run_icp(eng, name, poll=poll)
        assert torch.equal(again["rotation"], out["rotation"]) and torch.equal(again["translation"], out["translation"]), poll
        assert again["iterations"] == out["iterations"] and torch.equal(again["points"], out["points"]) and again["rmse"] == out["rmse"]
    seeded = run_icp(eng, name, init=(R0, t0))
    assert seeded["status"] == REG.CONVERGED and seeded["iterations"] <= 2


def test_icp_other_modes(eng):
    gv, gf = grid_mesh(5, 5)
    c = gv[gf].mean(1).astype(np.float32)
    flat = eng.icp(dev(c), dev(gv), dev(gf))
    assert flat["status"] == REG.DEGENERATE and flat["iterations"] == 0 and flat["inliers"] == len(c) and flat["rmse"] == 0.0
    assert torch.equal(flat["rotation"].cpu(), torch.eye(3, dtype=torch.float64)) and not bool(flat["translation"].any())
    seed = (REG.rodrigues([0.0, 0.0, 0.25]), np.zeros(3))
    kept = eng.icp(dev(c), dev(gv), dev(gf), init=seed, poll=1)
    assert kept["status"] == REG.DEGENERATE and np.array_equal(kept["rotation"].cpu().numpy(), seed[0])
    for method in ("plane", "point"):
        none = eng.icp(dev(c[:0]), dev(gv), dev(gf), method=method)
        assert none["status"] == REG.DEGENERATE and none["inliers"] == 0 and none["points"].shape == (0, 3)
        bare = eng.icp(dev(c), dev(gv), dev(gf[:0]), method=method)
        assert bare["status"] == REG.DEGENERATE and bare["inliers"] == 0 and bool((bare["triangle"] == -1).all())
    two = run_icp(eng, "large", max_iters=2)
    assert two["status"] == REG.MAX_ITERS and two["iterations"] == 2
    twin_two = REG.icp(*icp_case("large")[:3], max_iters=2)
    assert np.abs(two["rotation"].cpu().numpy() - twin_two["rotation"]).max() < 1e-12
    # point-to-point: 5 fixed iterations against the twin's transform after 5, by the measured rule
    p, v, f, _, _, _ = icp_case("small")
    want = REG.icp(p, v, f, method="point", tol=0.0, max_iters=5)
    out = eng.icp(dev(p), dev(v), dev(f), method="point", tol=0.0, max_iters=5)
    assert out["status"] == REG.MAX_ITERS and out["iterations"] == 5
    spread = permutation_spread(lambda perm: REG.icp(p[perm], v, f, method="point", tol=0.0, max_iters=5), len(p), ("rotation", "translation"))
    dist = max(float(np.abs(out[k].cpu().numpy() - want[k]).max()) for k in ("rotation", "translation"))
    print(f"REGISTRATION_MEASURED icp point, 5 iterations: twin spread over 8 row orders {spread:.3g}, device - twin {dist:.3g}, "
          f"bound {measured_tolerance(spread):.3g}")
    assert dist <= measured_tolerance(spread)
    assert out["rmse"] == pytest.approx(want["rmse"], rel=1e-6)
    for bad in (dict(method="planes"), dict(poll=0), dict(max_iters=-1), dict(max_distance=-1.0), dict(init=(np.eye(2), np.zeros(3)))):
        with pytest.raises(EndoSurfHipError):
            run_icp(eng, "small", **bad)


def test_bad_arguments_return_error_codes():
    """Status 1 with a message that names the argument, before anything is launched (host addresses, never dereferenced); nothing to
    do is status 0 with null buffers."""
    lib = _lib.load()
    buf = np.zeros(64, np.float64)
    b = buf.ctypes.data
    odd = b + 4

    def fails(status, word):
        assert status == 1 and word in lib.es_last_error(), (status, lib.es_last_error())
    assert lib.es_rigid_scratch_bytes(-1, 4) == -1 and b"negative" in lib.es_last_error()
    assert lib.es_rigid_scratch_bytes(1, -4) == -1 and b"negative" in lib.es_last_error()
    assert lib.es_rigid_scratch_bytes(1, (1 << 31) // 3 + 1) == -1 and b"2^31" in lib.es_last_error()
    assert lib.es_rigid_scratch_bytes(1 << 20, 1 << 20) == -1 and b"2^31" in lib.es_last_error()
    fails(lib.es_rigid_moments(None, b, None, 1, 4, 0, b, b, None), b"p, q")
    fails(lib.es_rigid_moments(b, b, None, 1, 4, 0, None, b, None), b"scratch")
    fails(lib.es_rigid_moments(b, b, None, 1, 4, 0, odd, b, None), b"aligned")
    fails(lib.es_rigid_moments(b, b, None, 1, 4, 0, b, None, None), b"out")
    fails(lib.es_rigid_moments(b, b, None, -1, 4, 0, b, b, None), b"negative")
    fails(lib.es_rigid_moments(b, b, None, 1, -4, 0, b, b, None), b"negative")
    fails(lib.es_rigid_moments(b, b, None, 1, 1 << 40, 0, b, b, None), b"2^31")
    fails(lib.es_rigid_solve(None, 1, b, b, b, None, None), b"moments")
    fails(lib.es_rigid_solve(b, 1, None, b, b, None, None), b"rotation")
    fails(lib.es_rigid_solve(b, -1, b, b, b, None, None), b"negative")
    fails(lib.es_rigid_rmse(b, 1, None, None), b"rmse")
    fails(lib.es_rigid_rmse(b, -1, b, None), b"negative")
    fails(lib.es_rigid_apply(b, b, b, 1, 4, 5, b, None, None, None, None), b"p_batch_stride")
    fails(lib.es_rigid_apply(b, b, b, 1, 4, 12, None, None, None, None, None), b"no output")
    fails(lib.es_rigid_apply(b, b, b, 1, 4, 12, None, None, b, None, None), b"need q")
    fails(lib.es_rigid_apply(None, b, b, 1, 4, 12, b, None, None, None, None), b"rotation")
    fails(lib.es_rigid_apply(odd, b, b, 1, 4, 12, b, None, None, None, None), b"aligned")
    fails(lib.es_rigid_apply(b, b, b, 1, -4, 0, b, None, None, None, None), b"negative")
    fails(lib.es_icp_normal_equations(None, b, b, b, b, b, 4, 2, 3, -1.0, b, b, None), b"x, closest")
    fails(lib.es_icp_normal_equations(b, b, b, b, None, b, 4, 2, 3, -1.0, b, b, None), b"vertices")
    fails(lib.es_icp_normal_equations(b, b, b, b, b, b, -4, 2, 3, -1.0, b, b, None), b"negative")
    fails(lib.es_icp_normal_equations(b, b, b, b, b, b, 4, 2, -3, -1.0, b, b, None), b"negative")
    fails(lib.es_icp_normal_equations(b, b, b, b, b, b, 1 << 31, 2, 3, -1.0, b, b, None), b"2^31")
    fails(lib.es_icp_normal_equations(b, b, b, b, b, b, 4, 2, 3, float("nan"), b, b, None), b"NaN")
    fails(lib.es_icp_normal_equations(b, b, b, b, b, b, 4, 2, 3, -1.0, odd, b, None), b"aligned")
    fails(lib.es_icp_normal_equations(b, b, b, b, b, b, 4, 2, 3, -1.0, b, None, None), b"out")
    fails(lib.es_icp_update(b, 2, 1e-6, b, None), b"method")
    fails(lib.es_icp_update(b, -1, 1e-6, b, None), b"method")
    fails(lib.es_icp_update(None, 1, 1e-6, b, None), b"sums")
    fails(lib.es_icp_update(b, 1, 1e-6, None, None), b"state")
    fails(lib.es_icp_update(b, 1, float("nan"), b, None), b"tol")
    assert lib.es_rigid_moments(None, None, None, 0, 4, 0, None, None, None) == 0 and lib.es_rigid_solve(None, 0, None, None, None, None, None) == 0
    assert lib.es_rigid_apply(None, None, None, 3, 0, 0, None, None, None, None, None) == 0 and lib.es_rigid_rmse(None, 0, None, None) == 0


# ---- the renderer ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def R():
    from gpu_util import renderer_for
    return renderer_for(11, "trained", True)


@pytest.mark.parametrize("name", list(ICP_CASES))
def test_register_points_through_the_renderer(R, name):
    """Host inputs, a mesh dict: the result is Engine.icp's on the same values, and the twin's status, inliers and pattern."""
    p, v, f, R0, t0, kept = icp_case(name)
    want = twin_icp(name, tol=1e-6)
    out = R.register_points(p, {"vertices": v, "triangles": f}, max_distance=ICP_CASES[name][3])
    direct = R.engine.icp(dev(p), dev(v), dev(f), max_distance=ICP_CASES[name][3])
    assert torch.equal(out["rotation"], direct["rotation"]) and torch.equal(out["translation"], direct["translation"]) and out["rotation"].is_cuda
    assert out["status"] == want["status"] and out["inliers"] == want["inliers"] and out["iterations"] <= want["iterations"] + 1
    assert np.array_equal(out["distance"].cpu().numpy() > 0.25, ~kept)
    assert max(motion_error(out["rotation"].cpu().numpy(), out["translation"].cpu().numpy(), R0, t0)) <= RECOVERY
    pair = R.register_points(dev(p), (dev(v), dev(f)), max_distance=ICP_CASES[name][3], poll=3)
    assert torch.equal(pair["rotation"], out["rotation"]) and torch.equal(pair["points"], out["points"])


def test_renderer_track_rigid_and_register_mesh(R):
    n = 17
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    verts = (np.array([-0.2, -0.25, 0.1])[None] + i.reshape(-1, 1) * np.array([0.02, 0.004, -0.006])[None]
             + j.reshape(-1, 1) * np.array([-0.002, 0.018, 0.008])[None]).astype(np.float32)
    tris = grid_mesh(n)[1]
    track = R.track_mesh(dev(verts), dev(tris), t=0.3, times=[0.3, 0.5, 0.9])
    out = R.track_rigid(track)
    assert set(out) == set(track) | {"rotation", "translation", "rmse", "valid", "residual", "residual_norm"} and out["triangles"] is track["triangles"]
    assert out["rotation"].shape == (3, 3, 3) and out["rotation"].dtype == torch.float64 and out["residual"].shape == (3, 289, 3) and out["residual"].is_cuda
    direct = R.engine.track_rigid(track["vertices"])
    assert all(torch.equal(direct[k], out[k]) for k in direct)
    assert float(out["rmse"][0]) < 1e-7 and bool(out["valid"].all())          # the reference frame onto itself
    host = R.track_rigid(track["vertices"].cpu().numpy(), weights=np.ones(289, np.float32))
    assert set(host) == set(direct) and torch.equal(host["residual"], out["residual"])
    want = REG.track_rigid(track["vertices"].cpu().numpy())
    assert np.abs(out["rotation"].cpu().numpy() - want["rotation"]).max() < 1e-9
    print(f"REGISTRATION_MEASURED tracked patch: rmse over the frames {out['rmse'].cpu().numpy().tolist()}")
    # a mesh registered onto another
    p, v, f, R0, t0, _ = icp_case("small")
    src_v, src_f = bumpy(17, 13)
    moved = ((src_v.astype(np.float64) - t0) @ R0).astype(np.float32)
    inner = (src_v[:, 0] >= 0.125) & (src_v[:, 0] <= 0.875) & (src_v[:, 1] >= 0.125) & (src_v[:, 1] <= 0.625)
    reg = R.register_mesh({"vertices": moved[inner], "triangles": src_f}, (v, f))
    assert reg["status"] == REG.CONVERGED and reg["triangles"] is src_f and reg["vertices"] is reg["points"]
    assert max(motion_error(reg["rotation"].cpu().numpy(), reg["translation"].cpu().numpy(), R0, t0)) <= RECOVERY
    assert float((reg["vertices"] - dev(src_v[inner])).abs().max()) < 1e-6
