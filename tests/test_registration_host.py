"""CPU: endosurf_amd.registration, the numpy specification of csrc/register.hip, on its own -- the rigid fit (Kabsch) with its validity
rule, the rigid part of a track, and ICP against the triangles of a mesh."""
import math

import numpy as np
import pytest

from endosurf_amd import registration as REG
from geodesic_util import bumpy, grid_mesh, rigid_track, ROT_X, ROT_Z
from registration_util import (ICP_CASES, INVALID_CASES, RECOVERY, icp_case, is_rotation, mirrored_plane, motion_error, random_cloud,
                               rotation, twin_icp)


def test_moments_are_the_sums_they_name():
    rng = np.random.default_rng(0)
    p, q = rng.normal(size=(2, 2, 50, 3)).astype(np.float32)
    w = rng.uniform(0.5, 2.0, (2, 50)).astype(np.float32)
    m = REG.rigid_moments(p, q, w)
    assert m.shape == (2, 17) and m.dtype == np.float64
    pd, qd, wd = p.astype(np.float64), q.astype(np.float64), w.astype(np.float64)
    want = np.concatenate([wd.sum(1)[:, None], np.einsum("bn,bni->bi", wd, pd), np.einsum("bn,bni->bi", wd, qd),
                           np.einsum("bn,bni,bnj->bij", wd, pd, qd).reshape(2, 9), np.einsum("bn,bni->b", wd, (pd - qd) ** 2)[:, None]], 1)
    assert np.allclose(m, want, rtol=1e-13, atol=1e-13)
    assert np.array_equal(REG.rigid_moments(p[0], q[0], w[0]), m[0])                       # unbatched
    assert np.array_equal(REG.rigid_moments(p, q, w[0])[1], REG.rigid_moments(p[1], q[1], w[0]))          # a shared [N] weight
    assert np.array_equal(REG.rigid_moments(p, q)[0], REG.rigid_moments(p[0], q[0], np.ones(50)))


def test_fit_recovers_a_known_motion():
    p, q, R0, t0 = random_cloud(500, 1)
    fit = REG.rigid_fit(p, q.astype(np.float32))
    assert fit["valid"] and fit["weight"] == 500.0 and is_rotation(fit["rotation"])
    angle, shift = motion_error(fit["rotation"], fit["translation"], R0, t0)
    assert angle < 1e-7 and shift < 1e-7 and fit["rmse"] < 2e-7          # q was rounded to fp32: 6e-8 per coordinate
    pb, qb, Rb, tb = random_cloud(300, 2, batches=3)
    fb = REG.rigid_fit(pb[None], qb.astype(np.float32))
    assert fb["rotation"].shape == (3, 3, 3) and fb["translation"].shape == (3, 3) and fb["valid"].all()
    for b in range(3):
        one = REG.rigid_fit(pb, qb[b].astype(np.float32))
        assert np.array_equal(one["rotation"], fb["rotation"][b]) and np.array_equal(one["translation"], fb["translation"][b])
        assert max(motion_error(fb["rotation"][b], fb["translation"][b], Rb[b], tb[b])) < 1e-7


def test_fit_returns_a_proper_rotation_where_the_best_map_is_a_reflection():
    p, q = mirrored_plane()
    fit = REG.rigid_fit(p, q)
    assert fit["valid"] and is_rotation(fit["rotation"]) and np.linalg.det(fit["rotation"]) > 0.999999
    assert fit["rmse"] < 1e-6          # in the plane a mirror image is also half a turn about the mirror line: a proper rotation fits
    mirror = rotation([0.3, -0.2, 0.5]) @ np.diag([-1.0, 1.0, 1.0])
    assert np.abs(fit["rotation"] - mirror @ np.diag([1.0, 1.0, -1.0])).max() < 1e-6
    # it is the minimiser among proper rotations: no nearby rotation does better
    x = p.astype(np.float64) - p.mean(0)
    y = q.astype(np.float64) - q.mean(0)
    cost = lambda R: float(((x @ R.T - y) ** 2).sum())
    base = cost(fit["rotation"])
    rng = np.random.default_rng(3)
    assert all(cost(rotation(rng.normal(size=3) * 1e-3) @ fit["rotation"]) >= base * (1 - 1e-12) for _ in range(50))
    # a mirrored cloud with depth: no rotation undoes it, the answer is still proper and still the minimiser among rotations
    p3, _, _, _ = random_cloud(80, 6)
    solid = REG.rigid_fit(p3, (p3 * np.float32([-1.0, 1.0, 1.0])))
    assert solid["valid"] and is_rotation(solid["rotation"]) and solid["rmse"] > 0.1
    x3 = p3.astype(np.float64) - p3.astype(np.float64).mean(0)
    y3 = x3 * [-1.0, 1.0, 1.0]
    cost3 = lambda R: float(((x3 @ R.T - y3) ** 2).sum())
    assert all(cost3(rotation(rng.normal(size=3) * 1e-3) @ solid["rotation"]) >= cost3(solid["rotation"]) * (1 - 1e-12) for _ in range(50))
    # planar data without the mirror: valid, exact recovery
    turned = (p.astype(np.float64) @ rotation([0.3, -0.2, 0.5]).T + [0.1, 0.2, -0.3]).astype(np.float32)
    flat = REG.rigid_fit(p, turned)
    assert flat["valid"] and max(motion_error(flat["rotation"], flat["translation"], rotation([0.3, -0.2, 0.5]), [0.1, 0.2, -0.3])) < 1e-6


def test_fit_ignores_rows_without_weight_and_non_finite_rows():
    p, q, _, _ = random_cloud(40, 4)
    q = q.astype(np.float32)
    keep = np.ones(40, bool)
    keep[[3, 7, 11, 19, 25]] = False
    w = np.ones(40, np.float32)
    p2, q2 = p.copy(), q.copy()
    w[3], w[7] = 0.0, -1.0
    w[11] = np.nan
    p2[19, 1], q2[25, 2] = np.inf, np.nan
    got, want = REG.rigid_fit(p2, q2, w), REG.rigid_fit(p[keep], q[keep])
    assert got["weight"] == 35.0
    for k in ("rotation", "translation", "rmse"):
        assert np.allclose(got[k], want[k], rtol=0, atol=1e-14), k
    assert np.array_equal(REG.rigid_moments(p2, q2, w), REG.rigid_moments(np.where(keep[:, None], p, 0), np.where(keep[:, None], q, 0), keep * 1.0))


@pytest.mark.parametrize("name", list(INVALID_CASES))
def test_fit_invalid_cases(name):
    p, q, w = INVALID_CASES[name]
    fit = REG.rigid_fit(p, q, w)
    assert not fit["valid"] and np.array_equal(fit["rotation"], np.eye(3))
    if name == "no_weight":
        assert fit["weight"] == 0.0 and np.array_equal(fit["translation"], np.zeros(3)) and fit["rmse"] == 0.0
    else:
        assert np.allclose(fit["translation"], q.astype(np.float64).mean(0) - p.astype(np.float64).mean(0), atol=1e-15)


def test_track_rigid_on_rigid_frames():
    v, f = bumpy(9, 7)
    track = rigid_track(v, f)
    out = REG.track_rigid(track)
    assert set(out) == set(track) | {"rotation", "translation", "rmse", "valid", "residual", "residual_norm"} and out["triangles"] is f
    assert out["residual"].shape == (3, 63, 3) and out["residual"].dtype == np.float32 and out["residual_norm"].shape == (3, 63)
    assert out["valid"].all() and out["rmse"].shape == (3,)
    known = [(np.eye(3), np.zeros(3)), (ROT_Z, np.array([0.25, -0.5, 0.125])), (ROT_Z @ ROT_X, np.array([-0.375, 0.25, 0.5]))]
    for fr, (R0, t0) in enumerate(known):
        assert max(motion_error(out["rotation"][fr], out["translation"][fr], R0, t0)) < 1e-14, fr
    assert np.abs(out["residual"]).max() < 1e-14 and out["residual_norm"].max() < 1e-14
    # another reference frame: the motions compose
    back = REG.track_rigid(track["vertices"], reference=1)
    assert set(back) == {"rotation", "translation", "rmse", "valid", "residual", "residual_norm"}
    assert max(motion_error(back["rotation"][0], back["translation"][0], ROT_Z.T, -ROT_Z.T @ [0.25, -0.5, 0.125])) < 1e-14
    with pytest.raises(ValueError):
        REG.track_rigid(track, reference=3)


def test_track_rigid_leaves_the_deformation():
    v, f = bumpy(9, 7)
    track = rigid_track(v, f, scaled=True)
    w = np.linspace(0.5, 1.5, len(v)).astype(np.float32)
    for weights in (None, w):
        out = REG.track_rigid(track, weights=weights)
        assert out["residual_norm"][:2].max() < 1e-14 and out["residual_norm"][2].max() > 0.1
        assert max(motion_error(out["rotation"][2], np.zeros(3), np.eye(3), np.zeros(3))) < 1e-14          # a scaling turns nothing
        x = track["vertices"].astype(np.float64)
        ww = np.ones(len(v)) if weights is None else weights.astype(np.float64)
        for fr in range(3):
            moved = REG.rigid_apply(out["rotation"][fr], out["translation"][fr], x[0]).astype(np.float64)
            direct = math.sqrt(float((ww * ((x[fr] - moved) ** 2).sum(1)).sum() / ww.sum()))
            assert out["rmse"][fr] == pytest.approx(direct, rel=1e-12, abs=1e-300), fr
            assert np.allclose(np.linalg.norm(out["residual"][fr], axis=1), out["residual_norm"][fr], rtol=1e-6, atol=1e-30)
        # the weighted mean of the residual vanishes: the translation is the least-squares one
        assert np.abs((ww[:, None] * out["residual"][2].astype(np.float64)).sum(0) / ww.sum()).max() < 1e-7


@pytest.mark.parametrize("name", list(ICP_CASES))
def test_icp_plane_recovers_the_motion(name):
    p, v, f, R0, t0, kept = icp_case(name)
    out = twin_icp(name)
    angle, shift = motion_error(out["rotation"], out["translation"], R0, t0)
    print(f"REGISTRATION_MEASURED twin icp {name}: {out['iterations']} iterations, angle error {angle:.3g} rad, translation error {shift:.3g}, "
          f"rmse {out['rmse']:.3g}, inliers {out['inliers']}")
    assert out["status"] == REG.CONVERGED and out["iterations"] <= 50 and out["step"] < 1e-7
    assert out["inliers"] == int(kept.sum())
    assert angle <= RECOVERY and shift <= RECOVERY
    assert np.array_equal(out["triangle"] >= 0, np.ones(192, bool))
    far = out["distance"] > 0.25
    assert np.array_equal(far, ~kept)          # the pushed rows stay 0.5 off the surface, everything else lies on it
    assert out["points"].dtype == np.float32 and np.array_equal(out["points"], REG.rigid_apply(out["rotation"], out["translation"], p))
    seeded = REG.icp(p, v, f, tol=1e-7, max_distance=ICP_CASES[name][3], init=(R0, t0))
    assert seeded["status"] == REG.CONVERGED and seeded["iterations"] <= 2


def test_icp_degenerate_systems():
    gv, gf = grid_mesh(5, 5)
    c = gv[gf].mean(1)
    out = REG.icp(c, gv, gf, method="plane")          # every normal is (0, 0, 1): three pivots are exactly 0
    assert out["status"] == REG.DEGENERATE and out["iterations"] == 0
    assert np.array_equal(out["rotation"], np.eye(3)) and np.array_equal(out["translation"], np.zeros(3))
    assert out["inliers"] == len(c) and out["rmse"] == 0.0
    seed = (rotation([0.0, 0.0, 0.25]), np.array([0.0, 0.0, 0.0]))
    kept = REG.icp(c, gv, gf, init=seed)
    assert kept["status"] == REG.DEGENERATE and np.array_equal(kept["rotation"], seed[0])
    for method in ("plane", "point"):
        none = REG.icp(np.zeros((0, 3), np.float32), gv, gf, method=method)
        assert none["status"] == REG.DEGENERATE and none["inliers"] == 0 and none["points"].shape == (0, 3)
        bare = REG.icp(c, gv, np.zeros((0, 3), np.int64), method=method)
        assert bare["status"] == REG.DEGENERATE and bare["inliers"] == 0 and (bare["triangle"] == -1).all()
    with pytest.raises(ValueError):
        REG.icp(c, gv, gf, method="planes")
    two = REG.icp(*icp_case("large")[:3], max_iters=2)
    assert two["status"] == REG.MAX_ITERS and two["iterations"] == 2
    assert {REG.CONVERGED, REG.MAX_ITERS, REG.DEGENERATE} == {0, 1, 2}


def test_icp_point_does_not_diverge():
    """Point-to-point slides along a smooth surface: it is not asked to converge, only to go downhill."""
    p, v, f, R0, t0, _ = icp_case("small")
    rmse = [REG.icp(p, v, f, method="point", tol=0.0, max_iters=k)["rmse"] for k in range(0, 21, 4)]
    assert all(b <= a for a, b in zip(rmse, rmse[1:])) and rmse[-1] < rmse[0]
    last = REG.icp(p, v, f, method="point", tol=0.0, max_iters=20)
    start = motion_error(np.eye(3), np.zeros(3), R0, t0)
    assert last["status"] == REG.MAX_ITERS and last["iterations"] == 20
    assert all(e <= s for e, s in zip(motion_error(last["rotation"], last["translation"], R0, t0), start))
    assert is_rotation(last["rotation"], 1e-13)
