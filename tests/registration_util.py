"""Helpers of the registration tests (tests/test_registration_host.py, tests/test_gpu_registration.py): the clouds with their known
motions, the ICP cases on ``geodesic_util.bumpy(17, 13)``, and the measures the recovered motions are held to."""
import functools

import numpy as np

from endosurf_amd import registration as REG
from geodesic_util import bumpy

RECOVERY = 2.0 ** -20          # 16 fp32 ulps of a unit coordinate: the coordinates are fp32 and the scene lies in the unit sphere


def rotation(rotvec):
    return REG.rodrigues(np.asarray(rotvec, np.float64))


def motion_error(R, t, R0, t0):
    """(angle of R R0^T in radians, |t - t0|)."""
    return REG.rotation_angle(np.asarray(R) @ np.asarray(R0).T), float(np.linalg.norm(np.asarray(t) - np.asarray(t0)))


def random_cloud(n, seed, batches=None):
    """fp32 points in the unit ball's box, and for each batch a known motion and the moved points (fp64, not rounded)."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
    if batches is None:
        R0, t0 = rotation(rng.uniform(-1.0, 1.0, 3)), rng.uniform(-0.5, 0.5, 3)
        return p, p.astype(np.float64) @ R0.T + t0, R0, t0
    R0 = np.stack([rotation(rng.uniform(-1.0, 1.0, 3)) for _ in range(batches)])
    t0 = rng.uniform(-0.5, 0.5, (batches, 3))
    return p, np.einsum("bij,nj->bni", R0, p.astype(np.float64)) + t0[:, None], R0, t0


def mirrored_plane(n=64, seed=5):
    """Planar points and their mirror image in the plane's own frame (x -> -x), then turned: the best orthogonal map is a reflection;
    the best proper rotation has det +1."""
    rng = np.random.default_rng(seed)
    p = np.concatenate([rng.uniform(-1.0, 1.0, (n, 2)), np.zeros((n, 1))], 1).astype(np.float32)
    q = (p.astype(np.float64) * [-1.0, 1.0, 1.0]) @ rotation([0.3, -0.2, 0.5]).T
    return p, q.astype(np.float32)


INVALID_CASES = {
    "no_weight": (np.eye(3, dtype=np.float32), np.eye(3, dtype=np.float32) + 1, np.zeros(3, np.float32)),
    "coincident": (np.full((5, 3), 0.25, np.float32), np.full((5, 3), 0.5, np.float32), None),
    "collinear": (np.outer(np.arange(6) / 8.0, [1.0, 2.0, -1.0]).astype(np.float32),
                  np.outer(np.arange(6) / 8.0, [0.0, 1.0, 1.0]).astype(np.float32) + np.float32(0.5), None),
}


# ---- the ICP cases -----------------------------------------------------------------------------------------------------------------------
ICP_CASES = {          # name -> (rotation vector, translation, push every tenth row 0.5 off the surface, max_distance)
    "small": ((0.02, -0.03, 0.04), (0.02, -0.015, 0.01), False, None),
    "large": ((0.1, 0.1, -0.1), (0.05, 0.05, -0.03), False, None),
    "outliers": ((0.1, 0.1, -0.1), (0.05, 0.05, -0.03), True, 0.1),
}


@functools.lru_cache(maxsize=None)
def icp_case(name):
    """(points [192,3] fp32, vertices, triangles, R0, t0, the rows not pushed): the cloud is the barycentres of the triangles of
    ``bumpy(17, 13)`` that lie at least 0.125 inside the boundary in x and y, every tenth optionally pushed 0.5 along z, taken out of
    place by the inverse of the motion (R0, t0) -- which is therefore the motion that lays the points back onto the mesh."""
    rotvec, t0, push, _ = ICP_CASES[name]
    v, f = bumpy(17, 13)
    c = v.astype(np.float64)[f].mean(1)
    c = c[(c[:, 0] >= 0.125) & (c[:, 0] <= 1.0 - 0.125) & (c[:, 1] >= 0.125) & (c[:, 1] <= 0.75 - 0.125)]
    assert len(c) == 192
    kept = np.ones(len(c), bool)
    if push:
        kept[::10] = False
        c = c + np.where(kept, 0.0, 0.5)[:, None] * [0.0, 0.0, 1.0]
    R0, t0 = rotation(rotvec), np.asarray(t0, np.float64)
    return ((c - t0) @ R0).astype(np.float32), v, f, R0, t0, kept


@functools.lru_cache(maxsize=None)
def twin_icp(name, method="plane", tol=1e-7, max_iters=50):
    """The twin's answer for a case, computed once."""
    p, v, f, _, _, _ = icp_case(name)
    return REG.icp(p, v, f, method=method, tol=tol, max_iters=max_iters, max_distance=ICP_CASES[name][3])


def permutation_spread(fn, n_rows, keys, seed=0, n=8):
    """The largest entry-wise spread of ``fn(perm)[key]`` over the identity and ``n`` random row permutations: how far the twin's own
    answer moves with the order of its sums."""
    rng = np.random.default_rng(seed)
    runs = [fn(np.arange(n_rows))] + [fn(rng.permutation(n_rows)) for _ in range(n)]
    return max(float(np.max(np.ptp(np.stack([np.asarray(r[k], np.float64) for r in runs]), axis=0))) for k in keys)


def measured_tolerance(spread):
    """16 x max(spread, 2^-50): the device uses another rotation solver and fused multiply-adds."""
    return 16.0 * max(spread, 2.0 ** -50)


def is_rotation(R, tol=1e-14):
    R = np.asarray(R, np.float64)
    return bool(np.abs(R @ np.swapaxes(R, -1, -2) - np.eye(3)).max() <= tol and np.all(np.abs(np.linalg.det(R) - 1.0) <= tol))
