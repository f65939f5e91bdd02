"""Shared by tests/test_cloud_host.py and tests/test_gpu_cloud.py: the point clouds of the neighbour-query tests and the analytic
RGB-D scene of the scene-normalisation tests."""
import numpy as np


def lattice_cloud(P=5000, seed=0):
    """Points on the lattice of multiples of 1/8 in [0, 8)^3, duplicates present (64^3 sites, the first P // 10 rows repeated at the
    end): every coordinate difference, square and sum below is exact in fp32, so every fp32 d2 is the true squared distance."""
    rng = np.random.default_rng(seed)
    p = rng.integers(0, 64, size=(P - P // 10, 3)).astype(np.float32) / 8
    return np.concatenate([p, p[:P // 10]])


def random_cloud(P, seed=1, scale=1.0):
    return (np.random.default_rng(seed).standard_normal((P, 3)) * scale).astype(np.float32)


def planar_cloud(P=300, seed=2):
    """z constant: the z axis of the grid is one cell."""
    p = np.random.default_rng(seed).random((P, 3)).astype(np.float32)
    p[:, 2] = 0.25
    return p


def collinear_cloud(P=300, seed=3):
    """on a line along x: two axes of one cell."""
    p = np.zeros((P, 3), np.float32)
    p[:, 0] = np.random.default_rng(seed).random(P).astype(np.float32) * 4
    p[:, 1], p[:, 2] = -1.5, 2.0
    return p


def with_bad_rows(p, seed=4):
    """``p`` with NaN / +inf / -inf planted in a tenth of its rows (one coordinate each)."""
    rng = np.random.default_rng(seed)
    q = p.copy()
    rows = rng.choice(len(q), max(1, len(q) // 10), replace=False)
    q[rows, rng.integers(0, 3, len(rows))] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), len(rows))
    return q


# ---- the analytic scene: a sphere of radius ~30 at distance ~100, three 40 x 48 frames, f = 60 --------------------------------------------
SCENE_H, SCENE_W, SCENE_F = 40, 48, 60.0
PLANTED_DEPTHS = (40.0, 55.0, 150.0)
PLANTED_PIXELS = ((2, 3), (37, 44), (3, 42))          # (row, column): image corners, off the sphere's silhouette
SPHERE_CENTRE = np.array([40.0, -30.0, 100.0])          # off the world's axes: no component of the scene's centre is a small difference
SCENE_ARGS = dict(radius_factor=4.0, nb_points=5, percentiles=(0.0, 100.0), down_sample=1.0)


def analytic_scene():
    """depths [3,40,48] fp32 (z-depth of the first hit of each pixel's ray on the frame's sphere, 0 beside it, three isolated
    background pixels planted per frame), intrinsics and camera-to-world poses [3,4,4] fp32; the cameras look along +z from about
    100 in front of the sphere, and camera position and sphere radius vary from frame to frame.
    Returns (depths, intrinsics, poses, planted [3,40,48] bool)."""
    H, W, f = SCENE_H, SCENE_W, SCENE_F
    K = np.array([[f, 0, (W - 1) * 0.5, 0], [0, f, (H - 1) * 0.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float64)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    rays = np.stack([(xs - K[0, 2]) / f, (ys - K[1, 2]) / f, np.ones_like(xs)], -1)          # camera frame, z = 1
    depths, poses, planted = [], [], np.zeros((3, H, W), bool)
    for i, (cam, rad) in enumerate((((0.0, 0.0, 0.0), 30.0), ((4.0, -2.0, 1.0), 28.5), ((-3.0, 3.0, -2.0), 32.0))):
        c2w = np.eye(4)
        c2w[:3, 3] = SPHERE_CENTRE * (1.0, 1.0, 0.0) + cam
        centre = SPHERE_CENTRE - c2w[:3, 3]          # the sphere's centre in the (unrotated) camera frame
        a, b, c = (rays * rays).sum(-1), -2 * (rays @ centre), centre @ centre - rad * rad
        disc = b * b - 4 * a * c
        z = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), 0.0)          # rays have z = 1: the parameter is the z-depth
        for (r, col), dep in zip(PLANTED_PIXELS, PLANTED_DEPTHS):
            assert z[r, col] == 0.0
            z[r, col] = dep
            planted[i, r, col] = True
        depths.append(z)
        poses.append(c2w)
    n = len(depths)
    return (np.stack(depths).astype(np.float32), np.tile(K[None], (n, 1, 1)).astype(np.float32), np.stack(poses).astype(np.float32), planted)
