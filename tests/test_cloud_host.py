"""CPU: the numpy twins of csrc/cloud.hip (meshing.self_nearest / radius_count / radius_outlier_mask) against scipy's cKDTree on a cloud
whose fp32 squared distances are exact, their edge cases, and the scene normalisation of endosurf_amd.data (depth_percentile,
scene_normalization, normalize_cameras, FrameSet.from_raw) on an analytic scene."""
import numpy as np
import pytest
import torch

from cloud_util import (PLANTED_DEPTHS, SCENE_ARGS, analytic_scene, collinear_cloud, lattice_cloud, planar_cloud, random_cloud, with_bad_rows)
from endosurf_amd import data as D
from endosurf_amd import meshing as M


@pytest.fixture(scope="module")
def lattice():
    from scipy.spatial import cKDTree
    p = lattice_cloud(5000)
    return p, cKDTree(p.astype(np.float64))


# ---- the twins against cKDTree ---------------------------------------------------------------------------------------------------------
def test_radius_count_equals_ckdtree_on_the_lattice(lattice):
    p, tree = lattice
    want = tree.query_ball_point(p.astype(np.float64), np.sqrt(1.25), return_length=True)
    d2 = ((p[:200, None].astype(np.float64) - p[None].astype(np.float64)) ** 2).sum(-1)
    assert (d2 == 1.25).any(), "no pair on the boundary (80 = 64 + 16 in units of 1/64)"
    got = M.radius_count(p, p, radius_sq=1.25)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert got.min() >= 1                                  # a row counts itself
    for cap in (1, 6):
        assert np.array_equal(M.radius_count(p, p, radius_sq=1.25, cap=cap), np.minimum(want, cap))
    q = (random_cloud(777, seed=5, scale=3.0) + 4).astype(np.float32)          # queries that are no rows, some outside the box
    assert np.array_equal(M.radius_count(q, p, radius=1.5), tree.query_ball_point(q.astype(np.float64), 1.5, return_length=True))


def test_self_nearest_equals_ckdtree_on_the_lattice(lattice):
    p, tree = lattice
    want = tree.query(p.astype(np.float64), k=2)[0][:, 1]
    dist, idx = M.self_nearest(p, chunk=1 << 20)          # (several chunks)
    assert dist.dtype == np.float32 and idx.dtype == np.int32
    assert np.array_equal(dist, np.sqrt((want * want).astype(np.float32)))          # want^2 is an exact fp32; the same correctly rounded root
    assert (dist[:500] == 0).all() and (dist[-500:] == 0).all()                     # the duplicated rows
    d2 = ((p[:, None] - p[None]) ** 2).sum(-1, dtype=np.float32)
    np.fill_diagonal(d2, np.inf)
    assert np.array_equal(idx, d2.argmin(1))                                        # the smallest index among the nearest
    assert (idx != np.arange(len(p))).all()


@pytest.mark.parametrize("P", [0, 1, 2])
def test_tiny_clouds(P):
    p = np.array([[1, 2, 3], [1, 2, 5]], np.float32)[:P]
    dist, idx = M.self_nearest(p)
    assert dist.shape == (P,) and idx.shape == (P,)
    if P == 2:
        assert dist.tolist() == [2.0, 2.0] and idx.tolist() == [1, 0]
    else:
        assert np.isinf(dist).all() and (idx == -1).all()
    q = np.array([[1, 2, 3], [9, 9, 9]], np.float32)
    assert M.radius_count(q, p, radius=2.0).tolist() == [P, 0]
    assert M.radius_count(p, p, radius_sq=0.0).tolist() == [1] * P
    assert M.radius_outlier_mask(p, 1, 2.0).tolist() == [P == 2] * P
    assert M.radius_count(np.zeros((0, 3), np.float32), p, radius=1.0).shape == (0,)


def test_identical_rows():
    p = np.tile(np.array([[0.5, -1.25, 3.0]], np.float32), (40, 1))
    dist, idx = M.self_nearest(p)
    assert (dist == 0).all() and idx.tolist() == [1] + [0] * 39
    assert (M.radius_count(p, p, radius_sq=0.0) == 40).all()
    assert (M.radius_count(p, p, radius_sq=0.0, cap=6) == 6).all()
    assert M.radius_outlier_mask(p, 39, 0.0).all() and not M.radius_outlier_mask(p, 40, 0.0).any()


def test_non_finite_rows():
    base = random_cloud(300, seed=7)
    p = with_bad_rows(base)
    bad = ~np.isfinite(p).all(1)
    assert bad.sum() == 30
    dist, idx = M.self_nearest(p)
    assert np.isinf(dist[bad]).all() and (idx[bad] == -1).all()
    good = np.nonzero(~bad)[0]
    d2, i2 = M.self_nearest(p[good])
    assert np.array_equal(dist[good], d2) and np.array_equal(idx[good], good[i2])          # the bad rows are as if absent
    n = M.radius_count(p, p, radius=0.5)
    assert (n[bad] == 0).all() and np.array_equal(n[good], M.radius_count(p[good], p[good], radius=0.5))
    assert not M.radius_outlier_mask(p, 0, 10.0)[bad].any() and M.radius_outlier_mask(p, 0, 10.0)[good].all()
    only_bad = p[bad]
    assert np.isinf(M.self_nearest(only_bad)[0]).all() and (M.radius_count(base, only_bad, radius_sq=np.inf) == 0).all()


@pytest.mark.parametrize("make", [planar_cloud, collinear_cloud])
def test_flat_clouds_against_ckdtree(make):
    from scipy.spatial import cKDTree
    p = make()
    tree = cKDTree(p.astype(np.float64))
    dist, idx = M.self_nearest(p)
    want, wi = tree.query(p.astype(np.float64), k=2)
    assert np.allclose(dist, want[:, 1], rtol=1e-6, atol=0) and (idx == wi[:, 1]).mean() > 0.99
    r = 0.2
    got, ref = M.radius_count(p, p, radius=r), tree.query_ball_point(p.astype(np.float64), r, return_length=True)
    assert (got != ref).mean() < 0.01 and np.abs(got - ref).max() <= 1          # (a pair at the radius to fp32 rounding may fall either way)


def test_cap_and_special_radii(lattice):
    p, _ = lattice
    q = np.concatenate([p[:50], np.array([[np.nan, 0, 0], [100, 100, 100]], np.float32)])
    full = M.radius_count(q, p, radius_sq=1.25, cap=0)
    assert full.max() > 6
    for cap in (1, 6):
        assert np.array_equal(M.radius_count(q, p, radius_sq=1.25, cap=cap), np.minimum(full, cap))
    zero = M.radius_count(q, p, radius_sq=0.0)
    assert zero[:50].min() >= 1 and zero[50:].tolist() == [0, 0]          # its own site (and the duplicates of it)
    assert M.radius_count(q, p, radius_sq=np.inf).tolist() == [len(p)] * 50 + [0, len(p)]
    assert M.radius_count(q, with_bad_rows(p), radius_sq=np.inf)[0] == len(p) - len(p) // 10
    for r2 in (np.nan, -1.0, -np.inf):
        assert (M.radius_count(q, p, radius_sq=r2) == 0).all()
    assert (M.radius_count(q, p, radius=np.nan) == 0).all()
    assert np.array_equal(M.radius_count(q, p, radius=-1.5), M.radius_count(q, p, radius=1.5))          # only the square matters
    with pytest.raises(ValueError):
        M.radius_count(q, p, radius=1.0, cap=-1)
    with pytest.raises(ValueError):
        M.radius_count(q, p)


# ---- depth_percentile ---------------------------------------------------------------------------------------------------------------------
def test_depth_percentile_is_numpy_percentile_of_the_nonzero_values():
    rng = np.random.default_rng(11)
    x = (rng.random(20011) * 180 + 3).astype(np.float32)
    x[rng.random(x.size) < 0.3] = 0
    nz = x[x != 0].astype(np.float64)
    for q in (0.0, 3.0, 50.0, 99.5, 99.9, 100.0):
        got, want = D.depth_percentile(x, q), float(np.percentile(nz, q))
        assert isinstance(got, float) and abs(got - want) <= 1e-12 * abs(want), (q, got, want)
    pair = D.depth_percentile(torch.from_numpy(x).reshape(-1, 1), (3.0, 99.9))
    assert pair == (D.depth_percentile(x, 3.0), D.depth_percentile(x, 99.9))
    assert D.depth_percentile(np.array([0, 0, 7.5, 0], np.float32), 40.0) == 7.5
    with pytest.raises(ValueError):
        D.depth_percentile(np.zeros(5, np.float32), 50.0)
    with pytest.raises(ValueError):
        D.depth_percentile(x, 101.0)


# ---- scene_normalization on the analytic scene ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    depths, K, poses, planted = analytic_scene()
    return depths, K, poses, planted, D.scene_normalization(depths, K, poses, **SCENE_ARGS)


def frame_points(depths, K, poses, i):
    """Every valid pixel of frame i back-projected in fp64, [H, W, 3] (NaN where the depth is 0)."""
    H, W = depths.shape[1:]
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    k, c2w, z = K[i].astype(np.float64), poses[i].astype(np.float64), depths[i].astype(np.float64)
    cam = np.stack([(xs - k[0, 2]) / k[0, 0] * z, (ys - k[1, 2]) / k[1, 1] * z, z], -1)
    world = cam @ c2w[:3, :3].T + c2w[:3, 3]
    return np.where((z > 0)[..., None], world, np.nan)


def test_scene_normalization_drops_the_planted_pixels(scene):
    depths, K, poses, planted, out = scene
    kept = out["kept_mask"].numpy()
    assert kept.shape == depths.shape and kept.dtype == bool
    assert planted.sum() == 9 and not (kept & planted).any()
    assert not (kept & (depths == 0)).any()
    c = out["counts"]
    assert c["valid"] == (depths > 0).sum((1, 2)).tolist() and c["sampled"] == c["valid"]
    assert c["kept"] == kept.sum((1, 2)).tolist() and c["merged"] == sum(c["kept"]) == len(out["points"])          # the merged pass drops nothing here
    dropped = np.array(c["valid"]) - np.array(c["kept"])
    assert (dropped >= 3).all() and (dropped <= 3 + 12).all()          # the planted three and at most a few sparse silhouette pixels
    assert out["close_depth"] == float(depths[depths > 0].min()) and out["inf_depth"] == PLANTED_DEPTHS[-1]


def test_scene_normalization_sphere_and_boxes(scene):
    depths, K, poses, planted, out = scene
    kept, radius, S = out["kept_mask"].numpy(), out["depth_norm_scale"], out["scale_mat"].numpy()
    assert S.dtype == np.float32 and np.array_equal(np.diag(S), np.float32([radius, radius, radius, 1])) and not S[3, :3].any()
    pts = out["points"].numpy().astype(np.float64)
    assert abs(np.linalg.norm(pts, axis=1).max() - 0.6) <= 1e-6
    world = np.concatenate([frame_points(depths, K, poses, i)[kept[i]] for i in range(3)])
    assert np.abs(pts * radius + S[:3, 3] - world).max() <= 1e-4          # the cloud is the kept pixels (fp32 back-projection of ~100)
    lo, hi = np.nanmin(world, 0), np.nanmax(world, 0)
    assert np.abs(S[:3, 3] - (lo + hi) / 2).max() <= 1e-4
    # the per-frame boxes, without pad: tight around exactly frame i's kept points
    flat = D.scene_normalization(depths, K, poses, pad=(0.0, 0.0, 0.0), **SCENE_ARGS)
    box = flat["bbox_minmax"].numpy()
    assert box.shape == (3, 3, 2) and box.dtype == np.float64
    ends = np.cumsum([0] + out["counts"]["kept"])
    for i in range(3):
        own = flat["points"].numpy().astype(np.float64)[ends[i]:ends[i + 1]]
        assert np.abs(box[i, :, 0] - own.min(0)).max() <= 1e-7 and np.abs(box[i, :, 1] - own.max(0)).max() <= 1e-7
    # the pad is the formula: -pad / radius below, +pad / radius above
    pad = np.array([-5.0, -5.0, 10.0])
    assert np.allclose(out["bbox_minmax"].numpy(), np.stack([box[..., 0] - pad / radius, box[..., 1] + pad / radius], -1), rtol=0, atol=1e-15)


def test_scene_normalization_down_sample_and_empty_frames(scene):
    depths, K, poses, planted, _ = scene
    u = torch.rand(depths.shape, generator=torch.Generator().manual_seed(3))
    args = dict(SCENE_ARGS, down_sample=0.5, nb_points=0, radius_factor=1e-3)          # no neighbour needed: every sampled pixel is kept
    out = D.scene_normalization(depths, K, poses, u=u, **args)
    assert np.array_equal(out["kept_mask"].numpy(), (depths > 0) & (u.numpy() < 0.5))
    assert out["counts"]["sampled"] == out["counts"]["kept"] and out["counts"]["valid"] == (depths > 0).sum((1, 2)).tolist()
    with pytest.raises(ValueError, match="frame 1"):
        empty = depths.copy()
        empty[1] = 0
        D.scene_normalization(empty, K, poses, **SCENE_ARGS)
    with pytest.raises(ValueError, match="frame 0"):          # nothing has six neighbours within a hair's breadth
        D.scene_normalization(depths, K, poses, **dict(SCENE_ARGS, radius_factor=1e-3))
    masks = np.ones_like(depths)
    masks[2] = 0
    with pytest.raises(ValueError, match="frame 2"):
        D.scene_normalization(depths, K, poses, masks=masks, **SCENE_ARGS)


# ---- normalize_cameras, FrameSet.from_raw ------------------------------------------------------------------------------------------------
def test_normalize_cameras_keeps_every_pixel():
    rng = np.random.default_rng(5)
    n, c, r = 4, np.array([3.0, -7.0, 90.0]), 52.5
    K = np.tile(np.array([[570.0, 0, 319.5, 0], [0, 560.0, 255.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]])[None], (n, 1, 1))
    poses = np.tile(np.eye(4)[None], (n, 1, 1))
    for i in range(n):
        poses[i, :3, :3] = np.linalg.qr(rng.standard_normal((3, 3)))[0]
        poses[i, :3, 3] = rng.standard_normal(3) * 10
    S = np.diag([r, r, r, 1.0])
    S[:3, 3] = c
    K2, poses2 = D.normalize_cameras(K, poses, S)
    assert np.array_equal(K2.numpy(), K) and np.array_equal(poses2.numpy()[:, :3, :3], poses[:, :3, :3])

    def project(k, c2w, X):
        cam = (X - c2w[:3, 3]) @ c2w[:3, :3]          # R^T (X - t)
        uvw = cam @ k[:3, :3].T
        return uvw[:, :2] / uvw[:, 2:]

    X = c + rng.standard_normal((500, 3)) * 20
    for i in range(n):
        assert np.abs(project(K[i], poses[i], X) - project(K2.numpy()[i], poses2.numpy()[i], (X - c) / r)).max() <= 1e-3
    k32, p32 = D.normalize_cameras(torch.from_numpy(K).float(), torch.from_numpy(poses).float(), torch.from_numpy(S).float())
    assert p32.dtype == torch.float32 and np.allclose(p32.numpy(), poses2.numpy(), rtol=1e-6, atol=1e-6)


def test_frameset_from_raw_equals_hand_normalised_inputs(scene):
    depths, K, poses, planted, out = scene
    n, H, W = depths.shape
    colors = np.random.default_rng(2).random((n, H, W, 3)).astype(np.float32)
    bounds = np.tile(np.array([[40.0, 160.0]], np.float32), (n, 1))
    fs = D.FrameSet.from_raw(colors, depths, K, poses, bounds, device="cpu", **SCENE_ARGS)
    r, c = out["depth_norm_scale"], out["scale_mat"].numpy()[:3, 3].astype(np.float64)
    assert fs.depth_scale == r and torch.equal(fs.scale_mat, out["scale_mat"]) and torch.equal(fs.bbox_minmax, out["bbox_minmax"])
    hand = poses.copy()
    hand[:, :3, 3] = ((poses[:, :3, 3].astype(np.float64) - c) / float(out["scale_mat"][0, 0])).astype(np.float32)          # scale_mat is fp32
    ref = D.FrameSet(colors, torch.from_numpy(depths)[..., None] / r, K, hand, torch.from_numpy(bounds) / r, device="cpu")
    assert torch.equal(fs.rays, ref.rays) and torch.equal(fs.depths, ref.depths) and torch.equal(fs.masks, ref.masks)
    origin = fs.rays[..., :3].reshape(n, -1, 3)[:, 0].double().numpy()
    assert np.abs(origin * r + c - poses[:, :3, 3]).max() <= 1e-4          # the camera centres, back in the raw frame
    # masked-out pixels take no part in the normalisation
    cm = np.ones((n, H, W, 1), np.float32)
    cm[planted] = 0
    masked = D.FrameSet.from_raw(colors, depths, K, poses, bounds, color_masks=cm, device="cpu", **SCENE_ARGS)
    want = D.scene_normalization(np.where(planted, np.float32(0), depths), K, poses, **SCENE_ARGS)
    assert masked.depth_scale == want["depth_norm_scale"] != r and torch.equal(masked.bbox_minmax, want["bbox_minmax"])
    assert torch.equal(masked.color_masks, torch.from_numpy(cm)) and torch.equal(masked.depths, torch.from_numpy(depths)[..., None] / masked.depth_scale)          # the depths themselves are not masked
