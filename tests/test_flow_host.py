"""CPU: ``endosurf_amd.flow``, the host specification and twin of the pixel tracks -- on an analytic scene in fp64
against closed forms, against a scalar restatement of the segment rule, and on the fp64 / fp32 oracles of the test weights.  Every test
prints the figures it asserts on."""
import math

import numpy as np
import pytest
import torch

from flow_util import (HEIGHT, K, KINDS, MARGIN, PAST, POSE, WIDTH, Recorded, cycle_pixels, rotated_pose, segments, twin_cycle, visible_case,
                       visible_scalar)
from trace_util import CASES, ITERS_CAP, STATUS_CAP, case, same, sdf_fn, sqrt64

from endosurf_amd import data
from endosurf_amd import flow as FL
from endosurf_amd import tracing as T

INF = float("inf")
RADIUS = 0.5
V = torch.tensor([0.30, -0.20, 0.10], dtype=torch.float64)          # the observed sphere's centre is t V
CAM = torch.tensor(POSE[:3, 3])


def moving_sphere():
    """sdf = |x_c| - 0.5 with D(x, t) = -t V: the observed sphere moves by +t V."""
    def sdf(x, t):
        c = x - t * V[None]
        return torch.sqrt(c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1] + c[:, 2] * c[:, 2])[:, None] - RADIUS
    return sdf, lambda y, t: -t[:, None] * V[None].to(y.dtype)


def project_closed_form(x, pose):
    """Pinhole projection written with numpy matrices: (pixel [..., 2], z)."""
    R, t = pose[:3, :3], pose[:3, 3]
    c = (np.asarray(x) - t) @ R          # R^T (x - t), row-wise
    return np.stack([K[0, 0] * c[..., 0] / c[..., 2] + K[0, 2], K[1, 1] * c[..., 1] / c[..., 2] + K[1, 2]], -1), c[..., 2]


def first_hit(o, d, centre, radius):
    """Ray o + s d (|d| = 1) against a sphere: (meets, s_first, discriminant)."""
    oc = o - centre
    b = (oc * d).sum(-1)
    disc = b * b - ((oc * oc).sum(-1) - radius * radius)
    return disc > 0, -b - torch.sqrt(disc.clamp(min=0.0)), disc


def scene_pixels(n=97, seed=5):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(np.stack([rng.uniform(0, WIDTH - 1, n), rng.uniform(0, HEIGHT - 1, n)], -1))


@pytest.mark.parametrize("second_camera", [False, True], ids=["fixed", "rotated"])
def test_track_pixels_against_the_closed_form(second_camera):
    sdf, dfm = moving_sphere()
    px = scene_pixels()
    t_a, times = 0.25, [0.0, 0.4, 0.8]
    poses = np.stack([POSE, rotated_pose(), POSE]) if second_camera else None
    out = FL.track_pixels(sdf, dfm, px, K, POSE, t_a, times, HEIGHT, WIDTH, poses_to=poses, trace_args=dict(eps=1e-12), track_args=dict(tol=1e-12))
    rays = FL.pixel_rays(px, K, POSE, t_a)
    meets, s0, disc = first_hit(rays[:, :3], rays[:, 3:6], t_a * V, RADIUS)
    clear = disc.abs() > 1e-3          # not grazing: the closed form and the tracer agree on what meets the sphere
    assert int(clear.sum()) >= 90 and int((meets & clear).sum()) >= 40 and int((~meets & clear).sum()) >= 5
    assert torch.equal(out["source_valid"][clear], meets[clear])
    hit = meets & clear
    x_a = rays[:, :3] + s0[:, None] * rays[:, 3:6]
    assert float((out["source_points"] - x_a)[hit].abs().max()) <= 1e-10
    worst_px = worst_pt = 0.0
    n_valid = n_hidden = 0
    for f, t_b in enumerate(times):
        pose = POSE if poses is None else poses[f]
        x_b = x_a + (t_b - t_a) * V[None]
        want_px, want_z = project_closed_form(x_b.numpy(), pose)
        want_px = torch.from_numpy(want_px)
        inside = torch.from_numpy(want_z > 0) & (want_px[:, 0] >= 0) & (want_px[:, 0] <= WIDTH - 1) & (want_px[:, 1] >= 0) & (want_px[:, 1] <= HEIGHT - 1)
        cam = torch.from_numpy(pose[:3, 3])
        u = x_b - cam[None]
        L = torch.sqrt((u * u).sum(-1))
        u = u / L[:, None]
        cos = ((x_b - t_b * V[None]) * u).sum(-1) / RADIUS          # < 0: the point faces the camera
        facing, away = cos < -0.1, cos > 0.1                              # (between the two a margin of 5e-3 decides; nothing is asserted)
        assert int((hit & (facing | away)).sum()) >= 0.8 * int(hit.sum())
        assert torch.equal(out["in_image"][f][hit], inside[hit]) and bool(out["converged"][f][hit].all())
        assert bool(out["visible"][f][hit & facing].all()) and not bool(out["visible"][f][hit & away].any())
        want_valid = hit & inside & facing
        sure = ~hit | ~inside | facing | away
        assert torch.equal(out["valid"][f][sure & clear], want_valid[sure & clear])
        v = out["valid"][f] & want_valid
        n_valid, n_hidden = n_valid + int(v.sum()), n_hidden + int((hit & away).sum())
        worst_px = max(worst_px, float((out["pixels"][f] - want_px)[v].abs().max()))
        worst_pt = max(worst_pt, float((out["points"][f] - x_b)[hit].abs().max()))
        assert float((out["flow"][f] - (want_px - px))[v].abs().max()) <= 1e-8
        assert float((out["scene_flow"][f] - (t_b - t_a) * V[None])[v].abs().max()) <= 1e-10
        nv = ~out["valid"][f]
        assert bool((out["pixels"][f][nv] == 0).all()) and bool((out["flow"][f][nv] == 0).all()) and bool((out["scene_flow"][f][nv] == 0).all())
    print(f"\nmoving sphere ({'second camera' if second_camera else 'fixed camera'}): {n_valid} valid rows, {n_hidden} facing away; "
          f"|pixel - closed form| max {worst_px:.3e} px, |point - closed form| max {worst_pt:.3e}")
    assert n_valid >= 100 and worst_px <= 1e-8 and worst_pt <= 1e-10


def test_an_occluder_that_moves_in_front():
    """A second sphere, joined by min, is far outside the unit ball at the source time and in front of the first at the target time:
    ``visible`` is the analytic line of sight on every row whose analytic clearance exceeds the margin."""
    t_a, t_b, r2 = 0.2, 0.7, 0.15
    c2 = lambda t: torch.tensor([0.10, 0.05, -0.75], dtype=torch.float64) + (t_b - t) * torch.tensor([6.0, 0.0, 0.0], dtype=torch.float64)
    base, dfm = moving_sphere()

    def sdf(x, t):
        centre = torch.stack([c2(float(tt)) for tt in t.reshape(-1)])
        e = x - centre
        return torch.minimum(base(x, t), torch.sqrt((e * e).sum(-1))[:, None] - r2)
    px = scene_pixels(197, 6)
    out = FL.track_pixels(sdf, dfm, px, K, POSE, t_a, [t_b], HEIGHT, WIDTH, trace_args=dict(eps=1e-12), track_args=dict(tol=1e-12))
    rays = FL.pixel_rays(px, K, POSE, t_a)
    meets, s0, disc = first_hit(rays[:, :3], rays[:, 3:6], t_a * V, RADIUS)
    hit = meets & (disc.abs() > 1e-3)
    assert torch.equal(out["source_valid"][hit], meets[hit]) and int(hit.sum()) >= 80
    x_b = rays[:, :3] + s0[:, None] * rays[:, 3:6] + (t_b - t_a) * V[None]
    u = x_b - CAM[None]
    L = torch.sqrt((u * u).sum(-1))
    u = u / L[:, None]
    cos = ((x_b - t_b * V[None]) * u).sum(-1) / RADIUS
    s_c = ((c2(t_b)[None] - CAM[None]) * u).sum(-1).clamp(min=0.0)          # the occluder's centre projected on the segment
    s_c = torch.minimum(s_c, L)
    e = CAM[None] + s_c[:, None] * u - c2(t_b)[None]
    dist = torch.sqrt((e * e).sum(-1))
    # from the occluder's silhouette, and from the sphere's own: the line through a point of the sphere passes its centre at R sqrt(1 - cos^2)
    clearance = torch.minimum((dist - r2).abs(), RADIUS * (1.0 - torch.sqrt((1.0 - cos * cos).clamp(min=0.0))))
    sure = hit & (clearance > MARGIN)
    blocked = (dist < r2) | (cos > 0)
    n_blocked = int((blocked & sure).sum())
    print(f"\noccluder: {int(hit.sum())} traced rows, {int(sure.sum())} with analytic clearance > margin, {n_blocked} of them blocked "
          f"({int(((dist < r2) & sure).sum())} by the occluder)")
    assert int(sure.sum()) >= 0.8 * int(hit.sum()) and int(((dist < r2) & sure).sum()) >= 5 and int((~blocked & sure).sum()) >= 20
    assert torch.equal(out["visible"][0][sure], ~blocked[sure])
    assert bool((out["status"][0][sure & (dist < r2)] == FL.OCCLUDED).all())


# ---- the segment rule --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_deform", [True, False], ids=["deform", "static"])
@pytest.mark.parametrize("mode,seed", CASES, ids=lambda v: str(v))
def test_the_twin_is_the_rule_and_the_caps(mode, seed, use_deform):
    """``segment_visible`` on the batch against ``visible_scalar`` row by row on the three kinds of segments: status, iters, blocker
    (and clearance), exactly, on the same field values; the fp32 oracle twin against the fp64 twin under the tracer's two caps; and what
    the segments are built to show."""
    v = visible_case(mode, seed, use_deform)
    c, a, t, hit = v["case"], v["a"], v["t"], v["hit"]
    for kind in KINDS:
        b = v["ends"][kind]
        rec = Recorded(sdf_fn(c["net64"]))
        twin = FL.segment_visible(rec.torch_fn, a, b, t)
        for k in ("status", "iters", "blocker", "clearance", "free_to"):
            assert same(twin[k], v[kind, 64][k]), (kind, k)          # (recording changes nothing)
        for i in range(a.shape[0]):
            want = visible_scalar(rec.float_fn, a[i].tolist(), b[i].tolist(), float(t[i]))
            got = (int(twin["status"][i]), int(twin["iters"][i]), float(twin["blocker"][i]), float(twin["clearance"][i]), float(twin["free_to"][i]))
            assert got == want, (kind, i, got, want)
        t64, t32 = v[kind, 64], v[kind, 32]
        d_status, d_iters = int((t32["status"] != t64["status"]).sum()), int((t32["iters"] != t64["iters"]).sum())
        counts = torch.bincount(t64["status"][hit], minlength=4).tolist()[1:]
        print(f"\n[{v['name']} {kind}] FREE / OCCLUDED / UNKNOWN on the {int(hit.sum())} traced rows {counts}; evaluations per row mean "
              f"{float(t64['iters'].double().mean()):.2f} max {int(t64['iters'].max())}; one-row evaluations the scalar rule needed {rec.misses}; "
              f"fp32 twin: status differs on {d_status} rows (cap {STATUS_CAP}), iters on {d_iters} (cap {ITERS_CAP})")
        assert rec.misses == 0 and d_status <= STATUS_CAP and d_iters <= ITERS_CAP
        st = t64["status"][hit]
        if kind == "hit":
            assert int((st == FL.FREE).sum()) > 0.5 * int(hit.sum())
        elif kind == "mid":
            assert bool((st == FL.FREE).all())
        else:
            assert bool((st == FL.OCCLUDED).all())
            # OCCLUDED at the fp64 hit +- margin, on every traced row: the crossing the walk found lies in (free_to, blocker], and the
            # fp64 hit -- at arc length L -- lies in that bracket, to the margin at either end.  (blocker alone is the first EVALUATED
            # point with a value <= 0: a step that overshoots lands past the crossing, at most on the clamped end L + PAST - MARGIN.)
            L = torch.sqrt(((v["ends"]["hit"] - a) ** 2).sum(-1))
            lo, hi = (t64["free_to"] - L)[hit], (t64["blocker"] - L)[hit]
            print(f"    free_to - L: max {float(lo.max()):.3e}; blocker - L: min {float(hi.min()):.3e} max {float(hi.max()):.3e}; blocker within the "
                  f"margin of the hit on {int((hi.abs() <= MARGIN).sum())} of {int(hit.sum())} rows")
            assert bool((lo <= MARGIN).all()) and bool((hi >= -MARGIN).all())
            lo32, hi32 = (t32["free_to"].double() - L)[hit], (t32["blocker"].double() - L)[hit]
            assert bool((lo32 <= MARGIN).all()) and bool((hi32 >= -MARGIN).all())
            assert float(hi.max()) <= PAST * (1 + 1e-6) - MARGIN          # (|d| of an fp32 unit vector)
        assert bool((t64["blocker"][t64["status"] != FL.OCCLUDED] == INF).all()) and bool((t64["clearance"][t64["iters"] == 0] == INF).all())
    assert PAST > MARGIN


def unit_sphere_field(scale=1.0):
    torch_fn = lambda x, t: (scale * (torch.sqrt(x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2]) - RADIUS))[:, None]
    return torch_fn, lambda x0, x1, x2, t: scale * (sqrt64(x0 * x0 + x1 * x1 + x2 * x2) - RADIUS)


SPECIAL_A = [[0.0, 0.0, -1.5]] * 8
SPECIAL_B = [[0.0, 0.0, 0.6],                       # through the sphere: OCCLUDED at s = 1
             [float("nan"), 0.0, 0.0],            # a NaN row
             [0.0, 0.0, -1.5],                      # a == b
             [0.0, 3.0, -1.5],                      # wholly outside the unit ball
             [0.0, 0.0, -1.497],                    # margin > L
             [0.0, 0.0, -0.6],                      # ends 0.1 in front of the sphere: FREE
             [0.0, 0.0, -0.5],                      # ends on the sphere: FREE by the margin
             [0.0, 0.0, -0.498]]                    # ends 2e-3 inside: FREE by the margin; OCCLUDED at margin = 0


def test_special_segments_one_assertion_each():
    torch_fn, float_fn = unit_sphere_field()
    a, b = torch.tensor(SPECIAL_A, dtype=torch.float64), torch.tensor(SPECIAL_B, dtype=torch.float64)
    out = FL.segment_visible(torch_fn, a, b, 0.3)
    for i in range(8):
        want = visible_scalar(float_fn, SPECIAL_A[i], SPECIAL_B[i], 0.3)
        assert (int(out["status"][i]), int(out["iters"][i]), float(out["blocker"][i]), float(out["clearance"][i]), float(out["free_to"][i])) == want, i
    print(f"\nspecial segments: status {out['status'].tolist()} iters {out['iters'].tolist()} blocker {out['blocker'].tolist()}")
    assert int(out["status"][0]) == FL.OCCLUDED and abs(float(out["blocker"][0]) - 1.0) <= 1e-3 and float(out["clearance"][0]) <= 0
    assert (int(out["status"][1]), int(out["iters"][1])) == (FL.UNKNOWN, 0)
    assert (int(out["status"][2]), int(out["iters"][2])) == (FL.UNKNOWN, 0)
    assert (int(out["status"][3]), int(out["iters"][3])) == (FL.FREE, 0)
    assert (int(out["status"][4]), int(out["iters"][4])) == (FL.FREE, 0) and float(out["clearance"][4]) == INF
    assert int(out["status"][5]) == FL.FREE and abs(float(out["clearance"][5]) - (0.1 + MARGIN)) <= 1e-12
    assert int(out["status"][6]) == FL.FREE and int(out["status"][7]) == FL.FREE
    assert int(FL.segment_visible(torch_fn, a[7:], b[7:], 0.3, margin=0.0)["status"][0]) == FL.OCCLUDED
    one = FL.segment_visible(torch_fn, a, b, 0.3, max_iters=1)          # the cap: a row that needs more is UNKNOWN after one evaluation
    assert one["status"].tolist() == [FL.UNKNOWN, FL.UNKNOWN, FL.UNKNOWN, FL.FREE, FL.FREE, FL.UNKNOWN, FL.UNKNOWN, FL.UNKNOWN]
    assert one["iters"].tolist() == [1, 0, 0, 0, 0, 1, 1, 1]
    nan_t = FL.segment_visible(torch_fn, a[:1], b[:1], float("nan"))
    assert (int(nan_t["status"][0]), int(nan_t["iters"][0])) == (FL.UNKNOWN, 0)
    bad = FL.segment_visible(lambda x, t: torch.full_like(t, float("nan")), a[:1], b[:1], 0.3)
    assert (int(bad["status"][0]), int(bad["iters"][0]), float(bad["blocker"][0]), float(bad["clearance"][0]), float(bad["free_to"][0])) == (FL.UNKNOWN, 1, INF, INF, -INF)
    assert float(out["free_to"][0]) < float(out["blocker"][0]) and float(out["free_to"][5]) == 0.9 - MARGIN and float(out["free_to"][3]) == -INF
    empty = FL.segment_visible(torch_fn, a[:0], b[:0], 0.3)
    assert all(empty[k].shape == (0,) for k in ("status", "iters", "blocker", "clearance", "free_to")) and empty["status"].dtype == torch.int32
    out32 = FL.segment_visible(torch_fn, a.float(), b.float(), torch.full((8,), 0.3))
    assert out32["blocker"].dtype == torch.float32 and out32["status"].tolist() == out["status"].tolist()


def test_a_step_that_overshoots_cannot_jump_the_end():
    """A field of gradient 3 with relax 1 steps three times the distance: a thin shell just before the end of the tested part is
    jumped by the walk, and found by the evaluation of the end itself."""
    shell = lambda x, t: (3.0 * ((torch.sqrt((x * x).sum(-1)) - RADIUS).abs() - 0.004))[:, None]          # |.| <= 0 within 4e-3 of the sphere
    a, b = torch.tensor([[0.0, 0.0, -1.5]], dtype=torch.float64), torch.tensor([[0.0, 0.0, -0.497]], dtype=torch.float64)
    out = FL.segment_visible(shell, a, b, 0.0)
    assert int(out["status"][0]) == FL.OCCLUDED and abs(float(out["blocker"][0]) - (1.003 - MARGIN)) <= 1e-12


def test_argument_refusals():
    torch_fn, _ = unit_sphere_field()
    a, b = torch.tensor(SPECIAL_A, dtype=torch.float64), torch.tensor(SPECIAL_B, dtype=torch.float64)
    bad = [("margin", -1e-9), ("margin", float("inf")), ("margin", float("nan")), ("tau", float("nan")), ("relax", 0.0), ("relax", 1.5),
           ("min_step", 0.0), ("min_step", float("inf")), ("max_iters", 0), ("max_iters", 1025), ("max_iters", 2.5)]
    for name, value in bad:
        with pytest.raises(ValueError, match=name):
            FL.segment_visible(torch_fn, a, b, 0.3, **{name: value})
        with pytest.raises(ValueError, match=name):
            FL.check_visible_args(**{name: value})
    assert FL.check_visible_args(0.0, 0.05, 1.0, 1e-3, 1024) == (0.0, 0.05, 1.0, 1e-3, 1024)
    with pytest.raises(ValueError, match="points"):
        FL.segment_visible(torch_fn, a, b[:, :2], 0.3)
    with pytest.raises(ValueError, match="one shape"):
        FL.segment_visible(torch_fn, a, b[:3], 0.3)
    assert (FL.FREE, FL.OCCLUDED, FL.UNKNOWN) == (1, 2, 3)


# ---- camera ------------------------------------------------------------------------------------------------------------------------------
def test_pixel_rays_is_get_rays_and_project_points_inverts_it():
    K4 = np.eye(4)
    K4[:3, :3] = K
    h, w = 7, 9
    grid = FL.pixel_grid(h, w, torch.float64)
    for pose in (POSE, rotated_pose(0.3, 0.1)):
        rays = FL.pixel_rays(grid, K4, pose, 0.4)
        ref = data.get_rays(torch.from_numpy(K4)[None], torch.from_numpy(pose)[None], w, h)[0].reshape(-1, 6)
        assert rays.shape == (h * w, 9) and bool((rays[:, 6:8] == 0).all()) and bool((rays[:, 8] == 0.4).all())
        assert torch.allclose(rays[:, :6], ref, rtol=1e-6, atol=0.0)
        assert torch.allclose(FL.pixel_rays(grid.float(), K, pose, 0.4)[:, :6], ref.float(), rtol=1e-6, atol=1e-7)
        px = torch.from_numpy(np.random.default_rng(2).uniform(-20, 660, size=(50, 2)))
        r = FL.pixel_rays(px, K, pose, 0.0)
        depth1 = r[:, :3] + r[:, 3:6] / (r[:, 3:6] @ torch.from_numpy(pose[:3, 2]))[:, None]          # camera depth 1 along each ray
        back = FL.project_points(depth1, K, pose)
        err = float((back["pixel"] - px).abs().max())
        print(f"\nproject(pixel_rays) - pixel: max {err:.3e} px; z - 1 max {float((back['z'] - 1).abs().max()):.3e}")
        assert err <= 1e-9 and bool(back["front"].all()) and float((back["z"] - 1).abs().max()) <= 1e-12
        want, _ = project_closed_form(depth1.numpy(), pose)
        assert float((back["pixel"] - torch.from_numpy(want)).abs().max()) <= 1e-9


def test_project_points_flags_shapes_and_refusals():
    pts = torch.tensor([[0.0, 0.0, 0.0], [0.0, 0.0, -2.0], [float("nan"), 0.0, 0.0], [0.0, 0.0, -1.5], [0.1, -0.1, 0.2]], dtype=torch.float64)
    out = FL.project_points(pts, K, POSE)
    assert out["front"].tolist() == [True, False, False, False, True] and bool((out["pixel"][~out["front"]] == 0).all())
    assert out["pixel"][0].tolist() == [319.5, 255.5] and float(out["z"][0]) == 1.5 and float(out["z"][1]) == -0.5 and math.isnan(float(out["z"][2]))
    assert FL.in_image(out["pixel"], out["front"], HEIGHT, WIDTH).tolist() == [True, False, False, False, True]
    assert not bool(FL.in_image(out["pixel"], out["front"], 200, 300)[0])
    poses = np.stack([POSE, rotated_pose()])
    many = FL.project_points(torch.stack([pts, pts]), K, poses)
    assert many["pixel"].shape == (2, 5, 2) and same(many["pixel"][0], out["pixel"]) and not same(many["pixel"][1], out["pixel"])
    assert same(many["pixel"][1], FL.project_points(pts, K, poses[1])["pixel"])
    assert same(FL.project_points(torch.stack([pts, pts]), np.stack([K, K]), poses)["pixel"], many["pixel"])
    assert FL.project_points(pts.float().reshape(5, 1, 3), K, POSE)["pixel"].shape == (5, 1, 2)
    with pytest.raises(ValueError, match="cameras take points"):
        FL.project_points(pts, K, poses)
    bad_K, bad_P = K.copy(), POSE.copy()
    bad_K[0, 0] = -1.0
    bad_P[:3, :3] *= 1.1
    for args, match in (((bad_K, POSE), "focal"), ((K, bad_P), "rigid"), ((K * np.nan, POSE), "finite")):
        with pytest.raises(ValueError, match=match):
            FL.project_points(pts, *args)
        with pytest.raises(ValueError, match=match):
            FL.pixel_rays(pts[:, :2], *args, 0.0)


# ---- cycle consistency -------------------------------------------------------------------------------------------------------------------
def test_cycle_consistency_on_the_trained_weights():
    """97 pixels tracked 0.3 -> 0.6 -> 0.3 in one camera: the worst return error over rows valid both ways, measured for the fp64 twin
    and the fp32-oracle twin (DESIGN.md 7o records both).  tol and eps are at most 1e-5 scene units at 800 px per unit, with room for
    grazing rows: the fp64 figure is below 1e-2 px."""
    (e64, n64), (e32, n32) = twin_cycle(64), twin_cycle(32)
    print(f"\ncycle 0.3 -> 0.6 -> 0.3: fp64 twin worst {e64:.3e} px over {n64} rows; fp32-oracle twin worst {e32:.3e} px over {n32} rows")
    assert cycle_pixels().shape == (97, 2) and n64 >= 49
    assert e64 < 1e-2


# ---- resampling, colour, metrics ---------------------------------------------------------------------------------------------------------
def identity_flow(F, H, W, dtype=torch.float32):
    return {"pixels": FL.pixel_grid(H, W, dtype).reshape(1, H, W, 2).repeat(F, 1, 1, 1), "valid": torch.ones(F, H, W, dtype=torch.bool)}


def test_static_identity_and_linear_frames():
    """Identical cameras and no deformation: every pixel maps to itself, and ``stabilize_frames`` returns the input frames bit for bit
    where valid (frames of 8-bit levels: on the last column and row the blend is a + 1 (b - a), exact for them).  Frames linear in
    (x, y) are reproduced at the predicted pixels within 8 x 2^-24 x max |texel|: a convex blend of at most that many fp32 roundings."""
    F, H, W = 2, 12, 16
    rng = np.random.default_rng(8)
    frames = torch.from_numpy(rng.integers(0, 256, size=(F, H, W, 3)).astype(np.float32))
    fl = identity_flow(F, H, W)
    fl["valid"][1, 3, 4] = False
    out = FL.stabilize_frames(frames, fl, background=0.5)
    assert out["frames"].shape == (F, H, W, 3) and same(out["valid"], fl["valid"])
    assert same(out["frames"][fl["valid"]], frames[fl["valid"]]) and bool((out["frames"][1, 3, 4] == 0.5).all())
    # the same through the model: a static field seen twice by one camera (a coarse 12 x 16 camera on the analytic sphere)
    Kc = np.array([[20.0, 0.0, 7.5], [0.0, 20.0, 5.5], [0.0, 0.0, 1.0]])
    static = lambda x, t: (torch.sqrt((x * x).sum(-1)) - RADIUS)[:, None]
    ff = FL.frame_flow(static, None, Kc, POSE, 0.1, [0.1, 0.9], H, W, trace_args=dict(eps=1e-12), dtype=torch.float64)
    assert ff["pixels"].shape == (2, H, W, 2) and ff["source_valid"].shape == (H, W) and int(ff["valid"].sum()) >= 2 * 40
    grid = FL.pixel_grid(H, W, torch.float64).reshape(H, W, 2)
    assert float((ff["pixels"] - grid[None])[ff["valid"]].abs().max()) <= 1e-9 and float(ff["flow"].abs().max()) <= 1e-9
    snapped = {"pixels": torch.round(ff["pixels"]), "valid": ff["valid"]}
    st = FL.stabilize_frames(frames, snapped, background=-1.0)
    assert same(st["frames"][ff["valid"]], frames[ff["valid"]]) and bool((st["frames"][~ff["valid"]] == -1.0).all())
    # linear frames
    coef = torch.tensor([[0.5, -0.25, 3.0], [0.125, 0.75, -2.0]])          # [2,3]: per channel a x + b y
    g = FL.pixel_grid(H, W).reshape(H, W, 2)
    linear = (g @ coef)[None] + 1.0
    px = torch.from_numpy(rng.uniform(0, 1, size=(300, 2)).astype(np.float32)) * torch.tensor([W - 1.0, H - 1.0])
    px[:4] = torch.tensor([[0.0, 0.0], [W - 1.0, H - 1.0], [W - 1.0, 2.5], [3.25, H - 1.0]])
    got = FL.sample_bilinear(linear[0], px, torch.ones(300, dtype=torch.bool))
    want = px.double() @ coef.double() + 1.0
    bound = 8 * 2.0 ** -24 * float(linear.abs().max())
    err = float((got.double() - want).abs().max())
    print(f"\nlinear frame: |sample - prediction| max {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    outside = torch.tensor([[-0.01, 1.0], [W - 0.99, 1.0], [1.0, H - 0.99], [float("nan"), 1.0], [2.0, 2.0]])
    o = FL.sample_bilinear(linear[0], outside, torch.tensor([True, True, True, True, False]), background=[7.0, 8.0, 9.0])
    assert o.tolist() == [[7.0, 8.0, 9.0]] * 5


def test_flow_to_rgb_at_the_sector_boundaries():
    m = 4.0
    ang = torch.arange(6, dtype=torch.float64) * (math.pi / 3)
    fl = torch.stack([m * torch.cos(ang), m * torch.sin(ang)], -1)
    want = [[255, 0, 0], [255, 255, 0], [0, 255, 0], [0, 255, 255], [0, 0, 255], [255, 0, 255]]
    got = FL.flow_to_rgb(fl, m)
    assert got.dtype == torch.uint8 and got.tolist() == want
    assert FL.flow_to_rgb(2 * fl, m).tolist() == want          # saturation is capped at 1
    assert FL.flow_to_rgb(torch.zeros(1, 2), m).tolist() == [[255, 255, 255]]
    assert FL.flow_to_rgb(torch.tensor([[2.0, 0.0], [0.0, -1.0], [float("nan"), 0.0]]), m).tolist() == [[255, 128, 128], [223, 191, 255], [0, 0, 0]]
    assert FL.flow_to_rgb(torch.zeros(3, 5, 2), m).shape == (3, 5, 3)
    with pytest.raises(ValueError, match="max_flow"):
        FL.flow_to_rgb(fl, 0.0)


def test_track_errors_on_a_hand_made_table():
    gt = torch.tensor([[10.0, 10.0], [20.0, 20.0], [30.0, 30.0], [40.0, 40.0], [50.0, 50.0]])
    pred = gt + torch.tensor([[0.0, 0.0], [3.0, 4.0], [0.0, 1.5], [100.0, 0.0], [0.0, 0.5]])
    gt_vis = torch.tensor([True, True, True, False, True])
    pred_vis = torch.tensor([True, False, True, False, False])
    e = FL.track_errors(pred, pred_vis, gt, gt_vis)
    assert all(v.dtype == torch.float64 for v in e.values())
    assert float(e["count"]) == 4 and float(e["epe"]) == (0.0 + 5.0 + 1.5 + 0.5) / 4
    assert e["delta"].tolist() == [0.5, 0.75, 0.75, 1.0, 1.0] and float(e["delta_avg"]) == 0.8
    assert float(e["occlusion_accuracy"]) == 3 / 5
    assert FL.track_errors(pred, pred_vis, gt, gt_vis, thresholds=(5,))["delta"].tolist() == [1.0]
    none = FL.track_errors(pred, pred_vis, gt, torch.zeros(5, dtype=torch.bool))
    assert math.isnan(float(none["epe"])) and float(none["count"]) == 0
