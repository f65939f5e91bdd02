"""GPU, renderer level: pixel tracks, optical flow and stabilised frames (renderer_flow.py over csrc/visible.hip and csrc/flow.hip,
DESIGN.md 7o) -- ``track_pixels`` against the composition of the public calls it is made of, the elementwise kernels against their fp64
twins, the dense flow against the sparse one, and the cycle consistency of the tracks against the fp32-oracle twin's."""
import math

import numpy as np
import pytest
import torch

from flow_util import CYCLE_T, HEIGHT, K, POSE, WIDTH, cycle_error, cycle_pixels, rotated_pose, twin_cycle
from gpu_util import renderer_for
from trace_util import same

from endosurf_amd import flow as FL

pytestmark = pytest.mark.gpu

EPS = 1e-5
T_FROM, TIMES = 0.3, [0.2, 0.5, 0.8]
KC = np.array([[20.0, 0.0, 7.5], [0.0, 20.0, 5.5], [0.0, 0.0, 1.0]])          # a coarse 12 x 16 camera on the same scene
TRACK_KEYS = ("pixels", "points", "source_points", "source_valid", "converged", "in_image", "visible", "valid", "flow", "scene_flow", "z",
              "status", "iters")


@pytest.fixture(scope="module", params=[True, False], ids=["deform", "static"])
def rr(request):
    return renderer_for(11, "trained", request.param)


def compose(r, px, poses_to, margin=5e-3):
    """``track_pixels`` spelled out in the renderer's public calls, the resolve rule restated in torch."""
    P, F = px.shape[0], len(TIMES)
    rays = r.pixel_rays(px, K, POSE, T_FROM)
    tr = r.trace_surface(rays)
    tk = r.track_points(tr["points"], T_FROM, TIMES)
    pts = tk["points"]
    target = POSE if poses_to is None else poses_to
    proj = r.project_points(pts, K, target)
    centres = torch.from_numpy(np.asarray(target)[..., :3, 3].astype(np.float32)).cuda()
    origins = (centres.expand(F, 3) if centres.dim() == 1 else centres)[:, None, :].expand(F, P, 3)
    times = torch.tensor(TIMES, device="cuda")
    vis = r.segment_visible(origins.reshape(-1, 3), pts.reshape(-1, 3), times.repeat_interleave(P), margin)
    x, y = proj["pixel"][..., 0], proj["pixel"][..., 1]
    inside = proj["front"] & (x >= 0) & (x <= WIDTH - 1) & (y >= 0) & (y <= HEIGHT - 1)
    visible = vis["visible"].reshape(F, P)
    valid = tr["valid"][None] & tk["converged"] & inside & visible
    zero = torch.zeros((), device="cuda")
    v = valid[..., None]
    return {"pixels": torch.where(v, proj["pixel"], zero), "points": pts, "source_points": tr["points"], "source_valid": tr["valid"],
            "converged": tk["converged"], "in_image": inside, "visible": visible, "valid": valid,
            "flow": torch.where(v, proj["pixel"] - px.cuda().float()[None], zero), "scene_flow": torch.where(v, pts - tr["points"][None], zero),
            "z": proj["z"], "status": vis["status"].reshape(F, P), "iters": vis["iters"].reshape(F, P)}


@pytest.mark.parametrize("second_camera", [False, True], ids=["fixed", "second-camera"])
def test_track_pixels_is_the_composition_of_its_public_calls(rr, second_camera):
    px = cycle_pixels().float()
    poses = np.stack([POSE, rotated_pose(0.1, 0.2), POSE]) if second_camera else None
    out = rr.track_pixels(px, K, POSE, T_FROM, TIMES, HEIGHT, WIDTH, poses_to=poses)
    want = compose(rr, px.cuda(), poses)
    assert sorted(out) == sorted(TRACK_KEYS) and all(v.is_cuda and not v.requires_grad for v in out.values())
    for k in TRACK_KEYS:
        assert out[k].shape == want[k].shape and out[k].dtype == want[k].dtype and same(out[k].cpu(), want[k].cpu()), k
    n = out["valid"].numel()
    counts = {k: int(out[k].sum()) for k in ("valid", "visible", "in_image", "converged")}
    print(f"\ntrack_pixels ({'deform' if rr.use_deform else 'static'}, {'second camera' if second_camera else 'fixed camera'}): of {n} rows "
          f"{counts}, source_valid {int(out['source_valid'].sum())} of 97; |flow| max {float(out['flow'].abs().max()):.2f} px")
    assert out["pixels"].shape == (3, 97, 2) and out["scene_flow"].shape == (3, 97, 3) and out["valid"].dtype == torch.bool
    assert counts["valid"] >= n / 2
    if rr.use_deform or second_camera:
        assert counts["visible"] < n or counts["in_image"] < n
    else:          # a static scene seen twice by one camera: every row projects onto its own pixel and is seen there
        assert counts["visible"] == n and counts["in_image"] == n and counts["converged"] == n
        assert float((out["pixels"] - px.cuda()[None])[out["valid"]].abs().max()) <= 1e-2
    nv = ~out["valid"]
    assert bool((out["pixels"][nv] == 0).all()) and bool((out["flow"][nv] == 0).all()) and bool((out["scene_flow"][nv] == 0).all())
    if not rr.use_deform:          # the identity track
        assert same(out["points"].cpu(), out["source_points"][None].expand(3, 97, 3).contiguous().cpu())
        assert bool((out["scene_flow"] == 0).all())
    again = rr.track_pixels(px, K, POSE, T_FROM, TIMES, HEIGHT, WIDTH, poses_to=poses)
    for k in TRACK_KEYS:
        assert same(again[k].cpu(), out[k].cpu()), k
    with pytest.raises(ValueError, match="margin"):
        rr.track_pixels(px, K, POSE, T_FROM, TIMES, HEIGHT, WIDTH, margin=-1.0)
    with pytest.raises(ValueError, match="target camera"):
        rr.track_pixels(px, K, POSE, T_FROM, TIMES, HEIGHT, WIDTH, poses_to=np.stack([POSE, POSE]))


def test_host_inputs_and_split_precision_change_nothing(rr):
    px = cycle_pixels().float()[:40]
    out = rr.track_pixels(px.cuda(), K, POSE, T_FROM, TIMES, HEIGHT, WIDTH)
    rr.engine.split_precision = True
    try:
        split = rr.track_pixels(px, K, POSE, T_FROM, TIMES, HEIGHT, WIDTH)
    finally:
        rr.engine.split_precision = False
    others = (split, rr.track_pixels(px.numpy(), torch.from_numpy(K), torch.from_numpy(POSE).cuda(), T_FROM, np.array(TIMES), HEIGHT, WIDTH),
              rr.track_pixels(px.double(), K, POSE, T_FROM, torch.tensor(TIMES, dtype=torch.float64), HEIGHT, WIDTH))
    for other in others:
        for k in TRACK_KEYS:
            assert other[k].is_cuda and same(other[k].cpu(), out[k].cpu()), k
    pts, t = out["points"].reshape(-1, 3), torch.tensor(TIMES, device="cuda").repeat_interleave(40)
    o = torch.from_numpy(POSE[:3, 3].astype(np.float32)).cuda().expand(120, 3)
    vis = rr.segment_visible(o, pts, t)
    assert sorted(vis) == ["blocker", "clearance", "free_to", "iters", "status", "visible"] and same(vis["status"].cpu(), out["status"].reshape(-1).cpu())
    for other in (rr.segment_visible(o.cpu().numpy(), pts.cpu(), t.cpu().double()), rr.segment_visible(o.double(), pts.double(), t)):
        for k in vis:
            assert same(other[k].cpu(), vis[k].cpu()), k
    with pytest.raises(ValueError, match="margin"):
        rr.segment_visible(o, pts, t, margin=float("nan"))
    empty = rr.segment_visible(o[:0], pts[:0], 0.3)
    assert empty["status"].shape == (0,) and empty["visible"].shape == (0,)


def ulps_off(got, want64):
    """How many entries of fp32 ``got`` differ from the fp64 twin's value rounded to fp32, and whether any differs by more than 1 ulp."""
    want = want64.float()
    differ = got != want
    both_nan = torch.isnan(got) & torch.isnan(want)
    differ &= ~both_nan
    gap = torch.from_numpy(np.spacing(np.abs(want.numpy()).astype(np.float32)))
    return int(differ.sum()), bool(((got - want).abs()[differ] <= gap[differ]).all())


def test_pixel_rays_and_project_points_against_the_fp64_twin(rr):
    rng = np.random.default_rng(12)
    px = torch.from_numpy(rng.uniform(-30, 670, size=(1000, 2)).astype(np.float32))
    for pose in (POSE, rotated_pose(0.3, 0.1)):
        got = rr.pixel_rays(px, K, pose, 0.37).cpu()
        want = FL.pixel_rays(px.double(), K, pose, 0.37)
        n, ok = ulps_off(got, want)
        print(f"\npixel_rays: {n} of {got.numel()} entries differ from the fp64 twin rounded to fp32, each by at most 1 ulp: {ok}")
        assert got.shape == (1000, 9) and ok and bool((got[:, 6:8] == 0).all()) and bool((got[:, 8] == np.float32(0.37)).all())
    pts = torch.from_numpy(rng.uniform(-1, 1, size=(3, 700, 3)).astype(np.float32))
    pts[0, 5] = torch.tensor([0.0, 0.0, -2.0])          # behind the first camera
    pts[1, 6, 2] = float("nan")
    pts[2, 7] = torch.from_numpy(POSE[:3, 3].astype(np.float32))          # the camera centre: z = 0
    poses = np.stack([POSE, rotated_pose(0.1, 0.2), rotated_pose(-0.2, -0.1)])
    for points, cams in ((pts, poses), (pts, POSE), (pts[0], POSE), (pts.reshape(3, 70, 10, 3), POSE)):
        got, want = rr.project_points(points, K, cams), FL.project_points(points.double(), K, cams)
        assert got["pixel"].shape == want["pixel"].shape and got["z"].shape == want["z"].shape and got["front"].dtype == torch.bool
        assert torch.equal(got["front"].cpu(), want["front"])
        for k in ("pixel", "z"):
            n, ok = ulps_off(got[k].cpu(), want[k])
            print(f"project_points {tuple(points.shape)} {k}: {n} of {want[k].numel()} entries differ, each by at most 1 ulp: {ok}")
            assert ok
    first = rr.project_points(pts, K, poses)
    assert not bool(first["front"][0, 5]) and not bool(first["front"][1, 6]) and not bool(first["front"][2, 7]) and math.isnan(float(first["z"][1, 6]))
    assert bool((first["pixel"][~first["front"]] == 0).all()) and int(first["front"].sum()) >= 2000
    with pytest.raises(ValueError, match="cameras take points"):
        rr.project_points(pts[0], K, poses)
    bad = K.copy()
    bad[1, 1] = 0.0
    with pytest.raises(ValueError, match="focal"):
        rr.project_points(pts, bad, POSE)


def test_sample_bilinear_flow_to_rgb_and_track_errors_against_the_twins(rr):
    rng = np.random.default_rng(13)
    H, W = 12, 16
    image = torch.from_numpy(rng.uniform(-2, 2, size=(H, W, 3)).astype(np.float32))
    px = torch.from_numpy(rng.uniform(-1, 1, size=(500, 2)).astype(np.float32)) * torch.tensor([W / 2 + 1.0, H / 2 + 1.0]) + torch.tensor([W / 2, H / 2])
    px[:6] = torch.tensor([[W - 1.0, H - 1.0], [W - 1.0, 3.5], [2.25, H - 1.0], [0.0, 0.0], [float("nan"), 2.0], [W - 0.5, 2.0]])
    valid = torch.from_numpy(rng.uniform(size=500) < 0.9)
    valid[:6] = True
    got = rr.sample_bilinear(image, px, valid, background=[0.25, 0.5, 0.75]).cpu()
    want = FL.sample_bilinear(image.double(), px.double(), valid, background=[0.25, 0.5, 0.75])
    bound = 8 * 2.0 ** -24 * float(image.abs().max())
    err = float((got.double() - want).abs().max())
    inside = valid & (px[:, 0] >= 0) & (px[:, 0] <= W - 1) & (px[:, 1] >= 0) & (px[:, 1] <= H - 1)
    print(f"\nsample_bilinear: |device - fp64 twin| max {err:.3e} (bound {bound:.3e}); {int(inside.sum())} rows inside, {int((~valid).sum())} not valid")
    assert err <= bound and 100 <= int(inside.sum()) < 480 and int((~valid).sum()) >= 20
    assert bool((got[~inside] == torch.tensor([0.25, 0.5, 0.75])).all()) and same(got[0], image[H - 1, W - 1]) and same(got[3], image[0, 0])
    assert same(rr.sample_bilinear(image.cuda(), px.cuda(), None, 0.0).cpu()[inside], got[inside])
    # colour
    fl = torch.from_numpy(rng.normal(size=(40, 50, 2)).astype(np.float32) * 3)
    ang = torch.arange(6, dtype=torch.float32) * (math.pi / 3)
    fl[0, :6] = torch.stack([4 * torch.cos(ang), 4 * torch.sin(ang)], -1)
    fl[0, 6], fl[0, 7, 0] = 0.0, float("nan")
    rgb, twin = rr.flow_to_rgb(fl, 4.0).cpu(), FL.flow_to_rgb(fl.double(), 4.0)
    off = (rgb.int() - twin.int()).abs()
    print(f"flow_to_rgb: {int((off > 0).sum())} of {off.numel()} channels differ from the twin, by at most {int(off.max())} level")
    assert rgb.dtype == torch.uint8 and rgb.shape == (40, 50, 3) and int(off.max()) <= 1
    assert rgb[0, 6].tolist() == [255, 255, 255] and rgb[0, 7].tolist() == [0, 0, 0] and rgb[0, 2].tolist() == [0, 255, 0]
    with pytest.raises(ValueError, match="max_flow"):
        rr.flow_to_rgb(fl, float("inf"))
    # metrics
    gt = torch.from_numpy(rng.uniform(0, 600, size=(3, 97, 2)).astype(np.float32))
    pred = gt + torch.from_numpy(rng.normal(size=(3, 97, 2)).astype(np.float32) * 4)
    gv, pv = torch.from_numpy(rng.uniform(size=(3, 97)) < 0.8), torch.from_numpy(rng.uniform(size=(3, 97)) < 0.7)
    e, ref = rr.track_errors(pred, pv, gt.cuda(), gv), FL.track_errors(pred, pv, gt, gv)
    for k in ref:
        assert e[k].is_cuda and e[k].dtype == torch.float64 and torch.allclose(e[k].cpu(), ref[k], rtol=1e-12, atol=0.0), k


def test_frame_flow_is_track_pixels_on_the_grid_and_stabilize_frames(rr):
    H, W = 12, 16
    grid = FL.pixel_grid(H, W)
    sparse = rr.track_pixels(grid, KC, POSE, T_FROM, TIMES, H, W)
    for chunk in (50, 65536):
        dense = rr.frame_flow(KC, POSE, T_FROM, TIMES, H, W, ray_chunk=chunk)
        assert sorted(dense) == sorted(TRACK_KEYS) and dense["pixels"].shape == (3, H, W, 2) and dense["source_valid"].shape == (H, W)
        for k in TRACK_KEYS:
            assert same(dense[k].reshape(sparse[k].shape).cpu(), sparse[k].cpu()), (chunk, k)
    print(f"\nframe_flow 12 x 16 -> 3 frames: valid {int(dense['valid'].sum())} of {dense['valid'].numel()}")
    assert int(dense["valid"].sum()) >= 100
    # the identity: identical cameras, no motion -- frames of 8-bit levels come back bit for bit where valid
    rng = np.random.default_rng(8)
    frames = torch.from_numpy(rng.integers(0, 256, size=(3, H, W, 3)).astype(np.float32))
    ident = {"pixels": grid.reshape(1, H, W, 2).repeat(3, 1, 1, 1), "valid": dense["valid"]}
    st = rr.stabilize_frames(frames, ident, background=-1.0)
    v = dense["valid"].cpu()
    assert st["frames"].shape == (3, H, W, 3) and st["frames"].is_cuda and same(st["valid"].cpu(), v)
    assert same(st["frames"].cpu()[v], frames[v]) and bool((st["frames"].cpu()[~v] == -1.0).all())
    if not rr.use_deform:          # the model's own static flow, snapped to the pixel it names
        snapped = {"pixels": torch.round(dense["pixels"]), "valid": dense["valid"]}
        assert float((dense["pixels"] - snapped["pixels"])[dense["valid"]].abs().max()) <= 1e-2
        assert same(rr.stabilize_frames(frames.cuda(), snapped)["frames"].cpu()[v], frames[v])
    # and against the twin on the model's flow
    got, want = rr.stabilize_frames(frames, dense, 0.5), FL.stabilize_frames(frames.double(), {k: dense[k].cpu().double() if k == "pixels" else dense[k].cpu() for k in ("pixels", "valid")}, 0.5)
    assert float((got["frames"].cpu().double() - want["frames"]).abs().max()) <= 8 * 2.0 ** -24 * 255.0


def test_cycle_consistency_on_the_device():
    """97 pixels tracked 0.3 -> 0.6 -> 0.3 in one camera: the worst return error over rows valid both ways is at most 4 x the fp32-oracle
    twin's measured figure plus 2 eps 800 px, the tracer's own form of budget."""
    r = renderer_for(11, "trained", True)
    track = lambda p, t_from, times: r.track_pixels(p, K, POSE, t_from, times, HEIGHT, WIDTH, trace_args=dict(eps=EPS))
    err, both = cycle_error(track, cycle_pixels().float(), *CYCLE_T)
    worst, (yard, n32) = float(err[both].max()), twin_cycle(32)
    bound = 4 * yard + 2 * EPS * 800
    print(f"\ncycle 0.3 -> 0.6 -> 0.3 on the device: worst return error {worst:.3e} px over {int(both.sum())} rows (bound {bound:.3e}: fp32-oracle "
          f"twin {yard:.3e} px over {n32} rows)")
    assert int(both.sum()) >= 49 and worst <= bound


def test_elementwise_entries_refuse_bad_arguments_before_launch():
    """es_pixel_rays, es_flow_project, es_flow_resolve, es_sample_bilinear and es_flow_panel: a count of 0 is status 0 without a launch;
    each bad argument is status 1 with its name in es_last_error() before anything is launched (the addresses are host numpy's and
    never dereferenced)."""
    import ctypes as C
    from endosurf_amd import _lib
    lib = _lib.load()
    buf = np.zeros(64, np.float64)
    b = buf.ctypes.data
    cam = (C.c_double * 21)(*([1.0] * 21))
    nan_cam = (C.c_double * 21)(*([1.0] * 20 + [float("nan")]))
    big = 1 << 31

    def rays(P=4, camera=cam, pixels=b, out=b):
        return lib.es_pixel_rays(pixels, P, camera, 0.5, out, None)

    def project(F=2, P=4, cameras=b, height=8, width=8, points=b, pixel=b, in_image=b):
        return lib.es_flow_project(points, F, P, cameras, 1, height, width, pixel, None, None, in_image, None, None)

    def resolve(F=2, P=4, pixel=b, visible=b):
        return lib.es_flow_resolve(pixel, b, b, b, b, b, b, b, F, P, visible, b, b, b, b, None)

    def sample(n_images=1, height=8, width=8, channels=3, M=4, rows=4, images=b, background=b):
        return lib.es_sample_bilinear(images, n_images, height, width, channels, b, None, M, rows, background, b, None)

    def panel(n=4, max_flow=1.0, flow=b, rgb=b):
        return lib.es_flow_panel(flow, n, max_flow, rgb, None)

    assert rays(P=0, pixels=None, out=None) == 0 and project(F=0, points=None, cameras=None) == 0 and project(P=0, points=None) == 0
    assert resolve(F=0, pixel=None, visible=None) == 0 and sample(M=0, images=None, background=None) == 0 and panel(n=0, flow=None, rgb=None) == 0
    bad = [(rays, "P", dict(P=-1)), (rays, "P", dict(P=big // 9 + 1)), (rays, "camera", dict(camera=None)), (rays, "finite", dict(camera=nan_cam)),
           (rays, "null buffer", dict(pixels=None)), (rays, "null buffer", dict(out=None)),
           (project, "F and P", dict(F=-1)), (project, "F and P", dict(P=-1)), (project, "2^31", dict(F=1024, P=big // 1024)),
           (project, "height and width", dict(height=0)), (project, "height and width", dict(width=32769)),
           (project, "null buffer", dict(points=None)), (project, "null buffer", dict(cameras=None)), (project, "8-byte", dict(cameras=b + 4)),
           (project, "every output", dict(pixel=None, in_image=None)),
           (resolve, "F and P", dict(F=-1)), (resolve, "2^31", dict(F=3, P=big // 3)), (resolve, "an input", dict(pixel=None)),
           (resolve, "an output", dict(visible=None)),
           (sample, "M", dict(M=-1)), (sample, "n_images", dict(n_images=0)), (sample, "rows_per_image", dict(rows=0)),
           (sample, "height and width", dict(height=0)), (sample, "height and width", dict(width=32769)), (sample, "channels", dict(channels=0)),
           (sample, "channels", dict(channels=65)), (sample, "2^31", dict(M=big // 3 + 1, rows=big)),
           (sample, "2^31", dict(n_images=16, height=32768, width=32768, channels=1, rows=4)), (sample, "rows_per_image", dict(M=9, rows=4, n_images=2)),
           (sample, "null buffer", dict(images=None)), (sample, "null buffer", dict(background=None)),
           (panel, "n", dict(n=-1)), (panel, "3 n", dict(n=big // 3 + 1)), (panel, "max_flow", dict(max_flow=0.0)),
           (panel, "max_flow", dict(max_flow=float("inf"))), (panel, "max_flow", dict(max_flow=float("nan"))),
           (panel, "null buffer", dict(flow=None)), (panel, "null buffer", dict(rgb=None))]
    for fn, name, kw in bad:
        assert fn(**kw) == 1 and name.encode() in lib.es_last_error(), (fn.__name__, name, kw, lib.es_last_error())
