"""Back to the image: pixel tracks with a visibility flag, optical flow, scene flow and motion-stabilised frames from the model.

``trace_surface`` takes a pixel's ray to the surface, ``track_points`` follows that piece of tissue through time; this module brings the
tracked point back into an image -- a float-pixel projection with its flags (``project_points``, the pinhole camera of
``meshing.project_vertices``) -- and asks whether it is *seen* there: ``segment_visible``, a segment query on the field, "is the straight
segment from a to b free of the surface?".  A point that projects into the image is not thereby seen: another fold of tissue may lie in
front of it at the target time.  On top of the two: ``track_pixels`` (2D tracks with a visibility flag, flow and scene flow),
``frame_flow`` (the same on a camera's whole pixel grid), ``sample_bilinear`` / ``stabilize_frames`` (every target frame resampled so that
the tissue holds still in the reference view), ``flow_to_rgb`` and ``track_errors``.

Plain torch in the dtype and on the device of its inputs.  ``sdf_fn(x [M,3], t [M,1]) -> [M,1]`` and ``deform_fn(y [M,3], t [M]) -> D``
are any callables, as in ``tracing`` and ``tracking`` (``deform_fn=None``: no deformation, D = 0).  Every product and sum is taken one by
one (no fused multiply-adds) in the order the docstrings fix: they are the specification of the device kernels (csrc/visible.hip,
csrc/flow.hip), and the renderer's methods of the same names pass those kernels the same arguments through the same checks.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import meshing, tracing, tracking

FREE, OCCLUDED, UNKNOWN = 1, 2, 3
MAX_ROWS = 2 ** 31 - 1          # row counts (and three times them) the device path indexes with int32 / size_t


def check_visible_args(margin=5e-3, tau=0.0, relax=1.0, min_step=1e-3, max_iters=128):
    """The argument checks of ``segment_visible``, shared by the device path: returns (margin, tau, relax, min_step, max_iters) as
    Python floats and an int, or raises ValueError naming the argument.  tau, relax, min_step and max_iters are the tracer's."""
    tau, _, relax, min_step, max_iters = tracing.check_trace_args(tau, 0.0, relax, min_step, max_iters)
    margin = float(margin)
    if not (0.0 <= margin < math.inf):
        raise ValueError(f"margin must be finite and not negative (got {margin})")
    return margin, tau, relax, min_step, max_iters


def _sqrt(x):
    """The correctly rounded square root.  torch's fp32 root on a CPU is, on some machines, an approximate one; taken in fp64 and rounded
    to fp32 it is the correctly rounded fp32 root whatever the last bit of the fp64 one (a root of an fp32 number is never that close
    to the middle between two fp32 numbers), and that is what the device computes."""
    return torch.sqrt(x.double()).to(x.dtype) if x.dtype == torch.float32 else torch.sqrt(x)


def _rows3(a, name):
    a = torch.as_tensor(a)
    if a.dim() != 2 or a.shape[1] != 3 or not a.dtype.is_floating_point:
        raise ValueError(f"{name} must be a floating [M, 3] tensor (got {tuple(a.shape)}, {a.dtype})")
    return a


def segment_visible(sdf_fn, origins, points, t, margin=5e-3, tau=0.0, relax=1.0, min_step=1e-3, max_iters=128):
    """Is the straight segment from a = ``origins`` [M,3] to b = ``points`` [M,3] free of the surface sdf(., t) = tau, up to ``margin``
    before b?  dict(status [M] int32 (FREE, OCCLUDED, UNKNOWN), iters [M] int32, blocker [M], clearance [M], free_to [M]).  ``t``: scalar
    or [M].
    Per row ("Segment rule"):

      (Every root is the correctly rounded one.)
      A non-finite a, b or t: UNKNOWN, iters = 0.  d = b - a, L = sqrt(d.d); ``L > 0`` false: UNKNOWN, iters = 0.
      u = d / L.  (s_in, s_out): the unit-ball interval of the line a + s u by ``tracing.ray_geometry``'s formulas with d = u --
        dd = u.u, d1 = -(u.a) / dd, p = a + d1 u, d2 = sqrt(max(1 - p.p, 0)) / sqrt(dd), s_in = max(d1 - d2, 0), s_out = d1 + d2.
      s_end = L - margin if that is < s_out, else s_out.  ``s_end > s_in`` false: FREE, iters = 0 -- no part of the segment lies inside
        the ball and before the margin.
      Otherwise s = s_in, last = false, and for k = 1 .. max_iters:
        f = sdf(a + s u, t) - tau; iters = k; clearance = f if f < clearance.
        f not finite: UNKNOWN, stop.   f <= 0: OCCLUDED, blocker = s, stop.   last: FREE, stop.
        s = s + max(relax f, min_step);  if s >= s_end: s = s_end, last = true -- the end of the tested part is always evaluated
        itself, so a step that overshoots (|grad sdf| of a trained field exceeds 1) cannot jump a thin occluder at the end.
      After the loop: UNKNOWN.
      blocker is +inf unless OCCLUDED; clearance is +inf at iters = 0.
      free_to = the s of the row's last evaluation with f > 0, -inf if it had none.  ``blocker`` is the first EVALUATED point with
      f <= 0, not the crossing: a step that overshoots lands as far past the surface as it is long, at most on s_end.  (free_to,
      blocker] is the bracket of the first crossing the walk found, and on a FREE row free_to = s_end is how far the row is known free.

    No refinement to an eps, no d_z parametrisation, no comparison of two nearly equal depths: s is arc length along the segment.
    ``sdf_fn`` is only ever called on the rows still live, so a row's result depends on its own (a, b, t) and on nothing else."""
    margin, tau, relax, min_step, max_iters = check_visible_args(margin, tau, relax, min_step, max_iters)
    a, b = _rows3(origins, "origins"), _rows3(points, "points")
    if a.shape != b.shape or a.dtype != b.dtype:
        raise ValueError(f"origins and points must have one shape and dtype (got {tuple(a.shape)} {a.dtype}, {tuple(b.shape)} {b.dtype})")
    M, dt, dev = a.shape[0], a.dtype, a.device
    tt = tracking._times(t, M, a)
    c = lambda v: torch.tensor(v, dtype=dt, device=dev)
    margin_, tau_, relax_, min_step_ = c(margin), c(tau), c(relax), c(min_step)
    inf = float("inf")
    dot = tracing._dot

    d = b - a
    L = _sqrt(dot(d, d))
    finite = torch.isfinite(a).all(-1) & torch.isfinite(b).all(-1) & torch.isfinite(tt)
    ok = finite & (L > 0)
    u = d / L[:, None]
    dd = dot(u, u)
    d1 = -dot(u, a) / dd
    p = a + d1[:, None] * u
    d2 = _sqrt(torch.clamp(1.0 - dot(p, p), min=0.0)) / _sqrt(dd)
    s_in, s_out = torch.clamp(d1 - d2, min=0.0), d1 + d2
    Lm = L - margin_
    s_end = torch.where(Lm < s_out, Lm, s_out)
    go = ok & (s_end > s_in)

    status = torch.full((M,), FREE, dtype=torch.int32, device=dev)
    status[~ok] = UNKNOWN
    status[go] = 0          # live
    iters = torch.zeros(M, dtype=torch.int32, device=dev)
    blocker = torch.full((M,), inf, dtype=dt, device=dev)
    clearance = torch.full((M,), inf, dtype=dt, device=dev)
    free_to = torch.full((M,), -inf, dtype=dt, device=dev)
    s = s_in.clone()
    last = torch.zeros(M, dtype=torch.bool, device=dev)
    for k in range(1, max_iters + 1):
        idx = torch.nonzero(status == 0).reshape(-1)
        if idx.numel() == 0:
            break
        si = s[idx]
        x = a[idx] + si[:, None] * u[idx]
        f = sdf_fn(x, tt[idx][:, None]).reshape(-1).to(dt) - tau_
        iters[idx] = k
        clearance[idx] = torch.where(f < clearance[idx], f, clearance[idx])
        fin = torch.isfinite(f)
        hit = fin & (f <= 0)
        done = fin & ~hit & last[idx]
        st = torch.zeros_like(status[idx])
        st[~fin] = UNKNOWN
        st[hit] = OCCLUDED
        st[done] = FREE
        blocker[idx] = torch.where(hit, si, blocker[idx])
        free_to[idx] = torch.where(fin & ~hit, si, free_to[idx])
        s_new = si + torch.maximum(relax_ * f, min_step_)
        over = s_new >= s_end[idx]
        walk = st == 0
        s[idx] = torch.where(walk, torch.where(over, s_end[idx], s_new), si)
        last[idx] = last[idx] | (walk & over)
        status[idx] = st
    status[status == 0] = UNKNOWN
    return {"status": status, "iters": iters, "blocker": blocker, "clearance": clearance, "free_to": free_to}


# ---- the camera ------------------------------------------------------------------------------------------------------------------------
def _host64(m):
    return np.asarray(m.detach().cpu() if hasattr(m, "detach") else m, np.float64)


def ray_camera(intrinsics, pose):
    """The 21 fp64 numbers ``pixel_rays`` reads: K^-1 [9] (row-major, the upper-left 3 x 3 of the inverse of ``intrinsics`` [3,3] or
    [4,4], as ``data.get_rays`` takes it), R [9] (row-major rotation of the camera-to-world ``pose``) and its translation [3].  Goes
    through ``meshing.camera_params``, so that function's refusals apply."""
    meshing.camera_params(intrinsics, pose)
    K, P = _host64(intrinsics), _host64(pose)
    kinv = torch.inverse(torch.from_numpy(K.copy()))[:3, :3].numpy()
    return np.concatenate([kinv.reshape(-1), P[:3, :3].reshape(-1), P[:3, 3]])


def camera_table(intrinsics, poses):
    """[F,17] fp64: ``meshing.camera_params`` of every camera.  ``poses`` [4,4] or [F,4,4]; ``intrinsics`` [3,3] / [4,4] for all of
    them, or one per pose.  Returns (table, shared) with ``shared`` true for a single [4,4] pose."""
    P, K = _host64(poses), _host64(intrinsics)
    if P.ndim == 2:
        if K.ndim != 2:
            raise ValueError(f"one pose takes one intrinsics matrix (got {K.shape})")
        return meshing.camera_params(K, P)[None], True
    if P.ndim != 3 or K.ndim not in (2, 3) or (K.ndim == 3 and K.shape[0] != P.shape[0]):
        raise ValueError(f"poses must be [4,4] or [F,4,4] with one intrinsics matrix or F of them (got {P.shape}, {K.shape})")
    rows = [meshing.camera_params(K if K.ndim == 2 else K[f], P[f]) for f in range(P.shape[0])]
    return (np.stack(rows) if rows else np.zeros((0, 17))), False


def pixel_rays(pixels, intrinsics, pose, t):
    """Rays [P,9] through the continuous pixel positions ``pixels`` [P,2], (x, y) = (column, row), by ``data.get_rays``' formula:
    c_i = (Kinv_i0 x + Kinv_i1 y) + Kinv_i2, n = sqrt(c.c), c = c / n, d_i = (R_i0 c_0 + R_i1 c_1) + R_i2 c_2, o = the pose's
    translation.  Columns 6:8 are zero, column 8 is ``t`` (one time for all rays)."""
    px = torch.as_tensor(pixels)
    if px.dim() != 2 or px.shape[1] != 2 or not px.dtype.is_floating_point:
        raise ValueError(f"pixels must be a floating [P, 2] tensor (got {tuple(px.shape)}, {px.dtype})")
    cam = torch.from_numpy(ray_camera(intrinsics, pose)).to(device=px.device, dtype=px.dtype)
    ki, R, o = cam[:9].reshape(3, 3), cam[9:18].reshape(3, 3), cam[18:]
    x, y = px[:, 0], px[:, 1]
    c = [(ki[i, 0] * x + ki[i, 1] * y) + ki[i, 2] for i in range(3)]
    n = torch.sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2])
    c = [ci / n for ci in c]
    d = [(R[i, 0] * c[0] + R[i, 1] * c[1]) + R[i, 2] * c[2] for i in range(3)]
    rays = torch.zeros(px.shape[0], 9, dtype=px.dtype, device=px.device)
    rays[:, :3] = o
    rays[:, 3], rays[:, 4], rays[:, 5] = d
    rays[:, 8] = float(t)
    return rays


def project_points(points, intrinsics, poses):
    """World points [..., 3] through the pinhole camera of ``meshing.project_vertices`` -- x_cam = R^T (x - t), u = (K00 x + K01 y) / z
    + K02, v = K11 y / z + K12, evaluated in fp64 in that function's operation order -- as a float pixel, not fixed point:
    dict(pixel [..., 2] = (u, v) = (column, row), z [...] = the camera depth, front [...] bool) in the dtype of ``points``.  One camera
    serves all rows, or ``poses`` [F,4,4] (with one ``intrinsics`` or [F] of them) serve ``points`` [F,P,3].  ``front`` = the point, z,
    u and v are finite and z > 0; rows that are not ``front`` have pixel 0, rows that are not finite z = NaN."""
    pts = torch.as_tensor(points)
    if pts.dim() < 1 or pts.shape[-1] != 3 or not pts.dtype.is_floating_point:
        raise ValueError(f"points must be a floating [..., 3] tensor (got {tuple(pts.shape)}, {pts.dtype})")
    table, shared = camera_table(intrinsics, poses)
    cam = torch.from_numpy(table).to(pts.device)
    if not shared:
        if pts.dim() != 3 or pts.shape[0] != cam.shape[0]:
            raise ValueError(f"{cam.shape[0]} cameras take points [{cam.shape[0]}, P, 3] (got {tuple(pts.shape)})")
        cam = cam[:, None, :]
    x = pts.double()
    d = [x[..., i] - cam[..., 9 + i] for i in range(3)]
    c = [(cam[..., i] * d[0] + cam[..., 3 + i] * d[1]) + cam[..., 6 + i] * d[2] for i in range(3)]
    u = (cam[..., 12] * c[0] + cam[..., 13] * c[1]) / c[2] + cam[..., 14]
    v = cam[..., 15] * c[1] / c[2] + cam[..., 16]
    finite = torch.isfinite(x).all(-1) & torch.isfinite(c[2])
    front = finite & torch.isfinite(u) & torch.isfinite(v) & (c[2] > 0)
    pixel = torch.where(front[..., None], torch.stack([u, v], -1), torch.zeros((), dtype=torch.float64, device=pts.device))
    z = torch.where(finite, c[2], torch.full((), float("nan"), dtype=torch.float64, device=pts.device))
    return {"pixel": pixel.to(pts.dtype), "z": z.to(pts.dtype), "front": front}


def in_image(pixel, front, height, width):
    """``front`` and 0 <= x <= W - 1 and 0 <= y <= H - 1."""
    x, y = pixel[..., 0], pixel[..., 1]
    return front & (x >= 0) & (x <= width - 1) & (y >= 0) & (y <= height - 1)


def camera_centres(poses, F, like):
    """[F,3]: the translation of each camera-to-world pose ([4,4]: the same for every frame), in the dtype and on the device of ``like``."""
    P = torch.from_numpy(_host64(poses)).to(device=like.device, dtype=like.dtype)
    return P[:3, 3].expand(F, 3) if P.dim() == 2 else P[:, :3, 3]


def resolve(pixel, points, source_pixels, source_points, source_valid, converged, inside, visible):
    """The flags and differences of ``track_pixels``: valid = source_valid & converged & in_image & visible; pixels, flow = pixels -
    source pixels and scene_flow = points - source_points, each zero on rows that are not valid."""
    valid = source_valid[None] & converged & inside & visible
    zero = torch.zeros((), dtype=pixel.dtype, device=pixel.device)
    v = valid[..., None]
    return {"valid": valid, "pixels": torch.where(v, pixel, zero), "flow": torch.where(v, pixel - source_pixels[None], zero),
            "scene_flow": torch.where(v, points - source_points[None], zero)}


def _image_size(height, width):
    H, W = int(height), int(width)
    if H != height or W != width or H < 1 or W < 1:
        raise ValueError(f"height and width must be positive integers (got {height!r}, {width!r})")
    return H, W


def track_pixels(sdf_fn, deform_fn, pixels, intrinsics, pose, t_from, times, height, width, intrinsics_to=None, poses_to=None,
                 margin=5e-3, trace_args=None, track_args=None):
    """``pixels`` [P,2] of the camera (``intrinsics``, ``pose``) at time ``t_from``, followed into F target images at ``times`` [F].
    The source rays (``pixel_rays``) are traced with ``tracing.trace_surface(**trace_args)``; the hits are followed with
    ``tracking.track_points(**track_args)``; the tracked points are projected (``project_points``) into the target cameras
    ``intrinsics_to`` / ``poses_to`` ([4,4] or [F,4,4]; default: the source camera for every frame, the fixed endoscope); and each is
    tested with ``segment_visible`` from its target camera's centre at its target time, with ``margin`` and the tau of ``trace_args``.

    dict(pixels [F,P,2], points [F,P,3], source_points [P,3], source_valid [P] = the trace's HIT, converged, in_image, visible, valid
    [F,P], flow [F,P,2] = pixels - source pixels, scene_flow [F,P,3] = points - source_points, z [F,P], status, iters [F,P] int32 of
    the segment query).  in_image = front and 0 <= x <= W - 1 and 0 <= y <= H - 1; visible = status FREE; valid = source_valid &
    converged & in_image & visible.  Rows that are not valid are zero in pixels, flow and scene_flow (the convention of 7i-7l)."""
    H, W = _image_size(height, width)
    trace_args, track_args = dict(trace_args or {}), dict(track_args or {})
    px = torch.as_tensor(pixels)
    rays = pixel_rays(px, intrinsics, pose, t_from)
    P, dt, dev = px.shape[0], px.dtype, px.device
    times = torch.as_tensor(times, dtype=dt, device=dev).reshape(-1)
    F = times.numel()
    deform = deform_fn if deform_fn is not None else (lambda y, t: torch.zeros_like(y))
    tr = tracing.trace_surface(sdf_fn, rays, **trace_args)
    source_points, source_valid = tr["points"], tr["status"] == tracing.HIT
    tk = tracking.track_points(deform, source_points, t_from, times, **track_args)
    pts = tk["points"]
    K_to, P_to = (intrinsics if intrinsics_to is None else intrinsics_to), (pose if poses_to is None else poses_to)
    proj = project_points(pts, K_to, P_to)
    origins = camera_centres(P_to, F, pts)[:, None, :].expand(F, P, 3)
    vis = segment_visible(sdf_fn, origins.reshape(-1, 3), pts.reshape(-1, 3), times.repeat_interleave(P), margin,
                          tau=trace_args.get("tau", 0.0))
    inside = in_image(proj["pixel"], proj["front"], H, W)
    status = vis["status"].reshape(F, P)
    out = resolve(proj["pixel"], pts, px, source_points, source_valid, tk["converged"], inside, status == FREE)
    out.update(points=pts, source_points=source_points, source_valid=source_valid, converged=tk["converged"], in_image=inside,
               visible=status == FREE, z=proj["z"], status=status, iters=vis["iters"].reshape(F, P))
    return out


def pixel_grid(height, width, dtype=torch.float32, device=None):
    """[H W, 2]: (x, y) = (column, row) of every pixel, row by row."""
    ys, xs = torch.meshgrid(torch.arange(height, dtype=dtype, device=device), torch.arange(width, dtype=dtype, device=device), indexing="ij")
    return torch.stack([xs, ys], -1).reshape(-1, 2)


FRAME_KEYS = ("pixels", "points", "converged", "in_image", "visible", "valid", "flow", "scene_flow", "z", "status", "iters")
SOURCE_KEYS = ("source_points", "source_valid")


def frame_flow(sdf_fn, deform_fn, intrinsics, pose, t_from, times, height, width, intrinsics_to=None, poses_to=None, margin=5e-3,
               trace_args=None, track_args=None, dtype=torch.float32, device=None):
    """``track_pixels`` on the full pixel grid of the source camera: dense optical flow and scene flow.  Outputs are shaped [F,H,W,...]
    (``source_points`` [H,W,3], ``source_valid`` [H,W])."""
    H, W = _image_size(height, width)
    out = track_pixels(sdf_fn, deform_fn, pixel_grid(H, W, dtype, device), intrinsics, pose, t_from, times, H, W, intrinsics_to, poses_to,
                       margin, trace_args, track_args)
    return shape_frames(out, H, W)


def shape_frames(out, H, W):
    F = out["valid"].shape[0]
    shaped = {k: out[k].reshape(F, H, W, *out[k].shape[2:]) for k in FRAME_KEYS if k in out}
    shaped.update({k: out[k].reshape(H, W, *out[k].shape[1:]) for k in SOURCE_KEYS})
    return shaped


# ---- resampling ------------------------------------------------------------------------------------------------------------------------
def sample_bilinear(image, pixels, valid, background=0.0):
    """``image`` [H,W,C] at the float positions ``pixels`` [M,2] = (x, y): [M,C] in the image's dtype.  x0 = min(floor(x), W - 2)
    (not below 0), x1 = min(x0 + 1, W - 1), fx = x - x0, likewise for y; the two row blends first, top = I[y0,x0] + fx (I[y0,x1] -
    I[y0,x0]) and bottom on y1, then the column blend top + fy (bottom - top).  Rows that are not ``valid``, or outside [0, W - 1] x
    [0, H - 1] (a NaN is outside), get ``background`` (a number or [C]).  At an integer position the weights are 0 -- the texel itself,
    bit for bit -- except on the last column and row, where they are 1 and a + (b - a) is b exactly whenever b - a is exact, as for
    frames that hold 8-bit levels."""
    img = torch.as_tensor(image)
    if img.dim() != 3 or not img.dtype.is_floating_point:
        raise ValueError(f"image must be a floating [H, W, C] tensor (got {tuple(img.shape)}, {img.dtype})")
    H, W, C = img.shape
    px = torch.as_tensor(pixels).to(device=img.device)
    if px.dim() != 2 or px.shape[1] != 2:
        raise ValueError(f"pixels must be [M, 2] (got {tuple(px.shape)})")
    px = px.to(img.dtype)
    x, y = px[:, 0], px[:, 1]
    ok = torch.as_tensor(valid).to(img.device).bool().reshape(-1) & (x >= 0) & (x <= W - 1) & (y >= 0) & (y <= H - 1)
    xs, ys = torch.where(ok, x, torch.zeros_like(x)), torch.where(ok, y, torch.zeros_like(y))
    x0 = torch.clamp(torch.clamp(torch.floor(xs), max=W - 2), min=0)
    y0 = torch.clamp(torch.clamp(torch.floor(ys), max=H - 2), min=0)
    fx, fy = (xs - x0)[:, None], (ys - y0)[:, None]
    j0, i0 = x0.long(), y0.long()
    j1, i1 = torch.clamp(j0 + 1, max=W - 1), torch.clamp(i0 + 1, max=H - 1)
    top = img[i0, j0] + fx * (img[i0, j1] - img[i0, j0])
    bottom = img[i1, j0] + fx * (img[i1, j1] - img[i1, j0])
    val = top + fy * (bottom - top)
    bg = torch.as_tensor(background, dtype=img.dtype, device=img.device).expand(C)
    return torch.where(ok[:, None], val, bg[None])


def stabilize_frames(frames, flow, background=0.0):
    """The motion-stabilised video: target frame f of ``frames`` [F,H,W,C] sampled (``sample_bilinear``) at ``flow["pixels"][f]``, where
    the tissue seen at each pixel of the reference view is in frame f, so that the tissue holds still in the reference view.
    ``flow``: the dict ``frame_flow`` returns.  dict(frames [F,H,W,C], valid [F,H,W] = the flow's ``valid``); pixels that are not
    valid get ``background``."""
    fr = torch.as_tensor(frames)
    px, valid = torch.as_tensor(flow["pixels"]), torch.as_tensor(flow["valid"])
    if fr.dim() != 4 or px.dim() != 4 or px.shape[0] != fr.shape[0] or px.shape[-1] != 2 or valid.shape != px.shape[:3]:
        raise ValueError(f"frames must be [F, H, W, C] and the flow's pixels [F, h, w, 2] with valid [F, h, w] (got {tuple(fr.shape)}, "
                         f"{tuple(px.shape)}, {tuple(valid.shape)})")
    F, h, w = px.shape[:3]
    out = [sample_bilinear(fr[f], px[f].reshape(-1, 2), valid[f].reshape(-1), background).reshape(h, w, fr.shape[3]) for f in range(F)]
    return {"frames": torch.stack(out) if out else fr.new_zeros(0, h, w, fr.shape[3]), "valid": valid.to(fr.device).bool()}


def flow_to_rgb(flow, max_flow):
    """Flow [..., 2] = (u, v) as colour, uint8 [..., 3]: hue h = atan2(v, u) / (2 pi) mod 1, saturation s = min(|flow| / max_flow, 1),
    value 1, through the six-sector HSV to RGB map:  h6 = 6 h, i = floor(h6) mod 6, f = h6 - floor(h6), p = 1 - s, q = 1 - s f,
    t = 1 - s (1 - f);  (r, g, b) = (1, t, p), (q, 1, p), (p, 1, t), (p, q, 1), (t, p, 1), (1, p, q) for i = 0 .. 5;  each channel
    floor(255 c + 0.5).  Zero flow is white; a row with a non-finite component is black."""
    max_flow = float(max_flow)
    if not (0.0 < max_flow < math.inf):
        raise ValueError(f"max_flow must be finite and positive (got {max_flow})")
    fl = torch.as_tensor(flow)
    if fl.dim() < 1 or fl.shape[-1] != 2 or not fl.dtype.is_floating_point:
        raise ValueError(f"flow must be a floating [..., 2] tensor (got {tuple(fl.shape)}, {fl.dtype})")
    u, v = fl[..., 0], fl[..., 1]
    fin = torch.isfinite(u) & torch.isfinite(v)
    u, v = torch.where(fin, u, torch.zeros_like(u)), torch.where(fin, v, torch.zeros_like(v))
    h = torch.remainder(torch.atan2(v, u) / (2.0 * math.pi), 1.0)
    s = torch.clamp(torch.sqrt(u * u + v * v) / max_flow, max=1.0)
    h6 = 6.0 * h
    fl6 = torch.floor(h6)
    i = torch.remainder(fl6, 6.0).long()
    f = h6 - fl6
    one = torch.ones_like(s)
    p, q, t = 1.0 - s, 1.0 - s * f, 1.0 - s * (1.0 - f)
    table = torch.stack([torch.stack(c, -1) for c in ((one, t, p), (q, one, p), (p, one, t), (p, q, one), (t, p, one), (one, p, q))], -2)
    rgb = torch.gather(table, -2, i[..., None, None].expand(*i.shape, 1, 3))[..., 0, :]
    rgb = torch.where(fin[..., None], rgb, torch.zeros_like(rgb))
    return torch.floor(255.0 * rgb + 0.5).to(torch.uint8)


def track_errors(pred_pixels, pred_visible, gt_pixels, gt_visible, thresholds=(1, 2, 4, 8, 16)):
    """How point-tracking benchmarks score 2D tracks [..., 2] with visibility flags [...]: dict(epe = the mean end-point error over
    rows with gt_visible, delta [n] = the share of those rows within each threshold (pixels), delta_avg = their mean,
    occlusion_accuracy = the share of all rows whose visibility flag is right, count = the rows with gt_visible).  Sums are in fp64;
    every value is a 0-dim (delta: [n]) fp64 tensor on the device of the inputs, NaN where its denominator is 0."""
    pp, gp = torch.as_tensor(pred_pixels), torch.as_tensor(gt_pixels)
    pv, gv = torch.as_tensor(pred_visible).bool().to(pp.device), torch.as_tensor(gt_visible).bool().to(pp.device)
    if pp.shape != gp.shape or pp.shape[-1:] != (2,) or pv.shape != pp.shape[:-1] or gv.shape != pv.shape:
        raise ValueError(f"pixels must be [..., 2] and flags [...] of one shape (got {tuple(pp.shape)}, {tuple(gp.shape)}, {tuple(pv.shape)}, "
                         f"{tuple(gv.shape)})")
    e = pp.double() - gp.double().to(pp.device)
    dist = torch.sqrt(e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1])
    g = gv.double()
    count = g.sum()
    epe = torch.where(gv, dist, torch.zeros_like(dist)).sum() / count
    th = torch.as_tensor(thresholds, dtype=torch.float64, device=pp.device).reshape(-1)
    delta = ((dist[..., None] <= th) & gv[..., None]).double().reshape(-1, th.numel()).sum(0) / count
    total = torch.tensor(float(pv.numel()), dtype=torch.float64, device=pp.device)
    return {"epe": epe, "delta": delta, "delta_avg": delta.mean(), "occlusion_accuracy": (pv == gv).double().sum() / total,
            "count": count}
