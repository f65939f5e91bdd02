"""Pixel tracks, optical flow and stabilised frames of ``renderer.EndoSurfRenderer`` (a mixin): ``flow``'s functions with the model's
own networks under them -- the segment visibility query in one launch (csrc/visible.hip), projection, flags and resampling as
elementwise launches (csrc/flow.hip).  Outputs are device tensors under the twin's keys and shapes; host inputs are moved to the
renderer's device; nothing is read back."""
from __future__ import annotations

import torch

from . import flow, tracing
from ._device import _on_device, f32


class RendererFlowMixin:
    def _flow_f32(self, a, last):
        """``a`` (tensor, numpy array or nested list, anywhere) as fp32 [..., last], contiguous, on this device."""
        r = torch.as_tensor(a)
        if r.dim() < 1 or r.shape[-1] != last:
            raise ValueError(f"expected [..., {last}] (got {tuple(r.shape)})")
        return f32(r.to(device=self.device, dtype=torch.float32))

    @_on_device
    def segment_visible(self, origins, points, t, margin=5e-3, tau=0.0, relax=1.0, min_step=1e-3, max_iters=128):
        """Is the straight segment from each of ``origins`` [M,3] to its ``points`` [M,3] free of the surface at time ``t`` (scalar or
        [M]), up to ``margin`` before the point?  ``flow.segment_visible``'s dict (status, iters [M] int32, blocker, clearance, free_to [M]) as
        device tensors plus ``visible`` [M] bool (``status == flow.FREE``); no grad, no read-back, one launch, fp32 whatever
        ``engine.split_precision`` says."""
        a, b = self._track_rows(origins), self._track_rows(points)
        tt = self._track_times(t, a.shape[0])
        weff, packed = self._weights()
        with torch.no_grad():
            out = self.engine.segment_visible(a, b, tt, weff.detach(), packed, self.use_deform, margin, tau, relax, min_step, max_iters)
            out["visible"] = out["status"] == flow.FREE
        return out

    @_on_device
    def pixel_rays(self, pixels, intrinsics, pose, t):
        """``flow.pixel_rays``: rays [P,9] through the float pixels [P,2] = (column, row) of the camera at time ``t``; one launch."""
        return self.engine.pixel_rays(self._flow_f32(pixels, 2).reshape(-1, 2), flow.ray_camera(intrinsics, pose), float(t))

    @_on_device
    def project_points(self, points, intrinsics, poses):
        """``flow.project_points``: dict(pixel [..., 2], z [...], front [...] bool) of world points [..., 3]; one camera for all rows or
        ``poses`` [F,4,4] for points [F,P,3]; one launch."""
        pts = self._flow_f32(points, 3)
        table, shared = flow.camera_table(intrinsics, poses)
        if not shared and (pts.dim() != 3 or pts.shape[0] != table.shape[0]):
            raise ValueError(f"{table.shape[0]} cameras take points [{table.shape[0]}, P, 3] (got {tuple(pts.shape)})")
        rows = pts.reshape(1, -1, 3) if shared else pts
        out = self.engine.flow_project(rows, self.engine.flow_cameras(table), not shared)
        return {"pixel": out["pixel"].reshape(*pts.shape[:-1], 2), "z": out["z"].reshape(pts.shape[:-1]), "front": out["front"].reshape(pts.shape[:-1])}

    @_on_device
    def track_pixels(self, pixels, intrinsics, pose, t_from, times, height, width, intrinsics_to=None, poses_to=None, margin=5e-3,
                     trace_args=None, track_args=None):
        """``flow.track_pixels`` with the model's networks: ``pixels`` [P,2] of the camera at ``t_from`` followed into the target images
        at ``times`` [F] -- the twin's dict as device tensors, no read-back.  Cold (the default ``track_args``), a fixed number of
        launches whatever F is, seven with a deformation network: rays, trace, to-canonical, inverse, project, visibility, resolve."""
        H, W = flow._image_size(height, width)
        trace_args, track_args = dict(trace_args or {}), dict(track_args or {})
        px = self._flow_f32(pixels, 2).reshape(-1, 2)
        times = f32(torch.as_tensor(times).to(device=self.device, dtype=torch.float32)).reshape(-1)
        F, P = times.numel(), px.shape[0]
        K_to, P_to = (intrinsics if intrinsics_to is None else intrinsics_to), (pose if poses_to is None else poses_to)
        table, shared = flow.camera_table(K_to, P_to)
        if not shared and table.shape[0] != F:
            raise ValueError(f"{F} times take one target camera or {F} of them (got {table.shape[0]})")
        vis_args = flow.check_visible_args(margin, trace_args.get("tau", 0.0))
        weff, packed = self._weights()
        with torch.no_grad():
            rays = self.engine.pixel_rays(px, flow.ray_camera(intrinsics, pose), float(t_from))
            tr = self.trace_surface(rays, **trace_args)
            tk = self.track_points(tr["points"], float(t_from), times, **track_args)
            pts = f32(tk["points"])
            proj = self.engine.flow_project(pts, self.engine.flow_cameras(table), not shared, H, W, want_origin=True)
            vis = self.engine.segment_visible(proj["origin"].reshape(-1, 3), pts.reshape(-1, 3), times.repeat_interleave(P), weff.detach(), packed,
                                              self.use_deform, *vis_args)
            status = vis["status"].reshape(F, P)
            out = self.engine.flow_resolve(proj["pixel"], pts, px, tr["points"], tr["valid"], tk["converged"], proj["in_image"], status)
        out.update(points=pts, source_points=tr["points"], source_valid=tr["valid"], converged=tk["converged"], in_image=proj["in_image"],
                   z=proj["z"], status=status, iters=vis["iters"].reshape(F, P))
        return out

    @_on_device
    def frame_flow(self, intrinsics, pose, t_from, times, height, width, intrinsics_to=None, poses_to=None, margin=5e-3, trace_args=None,
                   track_args=None, ray_chunk=65536):
        """``flow.frame_flow``: ``track_pixels`` on the full pixel grid of the source camera, in chunks of ``ray_chunk`` pixels; every
        output shaped [F,H,W,...] (``source_points`` [H,W,3], ``source_valid`` [H,W]).  A row's result does not depend on its chunk."""
        H, W = flow._image_size(height, width)
        C = int(ray_chunk)
        if C < 1:
            raise ValueError(f"ray_chunk must be at least 1 (got {ray_chunk})")
        grid = flow.pixel_grid(H, W, torch.float32, self.device)
        parts = [self.track_pixels(grid[i:i + C], intrinsics, pose, t_from, times, H, W, intrinsics_to, poses_to, margin, trace_args, track_args)
                 for i in range(0, H * W, C)]
        out = {k: torch.cat([p[k] for p in parts], 1) for k in flow.FRAME_KEYS}
        out.update({k: torch.cat([p[k] for p in parts], 0) for k in flow.SOURCE_KEYS})
        return flow.shape_frames(out, H, W)

    @_on_device
    def sample_bilinear(self, image, pixels, valid=None, background=0.0):
        """``flow.sample_bilinear``: ``image`` [H,W,C] at the float ``pixels`` [M,2] -> [M,C]; one launch."""
        img = f32(torch.as_tensor(image).to(device=self.device, dtype=torch.float32))
        return self.engine.sample_bilinear(img, self._flow_f32(pixels, 2).reshape(-1, 2), None if valid is None else torch.as_tensor(valid), background)

    @_on_device
    def stabilize_frames(self, frames, flow_dict, background=0.0):
        """``flow.stabilize_frames``: target frame f of ``frames`` [F,H,W,C] sampled at ``flow_dict["pixels"][f]`` (the dict ``frame_flow``
        returns), so that the tissue holds still in the reference view: dict(frames [F,H,W,C], valid [F,H,W]); one launch for all frames."""
        fr = f32(torch.as_tensor(frames).to(device=self.device, dtype=torch.float32))
        px = self._flow_f32(flow_dict["pixels"], 2)
        valid = torch.as_tensor(flow_dict["valid"]).to(self.device).bool()
        if fr.dim() != 4 or px.dim() != 4 or px.shape[0] != fr.shape[0] or valid.shape != px.shape[:3]:
            raise ValueError(f"frames must be [F, H, W, C] and the flow's pixels [F, h, w, 2] with valid [F, h, w] (got {tuple(fr.shape)}, "
                             f"{tuple(px.shape)}, {tuple(valid.shape)})")
        F, h, w = px.shape[:3]
        out = self.engine.sample_bilinear(fr, px.reshape(F, h * w, 2), valid, background)
        return {"frames": out.reshape(F, h, w, fr.shape[3]), "valid": valid}

    @_on_device
    def flow_to_rgb(self, flow_uv, max_flow):
        """``flow.flow_to_rgb``: uint8 [..., 3] of flow [..., 2]; one launch.  The device's atan2 is its own: a channel may differ from
        the twin's by one level."""
        max_flow = float(max_flow)
        if not (0.0 < max_flow < float("inf")):
            raise ValueError(f"max_flow must be finite and positive (got {max_flow})")
        return self.engine.flow_panel(self._flow_f32(flow_uv, 2), max_flow)

    @_on_device
    def track_errors(self, pred_pixels, pred_visible, gt_pixels, gt_visible, thresholds=(1, 2, 4, 8, 16)):
        """``flow.track_errors`` on the device: torch fp64 reductions, no kernel of the library's; the values are 0-dim device tensors."""
        dev = lambda a: torch.as_tensor(a).to(self.device)
        return flow.track_errors(dev(pred_pixels), dev(pred_visible), dev(gt_pixels), dev(gt_visible), thresholds)
