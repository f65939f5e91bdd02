"""The image-side methods of ``engine.Engine`` (a mixin): the segment visibility query in one launch (csrc/visible.hip) and the
elementwise kernels of the pixel tracks (csrc/flow.hip); ``flow`` is the specification and the fp64 twin.  Arguments and
results are device tensors; nothing is read back."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import flow
from ._device import f32, u8
from ._lib import EndoSurfHipError, check, ptr


class FlowMixin:
    def _flow_dev(self, a, what, last, dtype=torch.float32):
        if not torch.is_tensor(a) or a.device != self.device or a.dim() < 1 or (last and a.shape[-1] != last):
            got = f"{tuple(a.shape)} on {a.device}" if torch.is_tensor(a) else type(a).__name__
            raise ValueError(f"Engine.{what} takes [..., {last}] tensors on {self.device}; device tensors only (got {got})")
        return a.detach().to(dtype).contiguous()

    @staticmethod
    def _flow_rows(F, P, what):
        if 3 * F * P > flow.MAX_ROWS:
            raise EndoSurfHipError(f"{what}: {F} x {P} rows do not fit int32 indices")

    def segment_visible(self, origins, points, t, weff, packed, use_deform, margin=5e-3, tau=0.0, relax=1.0, min_step=1e-3, max_iters=128,
                        tile_points=0):
        """``flow.segment_visible`` (the specification and the fp64 twin, row rule included) for ``origins``, ``points`` [M,3] and ``t``
        [M] or [1] on this device: dict(status [M] int32, iters [M] int32, blocker [M], clearance [M], free_to [M]), the whole walk of a tile's
        segments in ONE launch, fp32 whatever ``split_precision`` says.  ``tile_points``: 32 or 64 rows per workgroup, 0 = the
        library's choice; the two give the same bits.  No read-back, no synchronisation."""
        a, b = self._flow_dev(origins, "segment_visible", 3).reshape(-1, 3), self._flow_dev(points, "segment_visible", 3).reshape(-1, 3)
        tt = self._flow_dev(t, "segment_visible", 0).reshape(-1)
        M = a.shape[0]
        if b.shape[0] != M or tt.numel() not in (1, M):
            raise ValueError(f"segment_visible: {M} origins take {M} points and 1 or {M} times (got {b.shape[0]}, {tt.numel()})")
        if tile_points not in (0, 32, 64):
            raise ValueError(f"tile_points must be 0 (the library's choice), 32 or 64 (got {tile_points})")
        margin, tau, relax, min_step, max_iters = flow.check_visible_args(margin, tau, relax, min_step, max_iters)
        self._flow_rows(1, M, "segment_visible")
        out = {"status": self.empty(M, dtype=torch.int32), "iters": self.empty(M, dtype=torch.int32), "blocker": self.empty(M),
               "clearance": self.empty(M), "free_to": self.empty(M)}
        check(self.lib.es_segment_visible(ptr(a), ptr(b), ptr(tt), int(tt.numel() == 1), M, margin, tau, relax, min_step, max_iters,
                                          int(tile_points), ptr(packed), ptr(weff), int(bool(use_deform)), ptr(out["status"]),
                                          ptr(out["iters"]), ptr(out["blocker"]), ptr(out["clearance"]), ptr(out["free_to"]), self.st()), "es_segment_visible")
        return out

    def pixel_rays(self, pixels, camera, t):
        """``flow.pixel_rays`` on the device: rays [P,9] through ``pixels`` [P,2]; ``camera`` = ``flow.ray_camera``'s 21 doubles."""
        px = self._flow_dev(pixels, "pixel_rays", 2).reshape(-1, 2)
        cam = np.ascontiguousarray(camera, np.float64).reshape(21)
        P = px.shape[0]
        self._flow_rows(1, 3 * P, "pixel_rays")
        rays = self.empty(P, 9)
        check(self.lib.es_pixel_rays(ptr(px), P, cam.ctypes.data_as(C.POINTER(C.c_double)), float(t), ptr(rays), self.st()), "es_pixel_rays")
        return rays

    def flow_cameras(self, table):
        """``flow.camera_table``'s [F,17] fp64 as the device buffer ``flow_project`` reads."""
        return torch.from_numpy(np.ascontiguousarray(table, np.float64)).to(self.device)

    def flow_project(self, points, cameras, per_frame, height=0, width=0, want_origin=False):
        """``points`` [F,P,3] through ``cameras`` (``flow_cameras``: [F,17] with ``per_frame``, else [1,17] for all) in one launch:
        dict(pixel [F,P,2], z [F,P], front [F,P] bool and, with ``height`` and ``width``, in_image [F,P] bool; with ``want_origin``,
        origin [F,P,3] = the camera centre of each row's frame)."""
        pts = self._flow_dev(points, "flow_project", 3)
        if pts.dim() != 3 or cameras.dtype != torch.float64 or cameras.device != self.device or tuple(cameras.shape) != (pts.shape[0] if per_frame else 1, 17):
            raise ValueError(f"flow_project takes points [F, P, 3] and fp64 cameras [F, 17] (per_frame) or [1, 17] on {self.device} "
                             f"(got {tuple(pts.shape)}, {tuple(cameras.shape)} {cameras.dtype})")
        F, P = int(pts.shape[0]), int(pts.shape[1])
        self._flow_rows(F, P, "flow_project")
        out = {"pixel": self.empty(F, P, 2), "z": self.empty(F, P), "front": self.empty(F, P, dtype=torch.uint8)}
        if height or width:
            out["in_image"] = self.empty(F, P, dtype=torch.uint8)
        if want_origin:
            out["origin"] = self.empty(F, P, 3)
        check(self.lib.es_flow_project(ptr(pts), F, P, ptr(cameras.contiguous()), int(bool(per_frame)), int(height), int(width), ptr(out["pixel"]),
                                       ptr(out["z"]), ptr(out["front"]), ptr(out.get("in_image")), ptr(out.get("origin")), self.st()),
              "es_flow_project")
        for k in ("front", "in_image"):
            if k in out:
                out[k] = out[k].view(torch.bool)
        return out

    def flow_resolve(self, pixel, points, source_pixels, source_points, source_valid, converged, in_image, status):
        """``flow.resolve`` in one launch: dict(visible, valid [F,P] bool, pixels, flow [F,P,2], scene_flow [F,P,3])."""
        pts = self._flow_dev(points, "flow_resolve", 3)
        F, P = int(pts.shape[0]), int(pts.shape[1])
        self._flow_rows(F, P, "flow_resolve")
        px = self._flow_dev(pixel, "flow_resolve", 2)
        spx, spt = self._flow_dev(source_pixels, "flow_resolve", 2), self._flow_dev(source_points, "flow_resolve", 3)
        sv, cv, ii = u8(source_valid), u8(converged), u8(in_image)
        st = self._flow_dev(status, "flow_resolve", 0, torch.int32)
        if (tuple(px.shape), tuple(spx.shape), tuple(spt.shape), sv.numel(), cv.numel(), ii.numel(), st.numel()) != \
                ((F, P, 2), (P, 2), (P, 3), P, F * P, F * P, F * P):
            raise ValueError(f"flow_resolve: the rows of {F} frames x {P} points do not pair up")
        out = {"visible": self.empty(F, P, dtype=torch.uint8), "valid": self.empty(F, P, dtype=torch.uint8), "pixels": self.empty(F, P, 2),
               "flow": self.empty(F, P, 2), "scene_flow": self.empty(F, P, 3)}
        check(self.lib.es_flow_resolve(ptr(px), ptr(pts), ptr(spx), ptr(spt), ptr(sv), ptr(cv), ptr(ii), ptr(st), F, P, ptr(out["visible"]),
                                       ptr(out["valid"]), ptr(out["pixels"]), ptr(out["flow"]), ptr(out["scene_flow"]), self.st()),
              "es_flow_resolve")
        out["visible"], out["valid"] = out["visible"].view(torch.bool), out["valid"].view(torch.bool)
        return out

    def sample_bilinear(self, images, pixels, valid=None, background=0.0):
        """``flow.sample_bilinear`` on the device, one launch: ``images`` [H,W,C] at ``pixels`` [M,2] -> [M,C]; or ``images`` [F,H,W,C] at
        ``pixels`` [F,R,2] -> [F,R,C], frame f's rows in image f (``flow.stabilize_frames``)."""
        img = self._flow_dev(images, "sample_bilinear", 0)
        if img.dim() not in (3, 4):
            raise ValueError(f"sample_bilinear takes an image [H, W, C] or images [F, H, W, C] (got {tuple(img.shape)})")
        px = self._flow_dev(pixels, "sample_bilinear", 2)
        if img.dim() == 4 and (px.dim() != 3 or px.shape[0] != img.shape[0]):
            raise ValueError(f"images {tuple(img.shape)} take pixels [F, R, 2] (got {tuple(px.shape)})")
        n, rows = (1, max(px.numel() // 2, 1)) if img.dim() == 3 else (int(img.shape[0]), max(int(px.shape[1]), 1))
        H, W, Cn = (int(s) for s in img.shape[-3:])
        M = px.numel() // 2
        if n == 0 or M == 0:
            return self.empty(*px.shape[:-1], Cn) if img.dim() == 4 else self.empty(M, Cn)
        if valid is not None:
            valid = u8(valid.to(self.device)).reshape(-1)
            if valid.numel() != M:
                raise ValueError(f"sample_bilinear: {M} pixels take {M} flags (got {valid.numel()})")
        bg = f32(torch.as_tensor(background, dtype=torch.float32).to(self.device).expand(Cn))
        out = self.empty(*px.shape[:-1], Cn) if img.dim() == 4 else self.empty(M, Cn)
        check(self.lib.es_sample_bilinear(ptr(img), n, H, W, Cn, ptr(px), ptr(valid), M, rows, ptr(bg), ptr(out), self.st()), "es_sample_bilinear")
        return out

    def flow_panel(self, flow_uv, max_flow):
        """``flow.flow_to_rgb`` on the device: uint8 [..., 3] of flow [..., 2], one launch."""
        fl = self._flow_dev(flow_uv, "flow_panel", 2)
        n = fl.numel() // 2
        rgb = self.empty(*fl.shape[:-1], 3, dtype=torch.uint8)
        check(self.lib.es_flow_panel(ptr(fl), n, float(max_flow), ptr(rgb), self.st()), "es_flow_panel")
        return rgb
