"""The surface-tracing method of ``engine.Engine`` (a mixin): rays to surface hits in one launch, csrc/trace.hip."""
from __future__ import annotations

import torch

from . import tracing
from ._device import f32
from ._lib import check, ptr


class TraceMixin:
    def trace_surface(self, rays, weff, packed, use_deform, tau=0.0, eps=1e-5, relax=1.0, min_step=1e-3, max_iters=128, tile_points=0):
        """``tracing.trace_surface`` (the specification and the fp64 twin, row rule included) for ``rays`` [N,9] on this device: dict(depth
        [N,1], status [N] int32, iters [N] int32, residual [N], points [N,3]), the whole iteration of a tile's rays in ONE launch, fp32
        whatever ``split_precision`` says.  ``tile_points``: 32 or 64 rays per workgroup, 0 = the library's choice; the two give the same bits.
        No read-back, no synchronisation: which rays hit is the caller's to ask (``status == tracing.HIT``)."""
        if not torch.is_tensor(rays) or not rays.is_cuda or rays.dim() != 2 or rays.shape[1] != 9:
            got = f"{tuple(rays.shape)} on {rays.device}" if torch.is_tensor(rays) else type(rays).__name__
            raise ValueError(f"Engine.trace_surface: rays must be [N, 9] on {self.device}; device tensors only (got {got})")
        if tile_points not in (0, 32, 64):
            raise ValueError(f"tile_points must be 0 (the library's choice), 32 or 64 (got {tile_points})")
        tau, eps, relax, min_step, max_iters = tracing.check_trace_args(tau, eps, relax, min_step, max_iters)
        rays = f32(rays)
        N = rays.shape[0]
        out = {"depth": self.empty(N, 1), "status": self.empty(N, dtype=torch.int32), "iters": self.empty(N, dtype=torch.int32),
               "residual": self.empty(N), "points": self.empty(N, 3)}
        check(self.lib.es_trace_surface(ptr(rays), N, tau, eps, relax, min_step, max_iters, int(tile_points), ptr(packed), ptr(weff),
                                        int(bool(use_deform)), ptr(out["depth"]), ptr(out["status"]), ptr(out["iters"]), ptr(out["residual"]),
                                        ptr(out["points"]), self.st()), "es_trace_surface")
        return out
