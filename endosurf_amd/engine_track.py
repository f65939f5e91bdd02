"""The deformation-only methods of ``engine.Engine`` (a mixin): D(x, t) and the inverse of x -> x + D(x, t), csrc/deform.hip."""
from __future__ import annotations

import ctypes as C

import torch

from ._device import f32
from ._lib import check, es_points, ptr


class TrackMixin:
    def deform_forward(self, pts: es_points, weff, packed, want: str = "xc"):
        """x_c = x + D(x, t) (``want="xc"``), D itself (``"d"``) or the pair (``"both"``) for explicit points, [M,3] each: one launch of
        the deformation network alone, fp32 whatever ``split_precision`` says.  No read-back, no synchronisation."""
        if want not in ("xc", "d", "both"):
            raise ValueError(f"want must be 'xc', 'd' or 'both' (got {want!r})")
        xc = self.empty(pts.M, 3) if want != "d" else None
        d = self.empty(pts.M, 3) if want != "xc" else None
        check(self.lib.es_deform_forward(C.byref(pts), ptr(packed), ptr(weff), ptr(xc), ptr(d), self.st()), "es_deform_forward")
        return (xc, d) if want == "both" else (xc if want == "xc" else d)

    def deform_inverse(self, pts: es_points, init, weff, packed, max_iters: int, tol: float):
        """(y [M,3], step [M], iters [M] int32) with y + D(y, t) = c for the points c of ``pts``: the fixed-point iteration of
        ``tracking.inverse_deform``, row rule included, in ONE launch.  ``init`` [M,3] on this device starts the rows (None: from c).
        No read-back, no synchronisation: how many rows converged is the caller's to ask (``step <= tol``)."""
        M = pts.M
        if init is not None:
            if not torch.is_tensor(init) or not init.is_cuda or tuple(init.shape) != (M, 3):
                got = f"{tuple(init.shape)} on {init.device}" if torch.is_tensor(init) else type(init).__name__
                raise ValueError(f"deform_inverse: init must be [{M}, 3] on {self.device} (got {got})")
            init = f32(init)
        y, step, iters = self.empty(M, 3), self.empty(M), self.empty(M, dtype=torch.int32)
        check(self.lib.es_deform_inverse(C.byref(pts), ptr(init), ptr(packed), ptr(weff), int(max_iters), float(tol), ptr(y), ptr(step), ptr(iters),
                                         self.st()), "es_deform_inverse")
        return y, step, iters
