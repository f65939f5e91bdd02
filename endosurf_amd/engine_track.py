"""The deformation-only methods of ``engine.Engine`` (a mixin): D(x, t) and the inverse of x -> x + D(x, t), csrc/deform.hip; the
Jacobian of that map in one launch, csrc/deform_jet.hip, and the strain of the tracked map row by row, csrc/strain.hip."""
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

    def deform_jacobian(self, pts: es_points, weff, packed, want_xc: bool = False):
        """J(x, t) = I + dD/dx [M,3,3] (dim_out, dim_in) for explicit points, with ``want_xc`` the pair (J, x_c = x + D [M,3]): the
        value and the three forward tangents in one launch of the deformation network alone (csrc/deform_jet.hip), nothing saved, fp32
        whatever ``split_precision`` says.  No read-back, no synchronisation."""
        jac = self.empty(pts.M, 3, 3)
        xc = self.empty(pts.M, 3) if want_xc else None
        check(self.lib.es_deform_jacobian(C.byref(pts), ptr(packed), ptr(weff), ptr(jac), ptr(xc), self.st()), "es_deform_jacobian")
        return (jac, xc) if want_xc else jac

    def strain_rows(self, jac_from, jac_to, normals=None):
        """``strain.strain_rows`` (the specification and the fp64 twin) on the device, csrc/strain.hip: ``jac_from`` ([M,3,3] or None:
        the identity), ``jac_to`` [M,3,3] and ``normals`` ([M,3] or None) on this device -> dict(F [M,3,3], det [M], stretch [M,3],
        valid [M] bool and, with normals, area [M], surface_stretch [M,2]), fp64 arithmetic per row, fp32 results, the same bits from
        call to call.  No read-back, no synchronisation."""
        def rows(a, shape, what):
            if not torch.is_tensor(a) or a.device != self.device or tuple(a.shape) != shape:
                got = f"{tuple(a.shape)} on {a.device}" if torch.is_tensor(a) else type(a).__name__
                raise ValueError(f"strain_rows: {what} must be {list(shape)} on {self.device} (got {got})")
            return f32(a)
        if not torch.is_tensor(jac_to) or jac_to.dim() != 3:
            raise ValueError("strain_rows: jac_to must be an [M, 3, 3] tensor")
        M = int(jac_to.shape[0])
        jac_to = rows(jac_to, (M, 3, 3), "jac_to")
        jac_from = None if jac_from is None else rows(jac_from, (M, 3, 3), "jac_from")
        normals = None if normals is None else rows(normals, (M, 3), "normals")
        out = {"F": self.empty(M, 3, 3), "det": self.empty(M), "stretch": self.empty(M, 3)}
        if normals is not None:
            out["area"], out["surface_stretch"] = self.empty(M), self.empty(M, 2)
        out["valid"] = self.empty(M, dtype=torch.bool)
        check(self.lib.es_strain_rows(ptr(jac_from), ptr(jac_to), ptr(normals), M, ptr(out["F"]), ptr(out["det"]), ptr(out["stretch"]),
                                      ptr(out.get("area")), ptr(out.get("surface_stretch")), ptr(out["valid"]), self.st()), "es_strain_rows")
        return out
