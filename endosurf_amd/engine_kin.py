"""The kinematics methods of ``engine.Engine`` (a mixin): the Jacobian, the time derivative and the pure second derivatives of the
deformation map in one launch, csrc/deform_jet.hip, and the velocity and strain rate row by row, csrc/kinematics.hip."""
from __future__ import annotations

import ctypes as C

import torch

from ._device import f32
from ._lib import check, es_points, ptr


class KinMixin:
    def deform_derivatives(self, pts: es_points, weff, packed, want_xc: bool = False):
        """dict(jac [M,3,3] = I + dD/dx, d_t [M,3] = dD/dt, dd [M,3,3] with dd[m,i,k] = d2 D_i / d x_k^2 and, with ``want_xc``, xc [M,3] =
        x + D) for explicit points: the value, the three spatial tangents, the time tangent and the three pure second tangents in one
        launch of the deformation network alone (csrc/deform_jet.hip), nothing saved, fp32 whatever ``split_precision`` says; ``jac``
        and ``xc`` are ``deform_jacobian``'s bit for bit.  No read-back, no synchronisation."""
        out = {"jac": self.empty(pts.M, 3, 3), "d_t": self.empty(pts.M, 3), "dd": self.empty(pts.M, 3, 3)}
        if want_xc:
            out["xc"] = self.empty(pts.M, 3)
        check(self.lib.es_deform_derivatives(C.byref(pts), ptr(packed), ptr(weff), ptr(out["jac"]), ptr(out["d_t"]), ptr(out["dd"]),
                                             ptr(out.get("xc")), self.st()), "es_deform_derivatives")
        return out

    def kinematics_rows(self, jac, d_t, dd, normals=None):
        """``kinematics.kinematics_rows`` (the specification and the fp64 twin; the diagonal ``dd``, ``d_xt`` zero) on the device,
        csrc/kinematics.hip: ``jac`` [M,3,3], ``d_t`` [M,3], ``dd`` [M,3,3] and ``normals`` ([M,3] or None) on this device ->
        dict(velocity [M,3], speed [M], L [M,3,3], rate [M,3,3], principal_rates [M,3], divergence [M], vorticity [M,3], valid [M] bool
        and, with normals, area_rate [M], surface_rates [M,2]), fp64 arithmetic per row, fp32 results, the same bits from call to call.
        No read-back, no synchronisation."""
        def rows(a, shape, what):
            if not torch.is_tensor(a) or a.device != self.device or tuple(a.shape) != shape:
                got = f"{tuple(a.shape)} on {a.device}" if torch.is_tensor(a) else type(a).__name__
                raise ValueError(f"kinematics_rows: {what} must be {list(shape)} on {self.device} (got {got})")
            return f32(a)
        if not torch.is_tensor(jac) or jac.dim() != 3:
            raise ValueError("kinematics_rows: jac must be an [M, 3, 3] tensor")
        M = int(jac.shape[0])
        jac, d_t, dd = rows(jac, (M, 3, 3), "jac"), rows(d_t, (M, 3), "d_t"), rows(dd, (M, 3, 3), "dd")
        normals = None if normals is None else rows(normals, (M, 3), "normals")
        out = {"velocity": self.empty(M, 3), "speed": self.empty(M), "L": self.empty(M, 3, 3), "rate": self.empty(M, 3, 3),
               "principal_rates": self.empty(M, 3), "divergence": self.empty(M), "vorticity": self.empty(M, 3)}
        if normals is not None:
            out["area_rate"], out["surface_rates"] = self.empty(M), self.empty(M, 2)
        out["valid"] = self.empty(M, dtype=torch.bool)
        check(self.lib.es_kinematics_rows(ptr(jac), ptr(d_t), ptr(dd), ptr(normals), M, ptr(out["velocity"]), ptr(out["speed"]), ptr(out["L"]),
                                          ptr(out["rate"]), ptr(out["principal_rates"]), ptr(out["divergence"]), ptr(out["vorticity"]),
                                          ptr(out.get("area_rate")), ptr(out.get("surface_rates")), ptr(out["valid"]), self.st()),
              "es_kinematics_rows")
        return out
