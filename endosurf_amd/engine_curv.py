"""The curvature methods of ``engine.Engine`` (a mixin): value, gradient and Hessian of the SDF network in one launch,
csrc/sdf_hess.hip, and the composition with the deformation and the curvatures row by row, csrc/curvature.hip."""
from __future__ import annotations

import ctypes as C

import torch

from ._device import f32
from ._lib import check, es_points, ptr


class CurvMixin:
    def sdf_hessian(self, xc, weff, packed, tile_rows: int = 0):
        """(sdf [M], gradient [M,3], hessian [M,3,3]) of the SDF network at the canonical points ``xc`` [M,3] on this device: second-order
        forward mode in one launch (csrc/sdf_hess.hip), nothing saved, fp32 whatever ``split_precision`` says; the Hessian is symmetric
        bit for bit.  ``tile_rows``: 32 or 64 MLP rows per workgroup, 0 = the library's choice; the two give the same bits.  No
        read-back, no synchronisation."""
        if not torch.is_tensor(xc) or xc.device != self.device or xc.dim() != 2 or xc.shape[1] != 3:
            got = f"{tuple(xc.shape)} on {xc.device}" if torch.is_tensor(xc) else type(xc).__name__
            raise ValueError(f"Engine.sdf_hessian: xc must be [M, 3] on {self.device}; device tensors only (got {got})")
        if tile_rows not in (0, 32, 64):
            raise ValueError(f"tile_rows must be 0 (the library's choice), 32 or 64 (got {tile_rows})")
        xc = f32(xc)
        M = int(xc.shape[0])
        p = es_points()
        p.x, p.mode, p.n_per_ray, p.ldz, p.M = ptr(xc), 0, 1, 1, M
        sdf, grad, hess = self.empty(M), self.empty(M, 3), self.empty(M, 3, 3)
        check(self.lib.es_sdf_hessian(C.byref(p), ptr(packed), ptr(weff), int(tile_rows), ptr(sdf), ptr(grad), ptr(hess), self.st()),
              "es_sdf_hessian")
        return sdf, grad, hess

    def curvature_rows(self, grad_c, hess_c, jac=None, dd=None, curvature: bool = True):
        """``curvature.compose_hessian`` and ``curvature.curvature_rows`` (the specification and the fp64 twin) on the device,
        csrc/curvature.hip: ``grad_c`` [M,3], ``hess_c`` [M,3,3], ``jac`` ([M,3,3] or None: the identity) and ``dd`` ([M,3] or None: zero)
        on this device -> dict(gradient [M,3] = J^T g_c, hessian [M,3,3] = J^T H_c J - diag(dd), mean [M], gauss [M], principal [M,2],
        valid [M] bool), fp64 arithmetic per row, fp32 results, the same bits from call to call; ``curvature=False``: the first two
        only.  No read-back, no synchronisation."""
        def rows(a, shape, what):
            if not torch.is_tensor(a) or a.device != self.device or tuple(a.shape) != shape:
                got = f"{tuple(a.shape)} on {a.device}" if torch.is_tensor(a) else type(a).__name__
                raise ValueError(f"curvature_rows: {what} must be {list(shape)} on {self.device} (got {got})")
            return f32(a)
        if not torch.is_tensor(grad_c) or grad_c.dim() != 2:
            raise ValueError("curvature_rows: grad_c must be an [M, 3] tensor")
        M = int(grad_c.shape[0])
        grad_c, hess_c = rows(grad_c, (M, 3), "grad_c"), rows(hess_c, (M, 3, 3), "hess_c")
        jac = None if jac is None else rows(jac, (M, 3, 3), "jac")
        dd = None if dd is None else rows(dd, (M, 3), "dd")
        out = {"gradient": self.empty(M, 3), "hessian": self.empty(M, 3, 3)}
        if curvature:
            out.update(mean=self.empty(M), gauss=self.empty(M), principal=self.empty(M, 2), valid=self.empty(M, dtype=torch.bool))
        check(self.lib.es_curvature_rows(ptr(grad_c), ptr(hess_c), ptr(jac), ptr(dd), M, ptr(out["gradient"]), ptr(out["hessian"]),
                                         ptr(out.get("mean")), ptr(out.get("gauss")), ptr(out.get("principal")), ptr(out.get("valid")),
                                         self.st()), "es_curvature_rows")
        return out
