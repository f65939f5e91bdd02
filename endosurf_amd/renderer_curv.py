"""Surface curvature of ``renderer.EndoSurfRenderer`` (a mixin): ``curvature``'s functions with the model's own networks under them --
value, gradient and Hessian of the SDF network in one launch (csrc/sdf_hess.hip), composed with the deformation's Jacobian
(csrc/deform_jet.hip) and the curvature of its encodings (the fp32 point forward's ``ES_WS_CURV``) row by row (csrc/curvature.hip,
DESIGN.md 7k)."""
from __future__ import annotations

import torch

from . import _lib, curvature
from ._device import _on_device, f32


class RendererCurvMixin:
    @_on_device
    def sdf_hessian(self, pts, t=None, space="observed"):
        """dict(sdf [M,1], gradient [M,3], hessian [M,3,3]) of the field at [M,3] points, no grad, device tensors, no read-back.
        ``space="canonical"``: ``pts`` are canonical points, the SDF network alone, one launch (``t`` is not read).
        ``space="observed"``: the field sdf(x + D(x, t)) at [M] / scalar time ``t``: J and x_c in one launch, the SDF network's value,
        gradient and Hessian at x_c in another, the curvature of the deformation's encodings from the fp32 point forward, and one
        launch that composes them: gradient = J^T g_c, hessian = J^T H_c J - diag(CURV(g_c)), exact away from the deformation network's
        ReLU kinks.  Without a deformation network J = I and CURV = 0, and the canonical launch is all that runs."""
        if space not in ("observed", "canonical"):
            raise ValueError(f"space must be 'observed' or 'canonical' (got {space!r})")
        x = self._track_rows(pts)
        M = x.shape[0]
        deform = space == "observed" and self.use_deform
        if deform:
            if t is None:
                raise TypeError("sdf_hessian in the observed space needs t, the time of the points")
            tt = self._track_times(t, M)
        if M == 0:
            return {"sdf": x.new_zeros(0, 1), "gradient": x.new_zeros(0, 3), "hessian": x.new_zeros(0, 3, 3)}
        weff, packed = self._weights()
        weff = weff.detach()
        eng = self.engine
        with torch.no_grad():
            if not deform:
                sdf, grad, hess = eng.sdf_hessian(x, weff, packed)
                return {"sdf": sdf[:, None], "gradient": grad, "hessian": hess}
            jac, xc = eng.deform_jacobian(eng.points(x=x, t=tt), weff, packed, want_xc=True)
            sdf, grad_c, hess_c = eng.sdf_hessian(xc, weff, packed)
            ctx = eng.point_forward(eng.points(x=x, t=tt), weff, packed, _lib.PF_DEFORM, fp32_only=True)
            out = eng.curvature_rows(grad_c, hess_c, jac, f32(ctx.view("curv")), curvature=False)
        return {"sdf": sdf[:, None], "gradient": out["gradient"], "hessian": out["hessian"]}

    def _hessian_fn(self, space):
        def fn(x, t):
            h = self.sdf_hessian(x, t, space)
            return h["sdf"], h["gradient"], h["hessian"]
        return fn

    def _curvature_rows(self, gradient, hessian):
        """``curvature``'s ``rows_fn=``: the per-row algebra in one launch (csrc/curvature.hip), no read-back."""
        out = self.engine.curvature_rows(self._track_rows(gradient), self._track_rows(hessian, 9).reshape(-1, 3, 3))
        return {k: out[k] for k in ("mean", "gauss", "principal", "valid")}

    @_on_device
    def surface_curvature(self, pts, t=None, space="observed"):
        """``sdf_hessian(pts, t, space)``'s dict plus the curvature of the level set through each point (``curvature.curvature_rows`` of
        that gradient and Hessian, one more launch): mean [M], gauss [M], principal [M,2] descending, valid [M] bool; the normal points
        towards increasing SDF, so a bulge of the tissue towards the camera has positive curvature.  Points from ``trace_surface``
        (``out["points"][out["valid"]]`` with the rays' times) lie on the surface to its ``eps``."""
        with torch.no_grad():
            return curvature.surface_curvature(self._hessian_fn(space), self._track_rows(pts), 0.0 if t is None else t,
                                               rows_fn=self._curvature_rows)

    @_on_device
    def mesh_curvature(self, mesh_or_track, t=None, times=None):
        """The curvature maps of a mesh in the observed space (``curvature.mesh_curvature``): [V,3] vertices or a mesh dict seen at time
        ``t`` -> mean, gauss, valid [V], principal [V,2]; the dict ``track_mesh`` returns with its ``times`` [F] -> [F,V] maps, one batch
        for all F*V rows (a time per row), rows of unconverged track entries not valid and zero.  Device tensors, no read-back."""
        if isinstance(mesh_or_track, dict) and "converged" in mesh_or_track:
            if times is None:
                raise TypeError("mesh_curvature of a track needs times, the times it was tracked through")
            dev = {"vertices": f32(torch.as_tensor(mesh_or_track["vertices"]).to(device=self.device, dtype=torch.float32)),
                   "converged": torch.as_tensor(mesh_or_track["converged"]).to(self.device)}
            when = f32(torch.as_tensor(times).to(device=self.device, dtype=torch.float32)).reshape(-1)
        else:
            if t is None:
                raise TypeError("mesh_curvature of a mesh needs t, the time of its vertices")
            dev = self._track_rows(mesh_or_track["vertices"] if isinstance(mesh_or_track, dict) else mesh_or_track)
            when = t
        with torch.no_grad():
            return curvature.mesh_curvature(self._hessian_fn("observed"), dev, when, rows_fn=self._curvature_rows)
