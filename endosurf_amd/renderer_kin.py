"""Tissue velocity and strain rate of ``renderer.EndoSurfRenderer`` (a mixin): ``kinematics``' functions with the model's own
deformation network under them -- J, dD/dt and the pure second derivatives of D in one launch (csrc/deform_jet.hip), the per-row
algebra in another (csrc/kinematics.hip)."""
from __future__ import annotations

import torch

from . import kinematics
from ._device import _on_device, f32


class RendererKinMixin:
    @_on_device
    def deform_derivatives(self, pts, t):
        """dict(jac [M,3,3] = I + dD/dx, d_t [M,3] = dD/dt, dd [M,3,3] with dd[m,i,k] = d2 D_i / d x_k^2) for [M,3] points and [M] / scalar
        time, no grad: ``kinematics``' ``derivs_fn``, one launch (csrc/deform_jet.hip).  Without a deformation network J = I, D_t = 0,
        dd = 0, and no launch."""
        x = self._track_rows(pts)
        M = x.shape[0]
        tt = self._track_times(t, M)
        if not self.use_deform or M == 0:
            return {"jac": torch.eye(3, device=self.device).expand(M, 3, 3).contiguous(), "d_t": x.new_zeros(M, 3),
                    "dd": x.new_zeros(M, 3, 3)}
        weff, packed = self._weights()
        with torch.no_grad():
            return self.engine.deform_derivatives(self.engine.points(x=x, t=tt), weff.detach(), packed)

    def _kinematics_rows(self, jac, d_t, dd, normals):
        """``kinematics``' ``rows_fn=``: the per-row algebra in one launch (csrc/kinematics.hip), no read-back."""
        return self.engine.kinematics_rows(self._track_rows(jac, 9).reshape(-1, 3, 3), self._track_rows(d_t),
                                           self._track_rows(dd, 9).reshape(-1, 3, 3), None if normals is None else self._track_rows(normals))

    @_on_device
    def point_kinematics(self, pts, t, normals=None):
        """Velocity and strain rate of the tissue seen at [M,3] points at [M] / scalar time ``t`` (``kinematics.point_kinematics``:
        velocity, speed, L, rate, principal_rates, divergence, vorticity, valid and, with ``normals`` of the surface there, area_rate
        and surface_rates; device tensors, no read-back).  One derivative launch and one launch of the algebra."""
        with torch.no_grad():
            return kinematics.point_kinematics(self.deform_derivatives, self._track_rows(pts), t,
                                               None if normals is None else self._track_rows(normals), rows_fn=self._kinematics_rows)

    @_on_device
    def mesh_kinematics(self, track, times, normals=None):
        """The velocity and strain-rate maps of a tracked mesh (``kinematics.mesh_kinematics`` on the dict ``track_mesh`` returns, over
        the same ``times``): every output [F,V,...] on the device, each frame at its own time.  One derivative launch for all F*V rows
        (a time per row) and one launch of the algebra; the default normals are ``Engine.vertex_normals`` of each frame's vertices
        and the track's triangles."""
        dev = {"vertices": f32(torch.as_tensor(track["vertices"]).to(device=self.device, dtype=torch.float32)),
               "converged": torch.as_tensor(track["converged"]).to(self.device),
               "triangles": track["triangles"]}
        times = f32(torch.as_tensor(times).to(device=self.device, dtype=torch.float32)).reshape(-1)
        normals_fn = lambda v, tri: self.engine.vertex_normals(self._track_rows(v), torch.as_tensor(tri).to(self.device))
        if normals is not None:
            normals = f32(torch.as_tensor(normals).to(device=self.device, dtype=torch.float32))
        with torch.no_grad():
            return kinematics.mesh_kinematics(self.deform_derivatives, dev, times, normals, normals_fn=normals_fn,
                                              rows_fn=self._kinematics_rows)
