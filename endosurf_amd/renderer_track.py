"""The surface tracks of ``renderer.EndoSurfRenderer`` (a mixin): ``tracking``'s functions with the model's own deformation network
under them -- D(x, t) in one launch of the deformation network alone, the inverse as one launch per solve (csrc/deform.hip) -- and
``strain``'s functions likewise: the Jacobian of the deformation in one launch (csrc/deform_jet.hip), the per-row algebra in another
(csrc/strain.hip)."""
from __future__ import annotations

import torch

from . import strain, tracking
from ._device import _on_device, f32

# The default stopping length of the device solver, where the host twin's fp64 default is 1e-6: fp32 evaluation noise of D is of order
# 1e-7, the step of a row that has arrived is that noise, and a step length cannot be trusted much below ten times it.
TRACK_TOL = 1e-5


class RendererTrackMixin:
    def _track_rows(self, a, width=3):
        """``a`` (tensor, numpy array or nested list, anywhere) as the library reads it: fp32 [M, width], contiguous, on this device."""
        return f32(torch.as_tensor(a).to(device=self.device, dtype=torch.float32)).reshape(-1, width)

    def _track_times(self, t, M):
        """``t`` (Python float, [1] or [M], anywhere) as fp32 on this device: [1] for a shared time, else [M].  One value expanded to M
        rows (``tracking`` hands a shared time on that way) is a shared time again: the kernel reads it as ``t_scalar``."""
        tt = torch.as_tensor(t).to(device=self.device, dtype=torch.float32).reshape(-1)
        if tt.numel() > 1 and tt.stride(0) == 0:
            tt = tt[:1]
        tt = f32(tt)
        if tt.numel() != 1 and tt.numel() != M:
            raise ValueError(f"t must be a scalar or one time per row (got {tt.numel()} for {M} rows)")
        return tt

    @_on_device
    def deform(self, pts, t):
        """D(x, t) [M,3] for [M,3] points and [M] / scalar time, no grad: ``tracking``'s ``deform_fn``.  A scalar time is read by the
        kernel as one shared value.  Zeros without a deformation network."""
        x = self._track_rows(pts)
        M = x.shape[0]
        tt = self._track_times(t, M)
        if not self.use_deform or M == 0:
            return torch.zeros_like(x)
        weff, packed = self._weights()
        with torch.no_grad():
            return self.engine.deform_forward(self.engine.points(x=x, t=tt), weff.detach(), packed, want="d")

    def _inverse(self, c, t, init, max_iters, tol):
        """``tracking``'s ``inverse=``: the whole fixed-point iteration in one launch, no read-back."""
        if int(max_iters) < 1:
            raise ValueError(f"max_iters must be at least 1 (got {max_iters})")
        tol = float(tol)
        if not (0.0 <= tol < float("inf")):
            raise ValueError(f"tol must be finite and not negative (got {tol})")
        c = self._track_rows(c)
        M = c.shape[0]
        tt = self._track_times(t, M)
        if init is not None:
            init = self._track_rows(init)
        if M == 0:
            return c.clone(), c.new_zeros(0), torch.zeros(0, dtype=torch.int32, device=self.device)
        weff, packed = self._weights()
        with torch.no_grad():
            return self.engine.deform_inverse(self.engine.points(x=c, t=tt), init, weff.detach(), packed, int(max_iters), tol)

    def _track_solver(self):
        """Without a deformation network D = 0 and the host twin runs on device tensors: nothing of csrc/deform.hip is launched."""
        return self._inverse if self.use_deform else None

    @_on_device
    def to_canonical(self, pts, t):
        """x_c = x + D(x, t) for [M,3] points and [M] / scalar time, no grad; a device tensor."""
        with torch.no_grad():
            return tracking.to_canonical(self.deform, self._track_rows(pts), t)

    @_on_device
    def to_observed(self, canonical, t, init=None, max_iters=64, tol=TRACK_TOL):
        """The observed positions at ``t`` of canonical points, ``tracking.to_observed``'s dict (points, step, iters, converged) as device
        tensors with no read-back; one launch.  ``tol`` defaults to 1e-5, not the host twin's 1e-6: the fp32 evaluation noise of D is
        of order 1e-7, and a step length cannot be trusted much below ten times that."""
        with torch.no_grad():
            return tracking.to_observed(self.deform, self._track_rows(canonical), t, None if init is None else self._track_rows(init),
                                        max_iters, tol, inverse=self._track_solver())

    @_on_device
    def warp_points(self, pts, t_from, t_to, init=None, max_iters=64, tol=TRACK_TOL):
        """Where the tissue seen at ``pts`` at ``t_from`` is at ``t_to`` (``tracking.warp_points``): two launches, device tensors."""
        with torch.no_grad():
            return tracking.warp_points(self.deform, self._track_rows(pts), t_from, t_to, None if init is None else self._track_rows(init),
                                        max_iters, tol, inverse=self._track_solver())

    @_on_device
    def track_points(self, pts, t_from, times, warm_start=False, max_iters=64, tol=TRACK_TOL):
        """``pts`` [P,3] seen at ``t_from`` followed through ``times`` [F] (``tracking.track_points``, same keys and shapes, device
        tensors, no read-back).  Cold: one launch for all F*P rows; ``warm_start``: one launch per frame, each from the frame before."""
        times = f32(torch.as_tensor(times).to(device=self.device, dtype=torch.float32)).reshape(-1)
        with torch.no_grad():
            return tracking.track_points(self.deform, self._track_rows(pts), t_from, times, warm_start, max_iters, tol,
                                         inverse=self._track_solver())

    @_on_device
    def track_mesh(self, mesh_or_vertices, triangles=None, t=None, times=None, warm_start=True, max_iters=64, tol=TRACK_TOL):
        """The mesh seen at time ``t`` carried through ``times`` (``tracking.track_mesh``: vertices [F,V,3], triangles -- the object
        passed in --, canonical, displacement, step, iters, converged).  ``mesh_or_vertices``: [V,3] vertices with ``triangles``, or
        the dict ``extract_observation_mesh`` returns (its ``vertices`` and ``triangles``)."""
        if isinstance(mesh_or_vertices, dict):
            if triangles is not None:
                raise TypeError("track_mesh takes a mesh dict or (vertices, triangles), not both")
            vertices, triangles = mesh_or_vertices["vertices"], mesh_or_vertices["triangles"]
        else:
            vertices = mesh_or_vertices
        if t is None or times is None:
            raise TypeError("track_mesh needs t, the time of the given vertices, and times")
        times = f32(torch.as_tensor(times).to(device=self.device, dtype=torch.float32)).reshape(-1)
        with torch.no_grad():
            return tracking.track_mesh(self.deform, self._track_rows(vertices), triangles, t, times, warm_start, max_iters, tol,
                                       inverse=self._track_solver())

    # ---- strain along the tracks (strain.py) -----------------------------------------------------------------------------
    @_on_device
    def deform_jacobian(self, pts, t):
        """J(x, t) = I + dD/dx [M,3,3] (dim_out, dim_in) for [M,3] points and [M] / scalar time, no grad: ``strain``'s ``jacobian_fn``,
        one launch (csrc/deform_jet.hip).  Identities, and no launch, without a deformation network."""
        x = self._track_rows(pts)
        M = x.shape[0]
        tt = self._track_times(t, M)
        if not self.use_deform or M == 0:
            return torch.eye(3, device=self.device).expand(M, 3, 3).contiguous()
        weff, packed = self._weights()
        with torch.no_grad():
            return self.engine.deform_jacobian(self.engine.points(x=x, t=tt), weff.detach(), packed)

    def _strain_rows(self, jac_from, jac_to, normals):
        """``strain``'s ``rows_fn=``: the per-row algebra in one launch (csrc/strain.hip), no read-back."""
        return self.engine.strain_rows(None if jac_from is None else self._track_rows(jac_from, 9).reshape(-1, 3, 3),
                                       self._track_rows(jac_to, 9).reshape(-1, 3, 3), None if normals is None else self._track_rows(normals))

    @_on_device
    def track_strain(self, points_from, t_from, points_to, t_to, normals=None):
        """The strain of the tissue between the two ends of track rows (``strain.track_strain``: F, det, stretch, valid and, with
        ``normals`` at the "from" end, area and surface_stretch; device tensors, no read-back): ``points_from`` at ``t_from`` and
        ``points_to`` at ``t_to`` are the same tissue, e.g. ``pts`` and ``warp_points(pts, t_from, t_to)["points"]``.
        ``points_from=None``: relative to the canonical shape.  One Jacobian launch per end and one strain launch."""
        with torch.no_grad():
            return strain.track_strain(self.deform_jacobian, None if points_from is None else self._track_rows(points_from), t_from,
                                       self._track_rows(points_to), t_to, None if normals is None else self._track_rows(normals),
                                       rows_fn=self._strain_rows)

    @_on_device
    def mesh_strain(self, track, times, reference=0, normals=None):
        """The strain maps of a tracked mesh (``strain.mesh_strain`` on the dict ``track_mesh`` returns, over the same ``times``):
        every frame against frame ``reference`` or against ``"canonical"``, every output [F,V,...] on the device.  One Jacobian launch
        for all F*V rows (a time per row) and one strain launch; the default normals are ``Engine.vertex_normals`` of the reference
        vertices and the track's triangles."""
        dev = {"vertices": f32(torch.as_tensor(track["vertices"]).to(device=self.device, dtype=torch.float32)),
               "converged": torch.as_tensor(track["converged"]).to(self.device),
               "triangles": track["triangles"]}
        if isinstance(reference, str):
            dev["canonical"] = self._track_rows(track["canonical"])
        times = f32(torch.as_tensor(times).to(device=self.device, dtype=torch.float32)).reshape(-1)
        normals_fn = lambda v, tri: self.engine.vertex_normals(self._track_rows(v), torch.as_tensor(tri).to(self.device))
        with torch.no_grad():
            return strain.mesh_strain(self.deform_jacobian, dev, times, reference, None if normals is None else self._track_rows(normals),
                                      normals_fn=normals_fn, rows_fn=self._strain_rows)
