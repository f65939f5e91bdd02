"""Rigid registration of ``renderer.EndoSurfRenderer`` (a mixin): ``registration``'s functions on the renderer's device -- the rigid
part of a surface track and what is left of it, and the alignment of a point cloud or another mesh onto an extracted mesh by ICP
(csrc/register.hip through ``Engine.track_rigid`` / ``Engine.icp``)."""
from __future__ import annotations

import torch

from ._device import _on_device, f32


def _mesh_pair(mesh):
    return (mesh["vertices"], mesh["triangles"]) if isinstance(mesh, dict) else mesh


class RendererRegMixin:
    def _reg_rows(self, a):
        """Rows (tensor, numpy array or nested list, anywhere) as fp32 on this device."""
        return f32(torch.as_tensor(a).to(device=self.device, dtype=torch.float32))

    @_on_device
    def track_rigid(self, track, reference=0, weights=None):
        """The dict ``track_mesh`` returns (or its [F,V,3] vertices, on any device), extended by the rigid part of the motion and what
        is left (``registration.track_rigid``, device tensors): rotation [F,3,3], translation [F,3], rmse [F] (fp64) and valid [F] of
        the best rigid motion from frame ``reference`` to each frame, residual [F,V,3] and residual_norm [F,V] (fp32), the
        displacement a rigid motion does not explain.  ``weights`` [V] or None."""
        is_dict = isinstance(track, dict)
        v = self._reg_rows(track["vertices"] if is_dict else track)
        w = None if weights is None else self._reg_rows(weights)
        with torch.no_grad():
            fit = self.engine.track_rigid(v, reference=reference, weights=w)
        out = dict(track) if is_dict else {}
        out.update(fit)
        return out

    @_on_device
    def register_points(self, points, mesh, method="plane", max_iters=50, tol=1e-6, max_distance=None, init=None, poll=4):
        """The rigid motion that lays ``points`` [N,3] onto ``mesh`` -- the dict ``extract_observation_mesh`` returns or a
        (vertices, triangles) pair, on any device -- by ICP against its triangles (``registration.icp``, which names the keys of the
        result; tensors on this device).  ICP is local: pass ``init`` = (R, t) for a large motion."""
        vertices, triangles = _mesh_pair(mesh)
        tri = torch.as_tensor(triangles).to(self.device)
        with torch.no_grad():
            return self.engine.icp(self._reg_rows(points), self._reg_rows(vertices), tri, method=method, max_iters=max_iters, tol=tol,
                                   max_distance=max_distance, init=init, poll=poll)

    @_on_device
    def register_mesh(self, source_mesh, mesh, **icp_args):
        """``register_points`` of the vertices of ``source_mesh`` (a mesh dict or a (vertices, triangles) pair): the result of the
        ICP extended by ``vertices`` (the source's vertices moved onto ``mesh``) and ``triangles`` (the source's, as passed in)."""
        vertices, triangles = _mesh_pair(source_mesh)
        out = self.register_points(vertices, mesh, **icp_args)
        out.update(vertices=out["points"], triangles=triangles)
        return out
