"""Geodesic distance of ``renderer.EndoSurfRenderer`` (a mixin): ``geodesic``'s functions on the renderer's device -- distance fields
along an extracted or tracked mesh, and the length between paired landmarks over the frames of a track (csrc/geodesic.hip through
``Engine.geodesic``)."""
from __future__ import annotations

import torch

from . import geodesic
from ._device import _on_device, f32


class RendererGeoMixin:
    def _geodesic_points(self, a):
        """Sources or targets (tensor, numpy array or nested list, anywhere) on this device: integers stay vertex ids, floats are fp32."""
        a = torch.as_tensor(a)
        return a.to(self.device) if not a.is_floating_point() else f32(a.to(device=self.device, dtype=torch.float32))

    @_on_device
    def mesh_geodesic(self, mesh_or_track, sources, targets=None, reference=0, poll=8):
        """Geodesic distance fields on a mesh (``geodesic.mesh_geodesic``, device tensors): ``mesh_or_track`` is the dict
        ``extract_observation_mesh`` returns, the dict ``track_mesh`` returns (its [F,V,3] vertices: a field per frame and source) or a
        (vertices, triangles) pair, on any device; ``sources`` an integer [S] array of vertex ids or [S,3] points, ``targets`` [Q,3]
        points or None, both given in frame ``reference``.  dict(distance [F,S,V] / [S,V], sweeps, target_distance [F,S,Q] / [S,Q])."""
        if isinstance(mesh_or_track, dict):
            vertices, triangles = mesh_or_track["vertices"], mesh_or_track["triangles"]
        else:
            vertices, triangles = mesh_or_track
        v = f32(torch.as_tensor(vertices).to(device=self.device, dtype=torch.float32))
        tri = torch.as_tensor(triangles).to(self.device)
        with torch.no_grad():
            return self.engine.geodesic(v, tri, self._geodesic_points(sources), None if targets is None else self._geodesic_points(targets),
                                        reference=reference, poll=poll)

    @_on_device
    def track_geodesic(self, track, points_a, points_b, reference=0):
        """[F,S] lengths along the tissue between the paired landmarks ``points_a[s]``, ``points_b[s]`` ([S,3], given in frame
        ``reference``) over the frames of a ``track_mesh`` dict (``geodesic.track_geodesic``): one launch per sweep for all F*S fields."""
        return geodesic.track_geodesic(track, points_a, points_b, reference,
                                       mesh_fn=lambda v, tri, a, targets, reference: self.mesh_geodesic((v, tri), a, targets, reference))
