"""Depth fusion of ``renderer.EndoSurfRenderer`` (a mixin): ``fusion``'s functions with the model's own deformation network under them
-- a TSDF volume of the depth frames in canonical space, each canonical voxel carried to a frame's time by the inverse deformation (one
launch per solve, csrc/deform.hip) and integrated by csrc/fuse.hip; its observed-only mesh; and the per-vertex coverage of any mesh or
track.  Outputs are device tensors under the twin's keys and shapes; host inputs are moved to the renderer's device."""
from __future__ import annotations

import math

import torch

from . import flow, fusion
from ._device import _on_device, f32
from .data import write_ply
from .renderer_mesh import _Lattice
from .renderer_track import TRACK_TOL


class RendererFuseMixin:
    def _fuse_f32(self, a, dim, what):
        r = torch.as_tensor(a)
        if r.dim() != dim:
            raise ValueError(f"{what} must have {dim} dimensions (got {tuple(r.shape)})")
        return f32(r.to(device=self.device, dtype=torch.float32))

    def _fuse_volume(self, volume):
        """A volume dict (``fuse_depth``'s, or the host twin's) with its arrays as fp32 tensors on this device."""
        out = dict(volume)
        for k, dim in (("tsdf", 3), ("weight", 3), ("color", 4)):
            out[k] = None if volume.get(k) is None else self._fuse_f32(volume[k], dim, k)
        R = out["tsdf"].shape[0]
        if tuple(out["tsdf"].shape) != (R, R, R) or out["weight"].shape != out["tsdf"].shape or R < 2:
            raise ValueError(f"a volume holds tsdf and weight [R, R, R] with R >= 2 (got {tuple(out['tsdf'].shape)}, {tuple(out['weight'].shape)})")
        return out

    @_on_device
    def fuse_depth(self, depths, intrinsics, poses, times, bound_min, bound_max, resolution=128, colors=None, masks=None, space="canonical",
                   trunc=None, depth_trunc=math.inf, max_iters=64, tol=TRACK_TOL, voxel_chunk=1 << 18, frame_block=8):
        """``fusion.fuse_depth`` with the model's deformation network: the TSDF volume of the depth frames ``depths`` [F,H,W] (z-depth;
        ``colors`` [F,H,W,3], ``masks`` [F,H,W], each or None) seen by ``intrinsics`` / ``poses`` [F,4,4] at ``times`` [F], on the
        resolution^3 lattice of (bound_min, bound_max).  ``space="canonical"``: the lattice is canonical and every voxel is carried
        to each frame's time by ``to_observed`` (rows that did not converge in ``max_iters`` to ``tol`` count for nothing in that
        frame); on a renderer without a deformation network that is ``"static"``, fusion in place.  Each (chunk of ``voxel_chunk``
        voxels, block of ``frame_block`` frames) is one cold ``to_observed`` launch over chunk x block rows, then one integrate launch;
        the chunking changes no bit.  ``trunc=None``: 4 x the largest lattice cell side.  The twin's dict with device tensors: tsdf,
        weight [R,R,R], color [R,R,R,3] or None, trunc, bound_min, bound_max, space; nothing is read back."""
        if space not in ("canonical", "static"):
            raise ValueError(f'space must be "canonical" or "static" (got {space!r})')
        space = space if self.use_deform else "static"
        dep = self._fuse_f32(depths, 3, "depths")
        F = int(dep.shape[0])
        col = None if colors is None else self._fuse_f32(colors, 4, "colors")
        msk = None if masks is None else torch.as_tensor(masks).to(self.device)
        tt = f32(torch.as_tensor(times).to(device=self.device, dtype=torch.float32)).reshape(-1)
        R, vc, fb = fusion.check_fuse_args(resolution, voxel_chunk, frame_block, F, tt, col, msk)
        table, shared = flow.camera_table(intrinsics, poses)
        if shared or table.shape[0] != F:
            raise ValueError(f"{F} depth frames take poses [{F}, 4, 4] (got {table.shape[0]} camera(s))")
        trunc, depth_trunc = fusion.check_trunc(fusion.default_trunc(bound_min, bound_max, R) if trunc is None else trunc, depth_trunc)
        cams = self.engine.flow_cameras(table)
        axes = _Lattice(bound_min, bound_max, R, self.device).axes()
        N = R * R * R
        state = self.engine.tsdf_state(N, col is not None)
        with torch.no_grad():
            for n0 in range(0, N, vc):
                pts = fusion.lattice_points(axes, n0, n0 + vc)
                n = int(pts.shape[0])
                part = {k: (None if state[k] is None else state[k][n0:n0 + n]) for k in fusion.STATE_KEYS}
                for f0 in range(0, F, fb):
                    sl = slice(f0, min(f0 + fb, F))
                    nb = sl.stop - sl.start
                    pos, valid = pts, None
                    if space == "canonical":
                        ob = self.to_observed(pts.repeat(nb, 1), tt[sl].repeat_interleave(n), max_iters=max_iters, tol=tol)
                        pos, valid = ob["points"].reshape(nb, n, 3), ob["converged"].reshape(nb, n)
                    self.engine.tsdf_integrate(part, pos, dep[sl], cams[sl], None if col is None else col[sl], None if msk is None else msk[sl],
                                               valid, trunc, depth_trunc)
            out = self.engine.tsdf_finalize(state)
        lo, hi = fusion._bounds64(bound_min, bound_max)
        return {"tsdf": out["tsdf"].view(R, R, R), "weight": out["weight"].view(R, R, R),
                "color": None if out["color"] is None else out["color"].view(R, R, R, 3), "trunc": trunc, "bound_min": lo, "bound_max": hi,
                "space": space}

    @_on_device
    def fused_mesh(self, volume, min_weight=1.0, method="tetrahedra", t=None):
        """``fusion.fused_mesh`` on the device: the zero level set of a fused volume by ``Engine.iso_surface(method)``, the observed part
        only -- a vertex is kept when both grid ends of its edge have weight >= ``min_weight``, a triangle when its three vertices are.
        dict(vertices [V,3] world (``canonical`` too for a canonical volume), triangles [T,3] int32, colors [V,3] or None, weight [V],
        edge_ends [V,2]); with ``t``, ``observed_vertices`` = ``to_observed(vertices, t)`` and its ``converged``."""
        vol = self._fuse_volume(volume)
        tsdf, R = vol["tsdf"], int(vol["tsdf"].shape[0])
        verts, tris, ends = self.engine.iso_surface(tsdf, 0.0, method)
        ends = ends.long()
        wflat, uflat = vol["weight"].reshape(-1), tsdf.reshape(-1)
        mw = float(min_weight)
        keep = (wflat[ends[:, 0]] >= mw) & (wflat[ends[:, 1]] >= mw)
        tl = tris.long()
        tl = tl[keep[tl].all(-1)] if tl.shape[0] else tl
        new = torch.cumsum(keep, 0) - 1
        verts, ends = verts[keep], ends[keep]
        ua, ub = uflat[ends[:, 0]], uflat[ends[:, 1]]
        w = ((0.0 - ua) / (ub - ua))[:, None]
        lerp = lambda a: a[ends[:, 0]] + w * (a[ends[:, 1]] - a[ends[:, 0]])
        world = _Lattice(vol["bound_min"], vol["bound_max"], R, self.device).to_world(verts)
        out = {"vertices": world, "triangles": new[tl].to(torch.int32), "colors": None if vol["color"] is None else lerp(vol["color"].reshape(-1, 3)),
               "weight": lerp(wflat[:, None])[:, 0], "edge_ends": ends.to(torch.int32)}
        if vol.get("space") == "canonical":
            out["canonical"] = world
        if t is not None:
            still = {"points": world, "converged": torch.ones(world.shape[0], dtype=torch.bool, device=self.device)}
            ob = self.to_observed(world, t) if vol.get("space") == "canonical" else still
            out.update(observed_vertices=ob["points"], converged=ob["converged"])
        return out

    @_on_device
    def mesh_coverage(self, mesh_or_track, volume, t=None):
        """Which parts of a mesh were ever observed: dict(coverage [V] = the volume's weight (how many frames saw this piece of tissue
        near the measured depth) sampled trilinearly at the vertices' canonical positions, inside [V] bool = the position lies in the
        volume's lattice; coverage is 0 outside).  ``mesh_or_track``: a dict with ``canonical`` [V,3] (``track_mesh``'s: one coverage
        for every frame of the track; ``fused_mesh``'s) is read there; else a mesh dict's ``vertices`` or [V,3] vertices seen at time
        ``t`` go through ``to_canonical(vertices, t)``.  For a ``"static"`` volume the vertices are used as they are."""
        vol = self._fuse_volume(volume)
        d = mesh_or_track if isinstance(mesh_or_track, dict) else None
        static = vol.get("space") == "static"
        if d is not None and "canonical" in d and not static and t is None:
            pts = self._track_rows(d["canonical"])
        else:
            v = d["vertices"] if d is not None else mesh_or_track
            v = torch.as_tensor(v)
            if v.dim() != 2:
                raise ValueError(f"mesh_coverage takes [V, 3] vertices or a dict with canonical [V, 3] (got vertices {tuple(v.shape)})")
            if static:
                pts = self._track_rows(v)
            elif t is None:
                raise TypeError("mesh_coverage needs t, the time of the given vertices, for a canonical volume")
            else:
                pts = self.to_canonical(v, t)
        cov, inside = self.engine.sample_volume(vol["weight"], pts, vol["bound_min"], vol["bound_max"])
        return {"coverage": cov, "inside": inside}

    @_on_device
    def export_fused_mesh(self, prefix, volume, min_weight=1.0, method="tetrahedra", t=None):
        """``fused_mesh`` written through ``data.write_ply``: ``prefix + "_geometry.ply"`` and, for a volume with colour, ``prefix +
        "_color.ply"`` (the fused colours clipped to [0, 1]); with ``t`` the files hold ``observed_vertices``.  Returns the mesh dict with
        ``paths``."""
        mesh = self.fused_mesh(volume, min_weight, method, t)
        v = mesh["observed_vertices"] if t is not None else mesh["vertices"]
        prefix = str(prefix)
        paths = {"geometry": f"{prefix}_geometry.ply"}
        write_ply(paths["geometry"], v, mesh["triangles"], engine=self.engine)
        if mesh["colors"] is not None:
            paths["color"] = f"{prefix}_color.ply"
            write_ply(paths["color"], v, mesh["triangles"], colors=mesh["colors"].clamp(0.0, 1.0), engine=self.engine)
        mesh["paths"] = paths
        return mesh
