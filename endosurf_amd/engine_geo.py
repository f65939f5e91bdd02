"""The geodesic method of ``engine.Engine`` (a mixin): distance fields along a triangle mesh by Jacobi sweeps of a first-order eikonal
update, csrc/geodesic.hip; ``geodesic.mesh_geodesic`` is the specification and the fp64 twin."""
from __future__ import annotations

import torch

from ._device import f32
from ._lib import EndoSurfHipError, check, ptr


def _dot(a, b):          # (x0 y0 + x1 y1) + x2 y2, every operation a launch of its own: rounded where the twin rounds
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


class GeoMixin:
    def _geodesic_project(self, points, v, t32):
        """``geodesic.project`` and ``geodesic.carry`` on the device: ``points`` [N,3] projected onto frame ``v[ref]`` given as ``v[0]``
        of the pair (reference vertices [V,3] fp32, all frames [F,V,3] fp32) -> (triangle [N] int32, -1 for none; corners [N,3] int64
        of that triangle, -1 for none; the carried points [F,N,3] fp64, NaN for none).  The projection is ``point_to_mesh``'s launch;
        the weights and the carried points are a few elementwise fp64 operations on N rows."""
        v_ref, v_all = v
        N, F = int(points.shape[0]), int(v_all.shape[0])
        if N == 0 or t32.shape[0] == 0 or v_ref.shape[0] == 0:
            return (torch.full((N,), -1, device=self.device, dtype=torch.int32), torch.full((N, 3), -1, device=self.device, dtype=torch.int64),
                    torch.full((F, N, 3), float("nan"), device=self.device, dtype=torch.float64))
        _, tri, closest = self.point_to_mesh(points, v_ref, t32)
        hit = tri >= 0
        corners = torch.where(hit[:, None], t32[tri.clamp(min=0).long()].long(), torch.zeros_like(hit[:, None], dtype=torch.int64))
        vd = v_ref.double()
        v0, v1, v2 = vd[corners[:, 0]], vd[corners[:, 1]], vd[corners[:, 2]]
        e1, e2, d = v1 - v0, v2 - v0, closest.double() - v0
        d11, d12, d22, b1, b2 = _dot(e1, e1), _dot(e1, e2), _dot(e2, e2), _dot(d, e1), _dot(d, e2)
        den = d11 * d22 - d12 * d12
        flat = ~(den > 0.0)
        zero = torch.zeros_like(den)
        w1 = torch.where(flat, zero, (d22 * b1 - d12 * b2) / den)
        w2 = torch.where(flat, zero, (d11 * b2 - d12 * b1) / den)
        w0 = (1.0 - w1) - w2
        va = v_all.double()
        carried = (w0[None, :, None] * va[:, corners[:, 0]] + w1[None, :, None] * va[:, corners[:, 1]]) + w2[None, :, None] * va[:, corners[:, 2]]
        carried = torch.where(hit[None, :, None], carried, torch.full_like(carried, float("nan")))
        return tri, torch.where(hit[:, None], corners, torch.full_like(corners, -1)), carried

    def geodesic(self, vertices: torch.Tensor, triangles: torch.Tensor, sources: torch.Tensor, targets=None, reference: int = 0,
                 poll: int = 8, max_sweeps=None):
        """``geodesic.mesh_geodesic`` (the specification and the fp64 twin) on the device, csrc/geodesic.hip: ``vertices`` [V,3] or
        [F,V,3], ``triangles`` [T,3] int32 / int64, ``sources`` an integer [S] tensor of vertex ids or a float [S,3] tensor of points,
        ``targets`` [Q,3] or None, all on this device -> dict(distance [F,S,V] fp32 ([S,V] for a single mesh, +inf = not reachable),
        sweeps and, with targets, target_distance [F,S,Q] ([S,Q])).  All F S fields advance in one launch per sweep; the host reads one
        word back every ``poll`` sweeps and stops at the first that says the last sweep changed nothing, so ``sweeps`` is the twin's
        count rounded up to a multiple of ``poll``.  Sweeps past the fixed point change nothing: the result is the same bits for any
        ``poll`` and from call to call, and the twin's values to one fp32 ulp.  More than ``max_sweeps`` (default V + poll; V always
        suffice) raises.  Source and target points are projected with ``point_to_mesh`` on frame ``reference``."""
        v = vertices
        if not torch.is_tensor(v) or v.dim() not in (2, 3) or v.shape[-1] != 3 or v.device != self.device:
            got = f"{tuple(v.shape)} on {v.device}" if torch.is_tensor(v) else type(v).__name__
            raise EndoSurfHipError(f"geodesic takes [V, 3] or [F, V, 3] vertices on {self.device} (got {got})")
        single = v.dim() == 2
        v = f32(v[None] if single else v)
        F, V = int(v.shape[0]), int(v.shape[1])
        if not -F <= int(reference) < F:
            raise EndoSurfHipError(f"geodesic: reference frame {reference} of {F}")
        poll = int(poll)
        if poll < 1:
            raise EndoSurfHipError(f"geodesic: poll must be at least 1 (got {poll})")
        t = triangles
        if torch.is_tensor(t) and t.dtype == torch.int64:          # an index beyond int32 must stay out of range, not wrap into it
            t = torch.where((t < 0) | (t >= V), torch.full_like(t, -1), t)
        t32 = self._tri_arg(t, "geodesic")
        T = int(t32.shape[0])
        if V >= 1 << 31 or T >= 1 << 31:
            raise EndoSurfHipError(f"geodesic: {V} vertices / {T} triangles do not fit int32 indices")
        src = sources
        if not torch.is_tensor(src) or src.device != self.device:
            raise EndoSurfHipError(f"geodesic takes its sources as a tensor on {self.device}")
        by_id = not src.is_floating_point()
        if (by_id and src.dim() != 1) or (not by_id and (src.dim() != 2 or src.shape[1] != 3)) or src.shape[0] < 1:
            raise EndoSurfHipError(f"geodesic takes an integer [S] tensor of vertex ids or a float [S, 3] tensor of points, S >= 1 "
                                   f"(got {src.dtype} {tuple(src.shape)})")
        S = int(src.shape[0])
        B = F * S
        frames = (v[int(reference) % F], v)
        st = self.st()
        # ---- seeds: (field, vertex, value) triples ---------------------------------------------------------------------------------
        field = torch.arange(B, device=self.device, dtype=torch.int32)
        if by_id:
            ids = src.long()
            ids = torch.where((ids < 0) | (ids >= V), torch.full_like(ids, -1), ids).to(torch.int32)
            seed_field, seed_vertex = field, ids.repeat(F).contiguous()
            seed_value = torch.zeros(B, device=self.device, dtype=torch.float64)
            s_tri = s_pts = None
        else:
            s_tri, corners, s_pts = self._geodesic_project(self._rows3_arg(src, "geodesic", "[S, 3] sources"), frames, t32)
            s_pts = s_pts.contiguous()
            d = v.double()[:, corners.clamp(min=0)] - s_pts[:, :, None, :]                  # [F,S,3 corners,3]
            seed_value = torch.sqrt(_dot(d, d)).contiguous()                                # NaN where there is no triangle
            seed_field = field.reshape(F, S, 1).expand(F, S, 3).contiguous()
            seed_vertex = corners.to(torch.int32)[None].expand(F, S, 3).contiguous()
        cur, nxt = self.empty(B, V, dtype=torch.int64), self.empty(B, V, dtype=torch.int64)
        check(self.lib.es_geodesic_seed(ptr(v), ptr(t32), F, V, T, S, ptr(seed_field), ptr(seed_vertex), ptr(seed_value), seed_field.numel(),
                                        ptr(cur), ptr(nxt), st), "es_geodesic_seed")
        # ---- sweeps: one launch each, one word read back per ``poll`` -----------------------------------------------------------------
        changed = self.empty(1, dtype=torch.int32)
        cap = V + poll if max_sweeps is None else int(max_sweeps)
        sweeps = 0
        while True:
            n = max(1, min(poll, cap - sweeps))
            for i in range(n):
                check(self.lib.es_geodesic_sweep(ptr(v), ptr(t32), F, V, T, S, ptr(cur), ptr(nxt), ptr(changed) if i == n - 1 else None, st),
                      "es_geodesic_sweep")
                cur, nxt = nxt, cur
            sweeps += n
            if not int(changed.item()):
                break
            if sweeps >= cap:
                raise EndoSurfHipError(f"geodesic did not reach its fixed point in {sweeps} sweeps ({V} vertices)")
        distance = self.empty(F, S, V)
        check(self.lib.es_geodesic_finish(ptr(cur), B * V, ptr(distance), st), "es_geodesic_finish")
        out = {"distance": distance[0] if single else distance, "sweeps": sweeps}
        if targets is not None:
            if not torch.is_tensor(targets) or targets.device != self.device:
                raise EndoSurfHipError(f"geodesic takes its targets as a tensor on {self.device}")
            q_tri, _, q_pts = self._geodesic_project(self._rows3_arg(targets, "geodesic", "[Q, 3] targets"), frames, t32)
            Q = int(q_tri.shape[0])
            td = self.empty(F, S, Q)
            check(self.lib.es_geodesic_read(ptr(cur), ptr(v), ptr(t32), F, V, T, S, ptr(q_tri), ptr(q_pts.contiguous()), Q, ptr(s_tri),
                                            ptr(s_pts), ptr(td), st), "es_geodesic_read")
            out["target_distance"] = td[0] if single else td
        return out
