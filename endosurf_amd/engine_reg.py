"""The registration methods of ``engine.Engine`` (a mixin): least-squares rigid motion between corresponding rows, the rigid part of a
surface track, and iterative closest point against the triangles of a mesh, csrc/register.hip; ``registration`` is the specification
and the fp64 twin.  Arguments and results are device tensors under the twin's keys; rotation, translation and rmse are
fp64; nothing but ICP's ``done`` word and its final record is read back."""
from __future__ import annotations

import numpy as np
import torch

from . import registration
from ._device import f32
from ._lib import EndoSurfHipError, check, ptr

_STATE_DOUBLES = 16          # R[9], t[3], step, then int32 status, iterations, done, (pad): es_icp_update's record
_STATE_WORDS = 26            # the first int32 of the record's words


class RegMixin:
    def _reg_pair(self, p, q, w, what):
        """(p [B,N,3], q [B,N,3] fp32 contiguous, w [B,N] / [N] fp32 or None, B, N, whether the call was unbatched)."""
        for name, a in (("p", p), ("q", q)):
            if not torch.is_tensor(a) or a.dim() not in (2, 3) or a.shape[-1] != 3 or a.device != self.device:
                got = f"{tuple(a.shape)} on {a.device}" if torch.is_tensor(a) else type(a).__name__
                raise EndoSurfHipError(f"{what} takes {name} as [N, 3] or [B, N, 3] on {self.device} (got {got})")
        single = p.dim() == 2 and q.dim() == 2
        p, q = (a[None] if a.dim() == 2 else a for a in (p, q))
        B, N = max(int(p.shape[0]), int(q.shape[0])), int(p.shape[1])
        if int(q.shape[1]) != N or int(p.shape[0]) not in (1, B) or int(q.shape[0]) not in (1, B):
            raise EndoSurfHipError(f"{what}: p {tuple(p.shape)} and q {tuple(q.shape)} do not pair up")
        if 3 * B * N >= 1 << 31:
            raise EndoSurfHipError(f"{what}: {B} x {N} rows do not fit int32 indices")
        if w is not None:
            if not torch.is_tensor(w) or w.device != self.device or tuple(w.shape) not in ((N,), (B, N)):
                raise EndoSurfHipError(f"{what} takes w as [N] or [B, N] = {(B, N)} on {self.device}")
            w = f32(w)
        return f32(p.expand(B, N, 3)), f32(q.expand(B, N, 3)), w, B, N, single

    def _rigid_moments(self, p, q, w, B, N):
        out = self.empty(B, registration.MOMENTS, dtype=torch.float64)
        scratch = self._scratch("es_rigid_scratch_bytes", B, N)
        check(self.lib.es_rigid_moments(ptr(p), ptr(q), ptr(w), B, N, int(w is not None and w.dim() == 2), ptr(scratch), ptr(out), self.st()),
              "es_rigid_moments")
        return out

    def rigid_moments(self, p: torch.Tensor, q: torch.Tensor, w=None):
        """``registration.rigid_moments`` on the device: [B,17] fp64 ([17] for [N,3] inputs), two launches, a fixed order of summation:
        the same bits from call to call."""
        p, q, w, B, N, single = self._reg_pair(p, q, w, "rigid_moments")
        out = self._rigid_moments(p, q, w, B, N)
        return out[0] if single else out

    def _rigid_fit(self, p, q, w, B, N):
        st = self.st()
        R, t = self.empty(B, 3, 3, dtype=torch.float64), self.empty(B, 3, dtype=torch.float64)
        W, valid, rmse = self.empty(B, dtype=torch.float64), self.empty(B, dtype=torch.uint8), self.empty(B, dtype=torch.float64)
        check(self.lib.es_rigid_solve(ptr(self._rigid_moments(p, q, w, B, N)), B, ptr(R), ptr(t), ptr(W), ptr(valid), st), "es_rigid_solve")
        moved = self.empty(B, N, 3)
        check(self.lib.es_rigid_apply(ptr(R), ptr(t), ptr(p), B, N, 3 * N, ptr(moved), None, None, None, st), "es_rigid_apply")
        check(self.lib.es_rigid_rmse(ptr(self._rigid_moments(moved, q, w, B, N)), B, ptr(rmse), st), "es_rigid_rmse")
        return {"rotation": R, "translation": t, "rmse": rmse, "weight": W, "valid": valid.bool()}

    def rigid_fit(self, p: torch.Tensor, q: torch.Tensor, w=None):
        """``registration.rigid_fit`` on the device: the proper rotation and the translation that minimise sum w |R p + t - q|^2 per
        batch, dict(rotation [B,3,3], translation [B,3], rmse [B], weight [B] fp64, valid [B] bool), unbatched for [N,3] inputs."""
        p, q, w, B, N, single = self._reg_pair(p, q, w, "rigid_fit")
        out = self._rigid_fit(p, q, w, B, N)
        return {k: v[0] for k, v in out.items()} if single else out

    def rigid_apply(self, rotation: torch.Tensor, translation: torch.Tensor, p: torch.Tensor):
        """``registration.rigid_apply`` on the device: R p + t in fp64, rounded to fp32; [3,3] / [B,3,3] rotations, [N,3] / [B,N,3]
        rows (one [N,3] is shared by all B motions)."""
        if not all(torch.is_tensor(a) and a.device == self.device for a in (rotation, translation, p)):
            raise EndoSurfHipError(f"rigid_apply takes its arguments as tensors on {self.device}")
        single = rotation.dim() == 2 and p.dim() == 2
        if p.dim() not in (2, 3) or p.shape[-1] != 3 or rotation.dim() not in (2, 3) or tuple(rotation.shape[-2:]) != (3, 3) \
                or tuple(translation.shape) != tuple(rotation.shape[:-2]) + (3,):
            raise EndoSurfHipError(f"rigid_apply takes [B, 3, 3], [B, 3] and [N, 3] / [B, N, 3] (got {tuple(rotation.shape)}, "
                                   f"{tuple(translation.shape)}, {tuple(p.shape)})")
        R = rotation.detach().to(torch.float64).reshape(-1, 3, 3).contiguous()
        t = translation.detach().to(torch.float64).reshape(-1, 3).contiguous()
        x = f32(p)
        n_motions, n_sets, N = int(R.shape[0]), int(x.shape[0]) if x.dim() == 3 else 1, int(x.shape[-2])
        B = max(n_motions, n_sets)
        if n_motions not in (1, B) or n_sets not in (1, B):
            raise EndoSurfHipError(f"rigid_apply: {n_motions} motions and {n_sets} sets of rows do not pair up")
        R, t = R.expand(B, 3, 3).contiguous(), t.expand(B, 3).contiguous()
        out = self.empty(B, N, 3)
        check(self.lib.es_rigid_apply(ptr(R), ptr(t), ptr(x), B, N, 0 if n_sets == 1 else 3 * N, ptr(out), None, None, None, self.st()),
              "es_rigid_apply")
        return out[0] if single else out

    def track_rigid(self, vertices: torch.Tensor, reference: int = 0, weights=None):
        """``registration.track_rigid`` on the device for [F,V,3] vertices: dict(rotation [F,3,3], translation [F,3], rmse [F] fp64,
        valid [F] bool, residual [F,V,3], residual_norm [F,V] fp32) with x_f ~ R_f x_ref + t_f.  Seven launches whatever F is."""
        v = vertices
        if not torch.is_tensor(v) or v.dim() != 3 or v.shape[-1] != 3 or v.device != self.device:
            got = f"{tuple(v.shape)} on {v.device}" if torch.is_tensor(v) else type(v).__name__
            raise EndoSurfHipError(f"track_rigid takes [F, V, 3] vertices on {self.device} (got {got})")
        v = f32(v)
        F, V = int(v.shape[0]), int(v.shape[1])
        if not -F <= int(reference) < F:
            raise EndoSurfHipError(f"track_rigid: reference frame {reference} of {F}")
        if weights is not None and (not torch.is_tensor(weights) or weights.device != self.device or tuple(weights.shape) != (V,)):
            raise EndoSurfHipError(f"track_rigid takes weights as [V] = [{V}] on {self.device}")
        ref = v[int(reference) % F].contiguous()
        p, q, w, B, N, _ = self._reg_pair(ref[None], v, weights, "track_rigid")
        fit = self._rigid_fit(p, q, w, B, N)
        residual, norm = self.empty(F, V, 3), self.empty(F, V)
        check(self.lib.es_rigid_apply(ptr(fit["rotation"]), ptr(fit["translation"]), ptr(ref), F, V, 0, None, ptr(v), ptr(residual), ptr(norm),
                                      self.st()), "es_rigid_apply")
        return {"rotation": fit["rotation"], "translation": fit["translation"], "rmse": fit["rmse"], "valid": fit["valid"],
                "residual": residual, "residual_norm": norm}

    def _icp_weights(self, tri, dist, max_distance):
        """``registration.icp_weights`` (a handful of elementwise launches on N rows; the sums are the library's)."""
        w = tri >= 0
        if max_distance is not None:
            w = w & (dist.double() <= float(max_distance))
        return w.to(torch.float32)

    def icp(self, points: torch.Tensor, vertices: torch.Tensor, triangles: torch.Tensor, method: str = "plane", max_iters: int = 50,
            tol: float = 1e-6, max_distance=None, init=None, poll: int = 4):
        """``registration.icp`` on the device: the rigid motion that lays ``points`` [N,3] onto the mesh ``vertices`` [V,3] /
        ``triangles`` [T,3], all on this device.  The triangle grid is built once (es_surf_build); an iteration is four launches
        (es_rigid_apply, es_surf_query, the accumulation, es_icp_update) and the transform never leaves the device: the host reads the
        record's ``done`` word every ``poll`` iterations and stops there, at ``max_iters`` at the latest.  Once done is set the update
        kernel changes nothing, so the result is the same bits for any ``poll`` and from call to call.  ``init`` = (R, t), tensors
        anywhere or arrays.  Returns the twin's dict: rotation [3,3], translation [3] (fp64, device), iterations (the device's own
        count), status, step, rmse, inliers (Python numbers, read once at the end), points [N,3], distance [N], triangle [N]."""
        if method not in registration.METHODS:
            raise EndoSurfHipError(f"icp: method must be 'point' or 'plane' (got {method!r})")
        poll, max_iters = int(poll), int(max_iters)
        if poll < 1 or max_iters < 0:
            raise EndoSurfHipError(f"icp: poll must be at least 1 and max_iters at least 0 (got {poll}, {max_iters})")
        if max_distance is not None and not float(max_distance) >= 0.0:
            raise EndoSurfHipError(f"icp: max_distance must be >= 0 or None (got {max_distance!r})")
        if not torch.is_tensor(points) or not torch.is_tensor(vertices):
            raise EndoSurfHipError(f"icp takes its points and vertices as tensors on {self.device}")
        p = self._rows3_arg(points, "icp", "[N, 3] points")
        v = self._rows3_arg(vertices, "icp", "[V, 3] vertices")
        N, V, t = int(p.shape[0]), int(v.shape[0]), triangles
        if torch.is_tensor(t) and t.dtype == torch.int64:          # an index beyond int32 must stay out of range, not wrap into it
            t = torch.where((t < 0) | (t >= V), torch.full_like(t, -1), t)
        t32 = self._tri_arg(t, "icp")
        T = int(t32.shape[0])
        R0, t0 = (np.eye(3), np.zeros(3)) if init is None else (np.asarray(torch.as_tensor(a).detach().cpu(), np.float64) for a in init)
        if R0.shape != (3, 3) or t0.shape != (3,):
            raise EndoSurfHipError(f"icp: init is (R [3, 3], t [3]) (got {R0.shape}, {t0.shape})")
        host = np.zeros(_STATE_DOUBLES)
        host[:9], host[9:12], host[12] = R0.reshape(9), t0, np.inf
        host.view(np.int32)[_STATE_WORDS:_STATE_WORDS + 3] = (registration.MAX_ITERS, 0, 0)
        state = torch.from_numpy(host).to(self.device)
        words = state.view(torch.int32)
        st, lib, code = self.st(), self.lib, registration.METHODS[method]
        md = -1.0 if max_distance is None else float(max_distance)
        grid = self._scratch("es_surf_scratch_bytes", V, T)
        scratch = self._scratch("es_rigid_scratch_bytes", 1, N)
        x, dist, tri, closest = self.empty(N, 3), self.empty(N), self.empty(N, dtype=torch.int32), self.empty(N, 3)
        sums = self.empty(registration.NORMAL_SUMS, dtype=torch.float64)
        check(lib.es_surf_build(ptr(v), ptr(t32), V, T, ptr(grid), st), "es_surf_build")

        def closest_triangles():
            check(lib.es_rigid_apply(ptr(state), ptr(state[9:]), ptr(p), 1, N, 3 * N, ptr(x), None, None, None, st), "es_rigid_apply")
            check(lib.es_surf_query(ptr(x), N, ptr(v), ptr(t32), V, T, ptr(grid), ptr(dist), ptr(tri), ptr(closest), None, st), "es_surf_query")

        issued = 0
        while issued < max_iters:
            n = min(poll, max_iters - issued)
            for _ in range(n):
                closest_triangles()
                if code == registration.METHODS["plane"]:
                    check(lib.es_icp_normal_equations(ptr(x), ptr(closest), ptr(tri), ptr(dist), ptr(v), ptr(t32), V, T, N, md, ptr(scratch),
                                                      ptr(sums), st), "es_icp_normal_equations")
                else:
                    w = self._icp_weights(tri, dist, max_distance)
                    check(lib.es_rigid_moments(ptr(x), ptr(closest), ptr(w), 1, N, 0, ptr(scratch), ptr(sums), st), "es_rigid_moments")
                check(lib.es_icp_update(ptr(sums), code, float(tol), ptr(state), st), "es_icp_update")
            issued += n
            if int(words[_STATE_WORDS + 2].item()):
                break
        closest_triangles()
        w = self._icp_weights(tri, dist, max_distance)
        moments = self.empty(1, registration.MOMENTS, dtype=torch.float64)
        check(lib.es_rigid_moments(ptr(x), ptr(closest), ptr(w), 1, N, 0, ptr(scratch), ptr(moments), st), "es_rigid_moments")
        rmse = self.empty(1, dtype=torch.float64)
        check(lib.es_rigid_rmse(ptr(moments), 1, ptr(rmse), st), "es_rigid_rmse")
        final = torch.cat([state, moments[0, :1], rmse]).cpu().numpy()          # the one read-back of the record
        status, iterations = (int(k) for k in final[:_STATE_DOUBLES].view(np.int32)[_STATE_WORDS:_STATE_WORDS + 2])
        return {"rotation": state[:9].reshape(3, 3).clone(), "translation": state[9:12].clone(), "iterations": iterations, "status": status,
                "step": float(final[12]), "rmse": float(final[17]), "inliers": int(final[16]), "points": x, "distance": dist, "triangle": tri}
