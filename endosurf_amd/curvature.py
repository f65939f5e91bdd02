"""Surface curvature: the second derivative of the field  sdf(x + D(x, t))  on its level sets.

``strain`` says what the tissue does along a track; this module says what the surface looks like there: a ridge or a flat patch, a fold
or a bulge, one scalar per vertex to paint on the tracked mesh.  With g and H the gradient and the Hessian of the field at a point,
n = g / |g| the normal (towards increasing SDF, out of the tissue), T = [t1 t2] an orthonormal basis of the plane normal to n and

    S = T^T H T / |g| = [[a, b], [b, c]]          (the shape operator of the level set through the point),

the mean curvature is (a + c) / 2, the Gauss curvature a c - b^2 and the principal curvatures mean +- hypot((a - c) / 2, b).  Sign: a
sphere |x| - R seen from outside has both curvatures +1/R.  The results do not depend on T beyond rounding; T is built as
``strain.strain_rows`` builds it: t1 = n x e normalised for the axis e the normal is furthest from, t2 = n x t1.

In observed space the field is the SDF network at x_c = x + D(x, t).  The SDF network is smooth (softplus), the deformation network is
piecewise linear in its encodings, so away from the ReLU kinks, with g_c, H_c the canonical gradient and Hessian at x_c, J the Jacobian
of the deformation and CURV(g_c) the curvature of its encodings against g_c (``ES_WS_CURV``, include/endosurf_hip.h):

    g_o = J^T g_c,        H_o = J^T H_c J - diag(CURV(g_c))          (``compose_hessian``).

Plain torch / numpy, computed in fp64 whatever the inputs are; results come back in the dtype and on the device of the inputs.
``hessian_fn(x, t) -> (sdf [M,1], gradient [M,3], hessian [M,3,3])`` is any callable on [M,3] points and [M] times, e.g. autograd through
the fp64 oracle.  ``compose_hessian`` and ``curvature_rows`` are the written specification and the fp64 twin of the device kernel
(csrc/curvature.hip); the functions that compose them take ``rows_fn=``, a callable ``(gradient, hessian) -> dict`` that
replaces ``curvature_rows``, and the renderer's methods of the same names (``renderer_curv``) pass the kernel there with the model's own
Hessian (csrc/sdf_hess.hip) as ``hessian_fn``.

Validity: a row is valid exactly when |g| is positive and finite and every entry of H is finite.  The tests are written
as "not > 0", so a NaN anywhere makes the row invalid.  A row that is not valid has zeros in mean, gauss and principal.
"""
from __future__ import annotations

import numpy as np
import torch

from .tracking import _times


def _rows(a, width, M=None, what="rows"):
    a = np.ascontiguousarray(torch.as_tensor(a).detach().cpu().numpy(), dtype=np.float64).reshape(-1, *width)
    if M is not None and a.shape[0] != M:
        raise ValueError(f"{what} must have one row per gradient (got {a.shape[0]} for {M})")
    return a


def _like(v, like):
    dtype = like.dtype if like.dtype.is_floating_point else torch.float64
    return torch.from_numpy(np.ascontiguousarray(v)).to(device=like.device, dtype=dtype)


def compose_hessian(grad_c, hess_c, jac=None, dd=None):
    """(grad_o [M,3], hess_o [M,3,3]) = (J^T g_c, J^T H_c J - diag(dd)) per row: ``grad_c`` [M,3] and ``hess_c`` [M,3,3] of the SDF
    network at the canonical points, ``jac`` [M,3,3] the Jacobian of the deformation (dim_out, dim_in; None: the identity) and ``dd``
    [M,3] = CURV(g_c) (None: zero).  fp64 arithmetic, the dtype and device of ``grad_c``."""
    like = torch.as_tensor(grad_c)
    g = _rows(like, (3,))
    M = g.shape[0]
    H = _rows(hess_c, (3, 3), M, "hess_c")
    J = np.broadcast_to(np.eye(3), (M, 3, 3)) if jac is None else _rows(jac, (3, 3), M, "jac")
    d = np.zeros((M, 3)) if dd is None else _rows(dd, (3,), M, "dd")
    with np.errstate(all="ignore"):
        go = np.stack([J[:, 0, j] * g[:, 0] + J[:, 1, j] * g[:, 1] + J[:, 2, j] * g[:, 2] for j in range(3)], -1)
        HJ = [[H[:, i, 0] * J[:, 0, j] + H[:, i, 1] * J[:, 1, j] + H[:, i, 2] * J[:, 2, j] for j in range(3)] for i in range(3)]
        Ho = np.stack([np.stack([J[:, 0, i] * HJ[0][j] + J[:, 1, i] * HJ[1][j] + J[:, 2, i] * HJ[2][j] - (d[:, i] if i == j else 0.0)
                                 for j in range(3)], -1) for i in range(3)], -2)
    return _like(go, like), _like(Ho.reshape(M, 3, 3), like)


def curvature_rows(gradient, hessian):
    """The per-row algebra of the module's formulas: ``gradient`` [M,3] and ``hessian`` [M,3,3] of a field -> dict(mean [M], gauss [M],
    principal [M,2] descending, valid [M] bool).  fp64 arithmetic, the dtype and device of ``gradient``."""
    like = torch.as_tensor(gradient)
    g = _rows(like, (3,))
    M = g.shape[0]
    H = _rows(hessian, (3, 3), M, "hessian")
    big = np.finfo(np.float64).max
    with np.errstate(all="ignore"):
        length = np.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1] + g[:, 2] * g[:, 2])
        valid = (length > 0.0) & (length <= big) & (np.abs(H).reshape(M, 9) <= big).all(-1)          # (false for NaN)
        # the rows that are not valid run through the algebra as a unit gradient and a zero Hessian and are zeroed at the end
        g = np.where(valid[:, None], g, np.array([0.0, 0.0, 1.0]))
        H = np.where(valid[:, None, None], H, 0.0)
        length = np.where(valid, length, 1.0)
        n = g / length[:, None]
        e = np.eye(3)[np.argmin(np.abs(n), axis=1)] if M else np.zeros((0, 3))
        t1 = np.cross(n, e)
        t1 = t1 / np.sqrt(t1[:, 0] * t1[:, 0] + t1[:, 1] * t1[:, 1] + t1[:, 2] * t1[:, 2])[:, None]
        t2 = np.cross(n, t1)
        h1 = np.stack([H[:, i, 0] * t1[:, 0] + H[:, i, 1] * t1[:, 1] + H[:, i, 2] * t1[:, 2] for i in range(3)], -1)
        h2 = np.stack([H[:, i, 0] * t2[:, 0] + H[:, i, 1] * t2[:, 1] + H[:, i, 2] * t2[:, 2] for i in range(3)], -1)
        dot = lambda u, v: u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1] + u[:, 2] * v[:, 2]
        a, b, c = dot(t1, h1) / length, dot(t1, h2) / length, dot(t2, h2) / length
        mean = 0.5 * (a + c)
        rad = np.hypot(0.5 * (a - c), b)
        out = {"mean": mean, "gauss": a * c - b * b, "principal": np.stack([mean + rad, mean - rad], -1)}
    res = {k: _like(np.where(valid.reshape((M,) + (1,) * (v.ndim - 1)), v, 0.0), like) for k, v in out.items()}
    res["valid"] = torch.from_numpy(valid).to(like.device)
    return res


def surface_curvature(hessian_fn, points, t, rows_fn=None):
    """The curvature of the level set of the field through each of ``points`` [M,3] at ``t`` (scalar or [M]): dict(sdf [M,1], gradient
    [M,3], hessian [M,3,3]) as ``hessian_fn`` gives them, plus ``curvature_rows``' mean, gauss, principal and valid."""
    points = torch.as_tensor(points)
    sdf, gradient, hessian = hessian_fn(points, _times(t, points.shape[0], points))
    return {"sdf": sdf, "gradient": gradient, "hessian": hessian, **(rows_fn or curvature_rows)(gradient, hessian)}


def mesh_curvature(hessian_fn, mesh_or_track, times, rows_fn=None):
    """The curvature maps of a mesh: mean, gauss, principal, valid per vertex.  ``mesh_or_track``: [V,3] vertices or a mesh dict (its
    ``vertices``) seen at the one time ``times`` -> [V] maps; or the dict of ``tracking.track_mesh`` over ``times`` [F] -> [F,V] maps,
    evaluated once on all F*V rows with a time per row, where ``valid`` also requires ``track["converged"]`` and a row that is not valid
    is zero as everywhere."""
    if isinstance(mesh_or_track, dict) and "converged" in mesh_or_track:
        verts = torch.as_tensor(mesh_or_track["vertices"])
        F, V = int(verts.shape[0]), int(verts.shape[1])
        times = torch.as_tensor(times, dtype=verts.dtype, device=verts.device).reshape(-1)
        if times.numel() != F:
            raise ValueError(f"times must hold one time per tracked frame (got {times.numel()} for {F})")
        conv = torch.as_tensor(mesh_or_track["converged"]).to(verts.device).reshape(F, V)
        rows = surface_curvature(hessian_fn, verts.reshape(F * V, 3), times.repeat_interleave(V), rows_fn)
        valid = rows["valid"].reshape(F, V) & conv
        out = {}
        for k in ("mean", "gauss", "principal"):
            v = rows[k].reshape(F, V, *rows[k].shape[1:])
            out[k] = torch.where(valid.reshape(F, V, *([1] * (v.dim() - 2))), v, torch.zeros_like(v))
        out["valid"] = valid
        return out
    verts = torch.as_tensor(mesh_or_track["vertices"] if isinstance(mesh_or_track, dict) else mesh_or_track).reshape(-1, 3)
    rows = surface_curvature(hessian_fn, verts, times, rows_fn)
    return {k: rows[k] for k in ("mean", "gauss", "principal", "valid")}
