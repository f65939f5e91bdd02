"""Tissue velocity and strain rate along surface tracks: how the tissue moves *at* a time.

``tracking`` says where a piece of tissue is, ``strain`` how it is stretched relative to another frame; this module gives the rates.
A material point keeps its canonical position: y(t) + D(y(t), t) = c.  Differentiating in time, with J = I + dD/dx and D_t = dD/dt at
(y, t),

    v = dy/dt = -J^-1 D_t,

and differentiating v over y (J^-1 depends on y through the second derivatives of D) gives the velocity gradient

    L_ik = dv_i/dy_k = -(J^-1)_il [ sum_j D_l,jk v_j + D_l,kt ],        dF/dt = L F  along a track.

From L: d = sym L, the strain-rate tensor, and its eigenvalues, the principal rates; tr L = d/dt ln(volume); the axial vector of
L - L^T, the vorticity (curl v); and with the unit normal n of the surface in the *current* configuration, tr d - n.d.n = d/dt ln(area)
of the surface element and the two eigenvalues of d restricted to the plane normal to n, whose sum it is.

The model's D is a ReLU MLP over an encoding that is separable by coordinate: inside a linear region D = A enc(x, t) + b, so every
*mixed* second derivative -- D_i,jk with j != k and D_i,kt -- vanishes identically, and the diagonal form dd[m,i,k] = d2 D_i / d x_k^2 with
``d_xt = None`` is the whole of it: L_ik = -(J^-1)_il dd_lk v_k.  The general form is kept so that the twin is right for any smooth D.
Everything is exact away from the network's ReLU kinks, where D is not differentiable.

Plain torch / numpy; results come back in the dtype and on the device of the inputs.  ``derivs_fn(x, t) -> dict(jac [M,3,3], d_t [M,3],
dd [M,3,3] or [M,3,3,3][, d_xt [M,3,3]])`` is any callable on [M,3] points and [M] times, e.g. autograd through the fp64 oracle.
``kinematics_rows`` is the written specification and the fp64 twin of the device kernel (csrc/kinematics.hip): the
functions that compose it take ``rows_fn=``, a callable ``(jac, d_t, dd, normals) -> dict`` that replaces it, and the renderer's methods
of the same names (``renderer_kin``) pass the kernel there with the model's own derivatives (csrc/deform_jet.hip) as ``derivs_fn``.

Validity (the rule of ``strain``): a row is valid exactly when det J > 0 -- the map preserves orientation there, the
condition under which it is locally invertible and v means anything --, every entry of its inputs is finite and, where normals are
given, its normal has a finite positive length.  The tests are written as "not > 0", so a NaN anywhere makes the row invalid.  A row
that is not valid has zeros in every other output, finite, like an unconverged row of a track.
"""
from __future__ import annotations

import numpy as np
import torch

from .strain import _cof3, _det3
from .tracking import _times


def _np64(a, shape, what, M=None):
    a = np.ascontiguousarray(torch.as_tensor(a).detach().cpu().numpy(), dtype=np.float64).reshape((-1,) + shape)
    if M is not None and a.shape[0] != M:
        raise ValueError(f"{what} must have one row per Jacobian (got {a.shape[0]} for {M})")
    return a


def kinematics_rows(jac, d_t, dd, normals=None, d_xt=None):
    """The per-row algebra.  ``jac`` [M,3,3]: J;  ``d_t`` [M,3]: dD/dt;  ``dd``: [M,3,3], the diagonal form dd[m,i,k] = d2 D_i / d x_k^2
    (every mixed second derivative zero), or [M,3,3,3], the full d2 D_i / d x_j d x_k;  ``d_xt`` [M,3,3]: d2 D_i / d x_k dt (None: zero, the
    network's case);  ``normals`` [M,3]: the surface normal in the current configuration, any finite positive length.  Returns a dict of
      velocity [M,3] = -J^-1 D_t (the inverse by adjugate and determinant);  speed [M];  L [M,3,3], the velocity gradient;
      rate [M,3,3] = (L + L^T) / 2;  principal_rates [M,3], the eigenvalues of rate, descending;  divergence [M] = tr L;
      vorticity [M,3] = (L_21 - L_12, L_02 - L_20, L_10 - L_01);  valid [M] bool (the module's rule);
    and with normals  area_rate [M] = tr d - n.d.n;  surface_rates [M,2]: the eigenvalues of T^T d T, T an orthonormal basis of the
    plane normal to n, descending.  Computed in fp64 (``numpy.linalg.eigvalsh``) whatever the inputs are, returned in their dtype, on
    their device."""
    like = torch.as_tensor(jac)
    J = _np64(like, (3, 3), "jac")
    M = J.shape[0]
    Dt = _np64(d_t, (3,), "d_t", M)
    dd_t = torch.as_tensor(dd)
    full = dd_t.dim() == 4
    H = _np64(dd_t, (3, 3, 3) if full else (3, 3), "dd", M)
    Xt = None if d_xt is None else _np64(d_xt, (3, 3), "d_xt", M)
    eye = np.broadcast_to(np.eye(3), (M, 3, 3))
    big = np.finfo(np.float64).max
    with np.errstate(all="ignore"):
        det = _det3(J)
        valid = det > 0.0          # (false for NaN)
        for a in (J, Dt, H) + (() if Xt is None else (Xt,)):
            valid &= (np.abs(a) <= big).all(axis=tuple(range(1, a.ndim)))          # finite (false for NaN)
        n = None
        if normals is not None:
            n = _np64(normals, (3,), "normals", M)
            length = np.sqrt((n * n).sum(-1))
            n_ok = (length > 0.0) & (length <= big)          # (false for NaN)
            valid &= n_ok
            n = np.where(valid[:, None], n / np.where(n_ok, length, 1.0)[:, None], np.array([0.0, 0.0, 1.0]))
        # the rows that are not valid run through the algebra as the identity at rest and are zeroed at the end
        J = np.where(valid[:, None, None], J, eye)
        Dt = np.where(valid[:, None], Dt, 0.0)
        H = np.where(valid.reshape((M,) + (1,) * (H.ndim - 1)), H, 0.0)
        Jinv = np.swapaxes(_cof3(J), 1, 2) / np.where(valid, det, 1.0)[:, None, None]
        v = -np.matmul(Jinv, Dt[:, :, None])[:, :, 0]
        B = np.einsum("mljk,mj->mlk", H, v) if full else H * v[:, None, :]          # sum_j D_l,jk v_j
        if Xt is not None:
            B = B + np.where(valid[:, None, None], Xt, 0.0)
        L = -np.matmul(Jinv, B)
        d = 0.5 * (L + np.swapaxes(L, 1, 2))
        out = {"velocity": v, "speed": np.sqrt((v * v).sum(-1)), "L": L, "rate": d,
               "principal_rates": np.linalg.eigvalsh(d)[:, ::-1] if M else np.zeros((0, 3)),
               "divergence": L[:, 0, 0] + L[:, 1, 1] + L[:, 2, 2],
               "vorticity": np.stack([L[:, 2, 1] - L[:, 1, 2], L[:, 0, 2] - L[:, 2, 0], L[:, 1, 0] - L[:, 0, 1]], -1)}
        if n is not None:
            out["area_rate"] = (d[:, 0, 0] + d[:, 1, 1] + d[:, 2, 2]) - np.einsum("mi,mij,mj->m", n, d, n)
            # T: n x e for the axis e the normal is furthest from, normalised, and n x that (as ``strain.strain_rows`` builds it)
            e = np.eye(3)[np.argmin(np.abs(n), axis=1)] if M else np.zeros((0, 3))
            t1 = np.cross(n, e)
            t1 /= np.sqrt((t1 * t1).sum(-1))[:, None]
            T = np.stack([t1, np.cross(n, t1)], axis=-1)
            S = np.matmul(np.swapaxes(T, 1, 2), np.matmul(d, T))
            out["surface_rates"] = np.linalg.eigvalsh(0.5 * (S + np.swapaxes(S, 1, 2)))[:, ::-1] if M else np.zeros((0, 2))
    dtype = like.dtype if like.dtype.is_floating_point else torch.float64
    res = {}
    for k, a in out.items():
        a = np.where(valid.reshape((M,) + (1,) * (a.ndim - 1)), a, 0.0)
        res[k] = torch.from_numpy(np.ascontiguousarray(a)).to(device=like.device, dtype=dtype)
    res["valid"] = torch.from_numpy(valid).to(like.device)
    return res


def _rows(derivs_fn, points, t, normals, rows_fn):
    dv = derivs_fn(points, t)
    if rows_fn is not None:
        return rows_fn(dv["jac"], dv["d_t"], dv["dd"], normals)
    return kinematics_rows(dv["jac"], dv["d_t"], dv["dd"], normals, dv.get("d_xt"))


def point_kinematics(derivs_fn, points, t, normals=None, rows_fn=None):
    """Velocity and strain rate of the tissue seen at ``points`` [M,3] at ``t`` (scalar or [M] times); ``normals`` [M,3] of the surface
    there.  ``kinematics_rows``' dict."""
    points = torch.as_tensor(points)
    return _rows(derivs_fn, points, _times(t, points.shape[0], points), normals, rows_fn)


def mesh_kinematics(derivs_fn, track, times, normals=None, normals_fn=None, rows_fn=None):
    """The velocity and strain-rate maps of a tracked mesh, the dict of ``tracking.track_mesh`` over ``times`` [F]: every output of
    ``kinematics_rows`` as [F,V,...], each frame at its own time.  ``valid`` also requires ``track["converged"]``, and a row that is not
    valid is zero as everywhere.  ``normals`` [F,V,3] at each frame's vertices; None: ``normals_fn(vertices, triangles)`` (default
    ``meshing.vertex_normals``) of *each frame's* vertices and ``track["triangles"]``.  The derivatives are evaluated once, on all F*V
    rows with a time per row."""
    verts = torch.as_tensor(track["vertices"])
    F, V = int(verts.shape[0]), int(verts.shape[1])
    times = torch.as_tensor(times, dtype=verts.dtype, device=verts.device).reshape(-1)
    if times.numel() != F:
        raise ValueError(f"times must hold one time per tracked frame (got {times.numel()} for {F})")
    conv = torch.as_tensor(track["converged"]).to(verts.device).reshape(F, V)
    if normals is None:
        if normals_fn is None:
            from .meshing import vertex_normals
            normals_fn = lambda v, f: torch.from_numpy(vertex_normals(torch.as_tensor(v).detach().cpu().numpy(),
                                                                      torch.as_tensor(f).detach().cpu().numpy()))
        normals = torch.stack([torch.as_tensor(normals_fn(verts[f], track["triangles"])).to(verts.device) for f in range(F)]) if F else \
            verts.new_zeros(0, V, 3)
    normals = torch.as_tensor(normals).to(device=verts.device)
    if normals.numel() != F * V * 3:
        raise ValueError(f"normals must be [F, V, 3], one per vertex of each frame (got {tuple(normals.shape)} for F = {F}, V = {V})")
    rows = _rows(derivs_fn, verts.reshape(F * V, 3), times.repeat_interleave(V), normals.reshape(F * V, 3), rows_fn)
    out = {}
    valid = rows["valid"].reshape(F, V) & conv
    for k, v in rows.items():
        if k == "valid":
            continue
        v = v.reshape(F, V, *v.shape[1:])
        out[k] = torch.where(valid.reshape(F, V, *([1] * (v.dim() - 2))), v, torch.zeros_like(v))
    out["valid"] = valid
    return out
