"""Tissue strain along surface tracks: the gradient of the tracked map, its stretches, area and volume ratios.

``tracking`` says where a piece of tissue is at every time; this module says what the tissue does there.  The map "tissue at time t_a ->
tissue at time t_b" is Phi = psi_b^-1 o psi_a with psi_t(x) = x + D(x, t), so at a tracked point (y_a at t_a, y_b at t_b, the same
canonical point) its gradient is

    F = J(y_b, t_b)^-1  J(y_a, t_a),        J(x, t) = I + dD/dx   (the reference's get_deform_grad_from_observed_space),

and the strain relative to the canonical shape is F = J(y_b, t_b)^-1.  From F: det F, the volume ratio; its singular values, the
principal stretches; and with the unit normal n of the surface at the "from" end, |cof(F) n| = det F |F^-T n|, the ratio of the surface
element's area (Nanson), and the two singular values of F restricted to the tangent plane, the stretches within the surface.

Plain torch / numpy; results come back in the dtype and on the device of the inputs.  ``jacobian_fn(y, t) -> J [M,3,3]`` is any callable
on [M,3] points and [M] times, e.g. the fp64 oracle's ``lambda y, t: net.deform(y, t)[1]``.  ``strain_rows`` is the written specification
and the fp64 twin of the device kernel (csrc/strain.hip): the functions that compose it take ``rows_fn=``, a callable
``(jac_from, jac_to, normals) -> dict`` that replaces it, and the renderer's methods of the same names (``renderer_track``) pass the
kernel there with the model's own Jacobian (csrc/deform_jet.hip) as ``jacobian_fn``.

Validity: a row is valid exactly when det J_from > 0 and det J_to > 0 -- both maps preserve orientation there, the
condition under which psi_t is locally invertible and F means anything -- and, where normals are given, its normal has a finite positive
length.  The tests are written as "not > 0", so a NaN anywhere makes the row invalid.  A row that is not valid has zeros in every other
output, finite, like an unconverged row of a track.
"""
from __future__ import annotations

import numpy as np
import torch

from .tracking import _times


def _det3(m):
    return (m[:, 0, 0] * (m[:, 1, 1] * m[:, 2, 2] - m[:, 1, 2] * m[:, 2, 1]) - m[:, 0, 1] * (m[:, 1, 0] * m[:, 2, 2] - m[:, 1, 2] * m[:, 2, 0])
            + m[:, 0, 2] * (m[:, 1, 0] * m[:, 2, 1] - m[:, 1, 1] * m[:, 2, 0]))


def _cof3(m):
    """The cofactor matrices [M,3,3]: cof(m)^T is the adjugate, m^-1 = cof(m)^T / det m."""
    c = np.empty_like(m)
    for i in range(3):
        i1, i2 = (i + 1) % 3, (i + 2) % 3
        for j in range(3):
            j1, j2 = (j + 1) % 3, (j + 2) % 3
            c[:, i, j] = m[:, i1, j1] * m[:, i2, j2] - m[:, i1, j2] * m[:, i2, j1]
    return c


def _rows33(a, M=None):
    a = np.ascontiguousarray(torch.as_tensor(a).detach().cpu().numpy(), dtype=np.float64).reshape(-1, 3, 3)
    if M is not None and a.shape[0] != M:
        raise ValueError(f"jac_from and jac_to must have the same number of rows (got {a.shape[0]} and {M})")
    return a


def strain_rows(jac_from, jac_to, normals=None):
    """The per-row algebra.  ``jac_from``, ``jac_to`` [M,3,3]: J at the two ends of each track row (``jac_from=None``: the identity,
    strain relative to the canonical shape); ``normals`` [M,3]: the surface normal at the "from" end, any finite positive length.
    Returns a dict of
      F [M,3,3] = jac_to^-1 @ jac_from (the inverse by adjugate and determinant);  det [M] = det F = det jac_from / det jac_to;
      stretch [M,3]: the singular values of F, descending;  valid [M] bool (the module's rule);
    and with normals  area [M] = |cof(F) n|;  surface_stretch [M,2]: the singular values of F T, T an orthonormal basis of the plane
    normal to n, descending.  Computed in fp64 (``numpy.linalg.svd``) whatever the inputs are, returned in their dtype, on their device."""
    like = torch.as_tensor(jac_to)
    Jb = _rows33(like)
    M = Jb.shape[0]
    Ja = None if jac_from is None else _rows33(jac_from, M)
    eye = np.broadcast_to(np.eye(3), (M, 3, 3))
    with np.errstate(all="ignore"):
        da = np.ones(M) if Ja is None else _det3(Ja)
        db = _det3(Jb)
        valid = (da > 0.0) & (db > 0.0)          # (false for NaN)
        n = None
        if normals is not None:
            n = np.ascontiguousarray(torch.as_tensor(normals).detach().cpu().numpy(), dtype=np.float64).reshape(-1, 3)
            if n.shape[0] != M:
                raise ValueError(f"normals must have one row per Jacobian (got {n.shape[0]} for {M})")
            length = np.sqrt((n * n).sum(-1))
            n_ok = (length > 0.0) & (length <= np.finfo(np.float64).max)          # (false for NaN)
            valid &= n_ok
            n = np.where(valid[:, None], n / np.where(n_ok, length, 1.0)[:, None], np.array([0.0, 0.0, 1.0]))
        # the rows that are not valid run through the algebra as identities and are zeroed at the end
        Jb = np.where(valid[:, None, None], Jb, eye)
        Ja = eye if Ja is None else np.where(valid[:, None, None], Ja, eye)
        db1 = np.where(valid, db, 1.0)
        F = np.matmul(np.swapaxes(_cof3(Jb), 1, 2), Ja) / db1[:, None, None]
        out = {"F": F, "det": np.where(valid, da, 1.0) / db1,
               "stretch": np.linalg.svd(F, compute_uv=False) if M else np.zeros((0, 3))}
        if n is not None:
            g = np.matmul(_cof3(F), n[:, :, None])[:, :, 0]
            out["area"] = np.sqrt((g * g).sum(-1))
            # T: n x e for the axis e the normal is furthest from, normalised, and n x that
            e = np.eye(3)[np.argmin(np.abs(n), axis=1)] if M else np.zeros((0, 3))
            t1 = np.cross(n, e)
            t1 /= np.sqrt((t1 * t1).sum(-1))[:, None]
            T = np.stack([t1, np.cross(n, t1)], axis=-1)
            out["surface_stretch"] = np.linalg.svd(np.matmul(F, T), compute_uv=False) if M else np.zeros((0, 2))
    dtype = like.dtype if like.dtype.is_floating_point else torch.float64
    res = {}
    for k, v in out.items():
        v = np.where(valid.reshape((M,) + (1,) * (v.ndim - 1)), v, 0.0)
        res[k] = torch.from_numpy(np.ascontiguousarray(v)).to(device=like.device, dtype=dtype)
    res["valid"] = torch.from_numpy(valid).to(like.device)
    return res


def track_strain(jacobian_fn, points_from, t_from, points_to, t_to, normals=None, rows_fn=None):
    """The strain of the tissue between the two ends of track rows: ``points_from`` [M,3] at ``t_from`` and ``points_to`` [M,3] at
    ``t_to`` (scalar or [M] times) are the same tissue, e.g. ``points`` and ``warp_points(...)["points"]``.  ``points_from=None``
    selects the canonical reference (``t_from`` is not read).  ``normals`` [M,3] at the "from" end.  ``strain_rows``' dict."""
    points_to = torch.as_tensor(points_to)
    M = points_to.shape[0]
    jac_to = jacobian_fn(points_to, _times(t_to, M, points_to))
    jac_from = None
    if points_from is not None:
        points_from = torch.as_tensor(points_from)
        if points_from.shape[0] != M:
            raise ValueError(f"points_from and points_to must have the same number of rows (got {points_from.shape[0]} and {M})")
        jac_from = jacobian_fn(points_from, _times(t_from, M, points_from))
    return (rows_fn or strain_rows)(jac_from, jac_to, normals)


def mesh_strain(jacobian_fn, track, times, reference=0, normals=None, normals_fn=None, rows_fn=None):
    """The strain maps of a tracked mesh, the dict of ``tracking.track_mesh`` over ``times`` [F]: every frame against the frame
    ``reference`` (an index into ``times``), or against the canonical shape (``reference="canonical"``: the reference vertices are
    ``track["canonical"]`` and there is no J_from).  Every output of ``strain_rows`` as [F,V,...]; ``valid`` also requires
    ``track["converged"]`` of the frame and of the reference frame, and a row that is not valid is zero as everywhere.  ``normals``
    [V,3] at the reference vertices; None: ``normals_fn(vertices, triangles)`` (default ``meshing.vertex_normals``) of the reference
    vertices and ``track["triangles"]``.  J is evaluated once, on all F*V rows with a time per row; the reference frame's rows of
    it are J_from."""
    verts = torch.as_tensor(track["vertices"])
    F, V = int(verts.shape[0]), int(verts.shape[1])
    times = torch.as_tensor(times, dtype=verts.dtype, device=verts.device).reshape(-1)
    if times.numel() != F:
        raise ValueError(f"times must hold one time per tracked frame (got {times.numel()} for {F})")
    conv = torch.as_tensor(track["converged"]).to(verts.device).reshape(F, V)
    canonical = isinstance(reference, str)
    if canonical:
        if reference != "canonical":
            raise ValueError(f"reference must be a frame index or 'canonical' (got {reference!r})")
        ref_verts = torch.as_tensor(track["canonical"])
    else:
        r = int(reference)
        if not 0 <= r < F:
            raise ValueError(f"reference must be a frame index in [0, {F}) or 'canonical' (got {reference!r})")
        ref_verts = verts[r]
        conv = conv & conv[r][None]
    if normals is None:
        if normals_fn is None:
            from .meshing import vertex_normals
            normals_fn = lambda v, f: torch.from_numpy(vertex_normals(torch.as_tensor(v).detach().cpu().numpy(),
                                                                      torch.as_tensor(f).detach().cpu().numpy()))
        normals = normals_fn(ref_verts, track["triangles"])
    normals = torch.as_tensor(normals).to(device=verts.device).reshape(V, 3)
    jac = jacobian_fn(verts.reshape(F * V, 3), times.repeat_interleave(V)).reshape(F, V, 3, 3)
    jac_from = None if canonical else jac[r][None].expand(F, V, 3, 3).reshape(F * V, 3, 3)
    rows = (rows_fn or strain_rows)(jac_from, jac.reshape(F * V, 3, 3), normals[None].expand(F, V, 3).reshape(F * V, 3))
    out = {}
    valid = rows["valid"].reshape(F, V) & conv
    for k, v in rows.items():
        if k == "valid":
            continue
        v = v.reshape(F, V, *v.shape[1:])
        out[k] = torch.where(valid.reshape(F, V, *([1] * (v.dim() - 2))), v, torch.zeros_like(v))
    out["valid"] = valid
    return out


def triangle_area_ratio(vertices_from, vertices_to, triangles):
    """Area of every triangle at ``vertices_to`` [..., V, 3] over its area at ``vertices_from`` [V,3] (or [..., V, 3]): the discrete
    counterpart of ``area``, [..., T] in fp64 arithmetic and the dtype of ``vertices_to``.  A triangle without an area in
    ``vertices_from`` gives inf or nan."""
    vt = torch.as_tensor(vertices_to)
    vf = torch.as_tensor(vertices_from).to(vt.device)
    f = torch.as_tensor(triangles).to(device=vt.device, dtype=torch.int64).reshape(-1, 3)

    def areas(v):
        v = v.to(torch.float64)
        a, b, c = v[..., f[:, 0], :], v[..., f[:, 1], :], v[..., f[:, 2], :]
        return 0.5 * torch.linalg.norm(torch.linalg.cross(b - a, c - a), dim=-1)
    return (areas(vt) / areas(vf)).to(vt.dtype if vt.dtype.is_floating_point else torch.float64)
