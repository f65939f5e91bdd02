"""Least-squares rigid motion from correspondences: Kabsch for given correspondences (the frames of a surface track) and iterative
closest point against the triangles of a mesh for found ones.  numpy only; this module is the specification and the fp64 host twin of
csrc/register.hip (``Engine.rigid_moments`` / ``rigid_fit`` / ``rigid_apply`` / ``track_rigid`` / ``icp``).  Coordinates
and weights are what the device reads, fp32; all arithmetic is fp64 on them; x.y = (x0 y0 + x1 y1) + x2 y2."""
from __future__ import annotations

import math

import numpy as np

from . import meshing

CONVERGED, MAX_ITERS, DEGENERATE = 0, 1, 2          # icp's status (csrc/register.hip ICP_*)
STATUS_NAMES = ("CONVERGED", "MAX_ITERS", "DEGENERATE")
METHODS = {"point": 0, "plane": 1}                   # the ``method`` word of es_icp_update
RANK_REL = 1e-12                                     # second singular value <= RANK_REL x the first: collinear, no rotation is determined
PIVOT_REL = 1e-12                                    # Cholesky pivot <= PIVOT_REL x the largest diagonal entry: the 6 x 6 system is singular
MOMENTS = 17                                         # W, sum w p (3), sum w q (3), sum w p q^T (9, row-major), sum w |p - q|^2
NORMAL_SUMS = 29                                     # 21 upper entries of A^T A (row-major), 6 of A^T b, sum w r^2, sum w
MOMENT_CHUNK = 1024                                  # rows one workgroup of the device's first reduction stage adds (register.hip REG_CHUNK)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _rows(a, what):
    a = np.asarray(a, np.float64)
    if a.ndim not in (2, 3) or a.shape[-1] != 3:
        raise ValueError(f"{what} must be [N, 3] or [B, N, 3] (got {a.shape})")
    return a


def _pair(p, q, w):
    """(p [B,N,3], q [B,N,3], w [B,N] fp64 with 0 for a row that takes no part, whether the call was unbatched)."""
    p, q = _rows(p, "p"), _rows(q, "q")
    single = p.ndim == 2 and q.ndim == 2
    p, q = (a[None] if a.ndim == 2 else a for a in (p, q))
    B = max(p.shape[0], q.shape[0])
    if p.shape[1] != q.shape[1] or p.shape[0] not in (1, B) or q.shape[0] not in (1, B):
        raise ValueError(f"p {p.shape} and q {q.shape} do not pair up")
    N = p.shape[1]
    p, q = np.broadcast_to(p, (B, N, 3)), np.broadcast_to(q, (B, N, 3))
    w = np.ones((B, N)) if w is None else np.asarray(w, np.float64)
    if w.shape not in ((N,), (B, N)):
        raise ValueError(f"w must be [N] or [B, N] = {(B, N)} (got {w.shape})")
    w = np.broadcast_to(w, (B, N))
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(w) & (w > 0) & np.isfinite(p).all(-1) & np.isfinite(q).all(-1)
    return p, q, np.where(ok, w, 0.0), ok, single


def rigid_moments(p, q, w=None):
    """[B,17] fp64 (17 for unbatched input): W = sum w, sum w p (3), sum w q (3), sum w p q^T (9, row-major: entry 7 + 3 i + j is
    sum w p_i q_j), sum w |p - q|^2, over the rows of ``p``, ``q`` [B,N,3] with weights ``w`` [B,N], [N] or None (ones).  A row takes
    part only if its w is finite and > 0 and all six coordinates are finite; otherwise its weight is 0."""
    p, q, w, ok, single = _pair(p, q, w)
    p, q = np.where(ok[..., None], p, 0.0), np.where(ok[..., None], q, 0.0)
    d = p - q
    out = np.concatenate([w.sum(1)[:, None], (w[..., None] * p).sum(1), (w[..., None] * q).sum(1),
                          ((w[..., None] * p)[..., :, None] * q[..., None, :]).sum(1).reshape(-1, 9),
                          (w * ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])).sum(1)[:, None]], 1)
    return out[0] if single else out


def solve_moments(m):
    """One row of ``rigid_moments`` -> (rotation [3,3], translation [3], weight, valid): the proper rotation and the translation that
    minimise sum w |R p + t - q|^2.  With the means pm = (sum w p) / W and qm, the centred covariance is
    S = sum w p q^T - (sum w p) (sum w q)^T / W = U diag(s) V^T (s descending), R = V diag(1, 1, det(V U^T)) U^T, t = qm - R pm.
    W == 0: not valid, R = I, t = 0.  s[1] <= 1e-12 s[0] (coincident or collinear points): not valid, R = I, t = qm - pm."""
    m = np.asarray(m, np.float64)
    W = float(m[0])
    if not W > 0.0:
        return np.eye(3), np.zeros(3), 0.0, False
    pm, qm = m[1:4] / W, m[4:7] / W
    S = m[7:16].reshape(3, 3) - (m[1:4, None] * m[None, 4:7]) / W
    U, s, Vt = np.linalg.svd(S)
    if not s[1] > RANK_REL * s[0]:
        return np.eye(3), qm - pm, W, False
    V = Vt.T
    D = np.diag([1.0, 1.0, 1.0 if np.linalg.det(V @ U.T) > 0 else -1.0])
    R = V @ D @ U.T
    return R, qm - R @ pm, W, True


def rigid_apply(rotation, translation, p):
    """R p + t evaluated in fp64, ((R_i0 p_0 + R_i1 p_1) + R_i2 p_2) + t_i, and rounded to fp32: ``rotation`` [B,3,3] / [3,3],
    ``translation`` [B,3] / [3], ``p`` [B,N,3] or [N,3] (one [N,3] is shared by all B motions) -> [B,N,3] / [N,3] fp32."""
    return _apply64(rotation, translation, p).astype(np.float32)


def _apply64(rotation, translation, p):
    R, t, p = np.asarray(rotation, np.float64), np.asarray(translation, np.float64), _rows(p, "p")
    if R.ndim == 3 and p.ndim == 2:
        p = p[None]
    R, t = (R[..., None, :, :], t[..., None, :]) if p.ndim == 3 or R.ndim == 3 else (R, t)
    return ((R[..., 0] * p[..., None, 0] + R[..., 1] * p[..., None, 1]) + R[..., 2] * p[..., None, 2]) + t


def rigid_fit(p, q, w=None):
    """dict(rotation [B,3,3], translation [B,3], rmse [B], weight [B], valid [B]) (unbatched for [N,3] inputs): ``solve_moments`` of
    ``rigid_moments(p, q, w)`` per batch.  rmse = sqrt(sum w |x - q|^2 / W) with x = ``rigid_apply(R, t, p)``, the moved rows as the
    device stores them (fp32), by a second moments pass: the closed form from the first moments cancels near a perfect fit.  W == 0
    gives rmse 0."""
    pp, qq, ww, _, single = _pair(p, q, w)
    m = rigid_moments(pp, qq, ww)
    sol = [solve_moments(row) for row in m]
    R, t = np.stack([s[0] for s in sol]), np.stack([s[1] for s in sol])
    W, valid = np.array([s[2] for s in sol]), np.array([s[3] for s in sol], bool)
    m2 = rigid_moments(rigid_apply(R, t, pp), qq, ww)
    rmse = np.sqrt(np.where(W > 0, m2[:, 16] / np.where(W > 0, W, 1.0), 0.0))
    out = {"rotation": R, "translation": t, "rmse": rmse, "weight": W, "valid": valid}
    return {k: v[0] for k, v in out.items()} if single else out


def track_rigid(track_or_vertices, reference=0, weights=None):
    """The rigid part of a surface track and what is left: ``track_or_vertices`` is the dict of ``track_mesh`` (its [F,V,3] vertices)
    or the [F,V,3] array.  Per frame f the motion from frame ``reference`` to frame f, x_f ~ R_f x_ref + t_f (``rigid_fit`` with the
    per-vertex ``weights`` [V] or None; the reference frame is not special-cased).  Returns the dict (a copy, or a new one) with
    rotation [F,3,3], translation [F,3], rmse [F], valid [F] and, fp32, residual [F,V,3] = x_f - (R_f x_ref + t_f) and residual_norm
    [F,V] = |residual|, both evaluated in fp64 before the rounding."""
    is_dict = isinstance(track_or_vertices, dict)
    v = np.asarray(track_or_vertices["vertices"] if is_dict else track_or_vertices, np.float32).astype(np.float64)
    if v.ndim != 3 or v.shape[-1] != 3:
        raise ValueError(f"track_rigid takes [F, V, 3] vertices (got {v.shape})")
    F = v.shape[0]
    if not -F <= int(reference) < F:
        raise ValueError(f"track_rigid: reference frame {reference} of {F}")
    ref = v[int(reference) % F]
    fit = rigid_fit(ref[None], v, weights)
    res = v - _apply64(fit["rotation"], fit["translation"], ref)
    out = dict(track_or_vertices) if is_dict else {}
    out.update(rotation=fit["rotation"], translation=fit["translation"], rmse=fit["rmse"], valid=fit["valid"],
               residual=res.astype(np.float32), residual_norm=np.sqrt(_dot(res, res)).astype(np.float32))
    return out


# ---- iterative closest point against the triangles of a mesh ------------------------------------------------------------------------------
def rodrigues(omega):
    """The rotation by |omega| about omega, I + a K + b K^2 with K = [omega]_x, a = sin(th) / th, b = (sin(th / 2) / (th / 2))^2 / 2
    (no cancellation at small angles); th == 0 gives I."""
    w = np.asarray(omega, np.float64)
    th = math.sqrt(float(_dot(w, w)))
    half = 0.5 * th
    a = math.sin(th) / th if th > 0.0 else 1.0
    s = math.sin(half) / half if th > 0.0 else 1.0
    b = 0.5 * (s * s)
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    return np.eye(3) + a * K + b * (K @ K)


def rotation_angle(R):
    """atan2(|v|, (trace R - 1) / 2) with v = the axial vector of (R - R^T) / 2: accurate at small angles."""
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return math.atan2(math.sqrt(float(_dot(v, v))), 0.5 * (R[0, 0] + R[1, 1] + R[2, 2] - 1.0))


def icp_weights(triangle, dist, max_distance=None):
    """Weight 1 for a row that has a closest triangle and, if ``max_distance`` is given, dist <= max_distance (compared in fp64);
    0 otherwise."""
    w = np.asarray(triangle) >= 0
    if max_distance is not None:
        w = w & (np.asarray(dist, np.float64) <= float(max_distance))
    return w.astype(np.float64)


def normal_equations(x, closest, triangle, dist, vertices, triangles, max_distance=None):
    """The 29 sums of one point-to-plane step (fp64): per row with weight 1 (``icp_weights``, a triangle index in [0, T) whose corners
    lie in [0, V), finite coordinates, and a triangle with area: n2 = |(v1 - v0) x (v2 - v0)|^2 > 0) the unit normal n = that cross
    product / sqrt(n2) from the fp32 corners, the row a = (x x n, n) of the 6 unknowns (omega, tau) and the residual r = (x - c).n of
    the linearised ((omega x x) + tau + x - c).n.  out = the 21 upper entries of sum a a^T (row-major), sum a b with b = -r (6),
    sum r^2, sum 1."""
    x, c = np.asarray(x, np.float32).astype(np.float64).reshape(-1, 3), np.asarray(closest, np.float32).astype(np.float64).reshape(-1, 3)
    v = np.asarray(vertices, np.float32).astype(np.float64).reshape(-1, 3)
    tri_all = np.asarray(triangles, np.int64).reshape(-1, 3)
    t = np.asarray(triangle, np.int64)
    ok = icp_weights(t, dist, max_distance) > 0
    ok &= (t >= 0) & (t < len(tri_all)) & np.isfinite(x).all(1) & np.isfinite(c).all(1)
    idx = tri_all[np.where(ok, t, 0)] if len(tri_all) else np.zeros((len(t), 3), np.int64)
    ok &= ((idx >= 0) & (idx < len(v))).all(1)
    idx = np.where(ok[:, None], idx, 0)
    out = np.zeros(NORMAL_SUMS)
    if not ok.any():
        return out
    v0, v1, v2 = v[idx[:, 0]], v[idx[:, 1]], v[idx[:, 2]]
    n = np.cross(v1 - v0, v2 - v0)
    n2 = _dot(n, n)
    with np.errstate(invalid="ignore", divide="ignore"):
        ok &= n2 > 0.0
        n = n / np.sqrt(n2)[:, None]
    a = np.concatenate([np.cross(x, n), n], 1)[ok]
    r = _dot(x - c, n)[ok]
    k = 0
    for i in range(6):
        for j in range(i, 6):
            out[k] = (a[:, i] * a[:, j]).sum()
            k += 1
    out[21:27] = -(a * r[:, None]).sum(0)
    out[27], out[28] = (r * r).sum(), float(len(r))
    return out


def solve_normal_equations(sums):
    """(omega [3], tau [3]) from the 29 sums by a Cholesky factorisation of the 6 x 6 matrix in fp64, or None where the system is
    degenerate: total weight 0, or a pivot <= 1e-12 x the largest diagonal entry."""
    s = np.asarray(sums, np.float64)
    if not s[28] > 0.0:
        return None
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = s[:21]
    A = A + np.triu(A, 1).T
    floor = PIVOT_REL * float(np.max(np.diag(A)))
    L = np.zeros((6, 6))
    for j in range(6):
        d = A[j, j]
        for k in range(j):
            d -= L[j, k] * L[j, k]
        if not d > floor:
            return None
        L[j, j] = math.sqrt(d)
        for i in range(j + 1, 6):
            e = A[i, j]
            for k in range(j):
                e -= L[i, k] * L[j, k]
            L[i, j] = e / L[j, j]
    y = np.zeros(6)
    for i in range(6):
        e = s[21 + i]
        for k in range(i):
            e -= L[i, k] * y[k]
        y[i] = e / L[i, i]
    z = np.zeros(6)
    for i in range(5, -1, -1):
        e = y[i]
        for k in range(i + 1, 6):
            e -= L[k, i] * z[k]
        z[i] = e / L[i, i]
    return z[:3], z[3:]


def icp_update(R, t, sums_or_moments, method):
    """One update of the transform from the sums of an iteration: (R', t', step) or None where the system is degenerate.
    "plane": ``solve_normal_equations``, dR = ``rodrigues(omega)``, dt = tau, angle = |omega|.  "point": ``solve_moments`` (must be
    valid), angle = ``rotation_angle(dR)``.  R' = dR R, t' = dR t + dt, step = max(angle, |dt|)."""
    if method == "plane":
        sol = solve_normal_equations(sums_or_moments)
        if sol is None:
            return None
        dR, dt = rodrigues(sol[0]), sol[1]
        angle = math.sqrt(float(_dot(sol[0], sol[0])))
    else:
        dR, dt, _, valid = solve_moments(sums_or_moments)
        if not valid:
            return None
        angle = rotation_angle(dR)
    return dR @ R, dR @ t + dt, max(angle, math.sqrt(float(_dot(dt, dt))))


def icp(points, vertices, triangles, method="plane", max_iters=50, tol=1e-6, max_distance=None, init=None):
    """Iterative closest point of ``points`` [N,3] against the *triangles* of a mesh: the rigid motion (R, t) that lays R p + t onto
    the surface.  One iteration: x = ``rigid_apply(R, t, points)`` (fp32); closest triangle and closest point of each x
    (``meshing.point_to_mesh``); weights by ``icp_weights``; then ``icp_update`` -- "point": the rigid fit of x onto its closest
    points; "plane" (the default: point-to-point slides slowly along a smooth surface): the linearised point-to-plane step.  The loop
    stops at step < tol (CONVERGED), after ``max_iters`` updates (MAX_ITERS) or at a degenerate system (DEGENERATE, the transform of
    the previous iteration is kept).  ``init`` = (R, t) seeds it.

    dict(rotation [3,3], translation [3], iterations (updates applied), status, step (of the last update; inf before the first),
    rmse, inliers, points [N,3] fp32 (the moved rows), distance [N] fp32, triangle [N] int32): the last five from one final
    closest-triangle pass with the final transform, rmse = sqrt(sum w |x - c|^2 / sum w) and inliers = sum w over its weights."""
    if method not in METHODS:
        raise ValueError(f"icp: method must be 'point' or 'plane' (got {method!r})")
    p = np.asarray(points, np.float32).reshape(-1, 3)
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    R, t = (np.eye(3), np.zeros(3)) if init is None else (np.array(init[0], np.float64).reshape(3, 3), np.array(init[1], np.float64).reshape(3))
    iterations, status, step = 0, MAX_ITERS, math.inf
    while iterations < int(max_iters):
        x = rigid_apply(R, t, p)
        dist, tri, closest = meshing.point_to_mesh(x, v, triangles)
        if method == "plane":
            sums = normal_equations(x, closest, tri, dist, v, triangles, max_distance)
        else:
            sums = rigid_moments(x, closest, icp_weights(tri, dist, max_distance))
        upd = icp_update(R, t, sums, method)
        if upd is None:
            status = DEGENERATE
            break
        R, t, step = upd
        iterations += 1
        if step < tol:
            status = CONVERGED
            break
    x = rigid_apply(R, t, p)
    dist, tri, closest = meshing.point_to_mesh(x, v, triangles)
    m = rigid_moments(x, closest, icp_weights(tri, dist, max_distance))
    return {"rotation": R, "translation": t, "iterations": iterations, "status": status, "step": step,
            "rmse": math.sqrt(m[16] / m[0]) if m[0] > 0 else 0.0, "inliers": int(m[0]), "points": x, "distance": dist, "triangle": tri}
