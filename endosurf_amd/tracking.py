"""Surface tracks: the deformation map inverted, points and meshes followed through time.

The model is a canonical SDF and a deformation x_c = x + D(x, t); two observed points are the same piece of tissue exactly when they
map to the same canonical point.  The package evaluates the forward direction only; this module adds the inverse, as the fixed-point
iteration y_k = c - D(y_{k-1}, t) with a per-row stopping rule, and composes it into ``track_points`` / ``track_mesh``: one triangle list
and per-vertex correspondence over a sequence of times, where ``extract_observation_mesh`` gives an unrelated mesh per frame.  Plain torch
in the dtype and on the device of its inputs; ``deform_fn(y, t) -> D`` is any callable on [M,3] points and [M] times, e.g. the fp64
oracle's ``lambda y, t: net.deform(y, t, with_jac=False)[0]`` (a model's ``deform_network`` has that signature for device tensors, a full
point evaluation per call).  ``inverse_deform`` is also the written specification, row rule included, of the device kernel that runs the
whole iteration in one launch (csrc/deform.hip): the functions that solve take ``inverse=``, a callable
``(c, t, init, max_iters, tol) -> (y, step, iters)`` that replaces ``inverse_deform`` over ``deform_fn``, and the renderer's methods of
the same names (``renderer_track``) pass that kernel there.

Contract: where D(., t) has a Lipschitz constant rho < 1 the inverse exists, is unique, and the iteration converges to it
from any start, |y_k - y*| <= rho^k / (1 - rho) |y_1 - y_0|.  Where rho >= 1 the surface folds and nothing is promised: such a row comes
back with ``converged = False`` and finite values.
"""
from __future__ import annotations

import torch


def _times(t, M, like):
    """``t`` (scalar, [1] or [M]) as [M] in the dtype and on the device of ``like``."""
    t = torch.as_tensor(t, dtype=like.dtype, device=like.device).reshape(-1)
    if t.numel() == 1:
        return t.expand(M)
    if t.numel() != M:
        raise ValueError(f"t must be a scalar or one time per row (got {t.numel()} for {M} rows)")
    return t


def inverse_deform(deform_fn, c, t, init=None, max_iters=64, tol=1e-6):
    """y [M,3] with y + D(y, t) = c by the fixed-point iteration y_k = c - D(y_{k-1}, t) from y_0 = ``init`` (``c`` when None).
    Returns (y, step [M], iters [M] int32).  Per row, for k = 1 .. max_iters: the row takes y_k, step = |y_k - y_{k-1}|_2, iters = k,
    and freezes -- nothing of it changes any more -- when tol > 0 and step <= tol; with tol == 0 exactly max_iters evaluations run.
    An update whose length is not finite is not taken: y stays, step = the dtype's largest finite value, the row freezes.  A row has
    converged exactly when step <= tol.  ``deform_fn`` is only ever called on the rows still live, so a row's result depends on its
    own (c, t, init) and on nothing else, provided ``deform_fn`` itself treats rows independently."""
    if int(max_iters) < 1:
        raise ValueError(f"max_iters must be at least 1 (got {max_iters})")
    tol = float(tol)
    if not (0.0 <= tol < float("inf")):
        raise ValueError(f"tol must be finite and not negative (got {tol})")
    c = torch.as_tensor(c)
    M = c.shape[0]
    tt = _times(t, M, c)
    y = (c if init is None else torch.as_tensor(init, dtype=c.dtype, device=c.device)).clone()
    step = torch.zeros(M, dtype=c.dtype, device=c.device)
    iters = torch.zeros(M, dtype=torch.int32, device=c.device)
    live = torch.ones(M, dtype=torch.bool, device=c.device)
    big = torch.finfo(c.dtype).max
    for k in range(1, int(max_iters) + 1):
        idx = torch.nonzero(live).reshape(-1)
        if idx.numel() == 0:
            break
        y_new = c[idx] - deform_fn(y[idx], tt[idx])
        e = y_new - y[idx]
        s = torch.sqrt((e * e).sum(-1))
        ok = s <= big          # (false for inf and nan)
        y[idx[ok]] = y_new[ok]
        step[idx] = torch.where(ok, s, torch.full_like(s, big))
        iters[idx] = k
        live[idx] = ok & ~((s <= tol) & (tol > 0.0))
    return y, step, iters


def _solver(deform_fn, inverse):
    """``inverse`` as given, or ``inverse_deform`` over ``deform_fn`` when it is None: (c, t, init, max_iters, tol) -> (y, step, iters)."""
    if inverse is not None:
        return inverse
    return lambda c, t, init, max_iters, tol: inverse_deform(deform_fn, c, t, init, max_iters, tol)


def _result(y, step, iters, tol):
    return {"points": y, "step": step, "iters": iters, "converged": step <= tol}


def to_canonical(deform_fn, points, t):
    """x_c = x + D(x, t)."""
    points = torch.as_tensor(points)
    return points + deform_fn(points, _times(t, points.shape[0], points))


def to_observed(deform_fn, canonical, t, init=None, max_iters=64, tol=1e-6, inverse=None):
    """The observed positions at ``t`` of canonical points: dict(points, step, iters, converged)."""
    return _result(*_solver(deform_fn, inverse)(canonical, t, init, max_iters, tol), float(tol))


def warp_points(deform_fn, points, t_from, t_to, init=None, max_iters=64, tol=1e-6, inverse=None):
    """Where the tissue seen at ``points`` at ``t_from`` is at ``t_to``: to_observed(to_canonical(points, t_from), t_to)."""
    return to_observed(deform_fn, to_canonical(deform_fn, points, t_from), t_to, init, max_iters, tol, inverse)


def track_points(deform_fn, points, t_from, times, warm_start=False, max_iters=64, tol=1e-6, inverse=None):
    """``points`` [P,3] seen at ``t_from`` followed through ``times`` [F]: dict(points [F,P,3], canonical [P,3], step, iters, converged
    [F,P]).  ``warm_start=False``: all F*P rows in one solve with a time per row, every row starting from its canonical point.
    ``warm_start=True``: the frames in the given order, frame f starting from frame f-1's solution and the first from ``points``."""
    points = torch.as_tensor(points)
    P = points.shape[0]
    times = torch.as_tensor(times, dtype=points.dtype, device=points.device).reshape(-1)
    F = times.numel()
    canon = to_canonical(deform_fn, points, t_from)
    solve = _solver(deform_fn, inverse)
    if not warm_start:
        y, step, iters = solve(canon.repeat(F, 1), times.repeat_interleave(P), None, max_iters, tol)
        y, step, iters = y.reshape(F, P, 3), step.reshape(F, P), iters.reshape(F, P)
    else:
        ys, steps, its, start = [], [], [], points
        for f in range(F):
            start, s, i = solve(canon, times[f], start, max_iters, tol)
            ys.append(start), steps.append(s), its.append(i)
        stack = lambda a, shape, dt: torch.stack(a) if a else torch.zeros(shape, dtype=dt, device=points.device)
        y, step, iters = stack(ys, (0, P, 3), points.dtype), stack(steps, (0, P), points.dtype), stack(its, (0, P), torch.int32)
    return {"points": y, "canonical": canon, "step": step, "iters": iters, "converged": step <= float(tol)}


def track_mesh(deform_fn, vertices, triangles, t, times, warm_start=True, max_iters=64, tol=1e-6, inverse=None):
    """The mesh (vertices [V,3] at time ``t``, triangles) carried through ``times``: one triangle list -- the object passed in -- and
    per-vertex correspondence: dict(vertices [F,V,3], triangles, canonical [V,3], displacement [F,V] = the distance from the source
    vertex, step, iters, converged [F,V])."""
    tr = track_points(deform_fn, vertices, t, times, warm_start, max_iters, tol, inverse)
    v = tr.pop("points")
    disp = torch.sqrt(((v - torch.as_tensor(vertices)[None]) ** 2).sum(-1))
    return {"vertices": v, "triangles": triangles, "displacement": disp, **tr}
