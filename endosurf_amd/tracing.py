"""Surface tracing: where a ray meets the level set  sdf(x, t) = tau, by sphere tracing with a bracket phase.

``ray_marching`` (the reference's routine, reproduced faithfully for training) evaluates 128 proposals and 8 secant points per ray, and
its depth is not on the surface: the reference negates the proposal values but feeds its secant un-negated ones, so each secant step
replaces the wrong end of the bracket.  ``trace_surface`` walks each ray by the field's own value, brackets the surface
when a step overshoots it -- |grad sdf| of a trained field exceeds 1 -- and refines the bracket by regula falsi with a bisection fall-back
until |sdf - tau| <= eps.  Plain torch in the dtype and on the device of ``rays``; ``sdf_fn(x [M,3], t [M,1]) -> [M,1]`` is any callable,
e.g. the fp64 oracle's ``net.sdf_observed``.  This function is also the written specification, row rule included, of the device kernel
that runs a tile's whole iteration in one launch (csrc/trace.hip); the renderer's ``trace_surface`` passes that kernel
the same arguments through the same checks.

Conventions (``ray_marching``'s and ``renderondepth``'s, so the depths are interchangeable):  w = d / (d_z + 1e-6), a point is
o + z w, (near, far) are the unit-sphere intersection ``ray_marching`` uses, s = |w|.  Every product and sum is taken one by one (no
fused multiply-adds), in the order written here.
"""
from __future__ import annotations

import math

import torch

HIT, MISS, OCCUPIED, NOT_CONVERGED = 1, 2, 3, 4
MAX_ITERS_CAP = 1024


def check_trace_args(tau=0.0, eps=1e-5, relax=1.0, min_step=1e-3, max_iters=128):
    """The argument checks of ``trace_surface``, shared by the device path: returns (tau, eps, relax, min_step, max_iters) as Python
    floats and an int, or raises ValueError naming the argument."""
    tau, eps, relax, min_step = float(tau), float(eps), float(relax), float(min_step)
    if not math.isfinite(tau):
        raise ValueError(f"tau must be finite (got {tau})")
    if not (0.0 <= eps < math.inf):
        raise ValueError(f"eps must be finite and not negative (got {eps})")
    if not (0.0 < relax <= 1.0):
        raise ValueError(f"relax must be in (0, 1] (got {relax})")
    if not (0.0 < min_step < math.inf):
        raise ValueError(f"min_step must be finite and positive (got {min_step})")
    if int(max_iters) != max_iters or not (1 <= int(max_iters) <= MAX_ITERS_CAP):
        raise ValueError(f"max_iters must be an integer in [1, {MAX_ITERS_CAP}] (got {max_iters})")
    return tau, eps, relax, min_step, int(max_iters)


def _dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def ray_geometry(rays):
    """(o [N,3], w [N,3], s [N], near [N], far [N], t [N]) of rays [N,9]: w = d / (d_z + 1e-6), s = |w|, (near, far) the unit-sphere
    intersection of ``ray_marching`` (near clamped at 0), every product and sum taken one by one."""
    o, d, t = rays[:, :3], rays[:, 3:6], rays[:, 8]
    dd = _dot(d, d)
    d1 = -_dot(d, o) / dd
    p = o + d1[:, None] * d
    tmp = 1.0 - _dot(p, p)
    d2 = torch.sqrt(torch.clamp(tmp, min=0.0)) / torch.sqrt(dd)
    near = torch.clamp(d1 - d2, min=0.0)
    far = d1 + d2
    w = d / (d[:, 2:] + 1e-6)
    return o, w, torch.sqrt(_dot(w, w)), near, far, t


def _next(z_lo, f_lo, z_hi, f_hi):
    """The next depth inside the bracket: the regula-falsi point, the midpoint if that is not strictly inside, and ``exhausted`` where
    neither is -- the bracket has no interior in this precision."""
    rf = z_lo - f_lo * (z_hi - z_lo) / (f_hi - f_lo)
    mid = 0.5 * (z_lo + z_hi)
    rf_in = (rf > z_lo) & (rf < z_hi)          # (false for NaN)
    mid_in = (mid > z_lo) & (mid < z_hi)
    return torch.where(rf_in, rf, mid), ~rf_in & ~mid_in


def trace_surface(sdf_fn, rays, tau=0.0, eps=1e-5, relax=1.0, min_step=1e-3, max_iters=128):
    """dict(depth [N,1], status [N] int32, iters [N] int32, residual [N], points [N,3]) for rays [N,9].  Per row ("Row
    rule"):

      If ``far > near`` is false: MISS, iters = 0, depth = inf, points = 0.
      Otherwise z = near, phase MARCH, and for k = 1 .. max_iters:
        f = sdf(o + z w, t) - tau; iters = k; residual = f; points is the point just evaluated.
        If f is not finite: NOT_CONVERGED, stop.
        If |f| <= eps: HIT, depth = z, stop.
        In MARCH with f > 0: (z_lo, f_lo) = (z, f); z = z + max(relax f / s, min_step); if z > far: MISS, stop.
        In MARCH with f < 0: if k == 1: OCCUPIED, depth = 0, stop; otherwise (z_hi, f_hi) = (z, f), phase REFINE,
          z = next(z_lo, f_lo, z_hi, f_hi).
        In REFINE: f > 0 replaces (z_lo, f_lo), otherwise (z_hi, f_hi); z = next(...).
        next: the regula-falsi point z_lo - f_lo (z_hi - z_lo) / (f_hi - f_lo); if it is not strictly inside (z_lo, z_hi), the midpoint
          0.5 (z_lo + z_hi); if that is not strictly inside either, the bracket has no interior in this precision and the row stops as
          HIT at z_lo, with residual = f_lo and points the point of z_lo.
      After the loop: NOT_CONVERGED.
      depth is z for HIT, 0 for OCCUPIED, inf for MISS and NOT_CONVERGED: ``ray_marching``'s three kinds of value, so
      ``renderondepth(rays, depth)`` takes it as it is.

    ``sdf_fn`` is only ever called on the rows still live, so a row's result depends on its own ray and on nothing else, provided
    ``sdf_fn`` itself treats rows independently."""
    tau, eps, relax, min_step, max_iters = check_trace_args(tau, eps, relax, min_step, max_iters)
    rays = torch.as_tensor(rays)
    if rays.dim() != 2 or rays.shape[1] != 9 or not rays.dtype.is_floating_point:
        raise ValueError(f"rays must be a floating [N, 9] tensor (got {tuple(rays.shape)}, {rays.dtype})")
    N, dt, dev = rays.shape[0], rays.dtype, rays.device
    o, w, s, near, far, t = ray_geometry(rays)
    c = lambda v: torch.tensor(v, dtype=dt, device=dev)
    tau_, eps_, relax_, min_step_ = c(tau), c(eps), c(relax), c(min_step)
    inf = float("inf")

    status = torch.zeros(N, dtype=torch.int32, device=dev)          # 0: live
    iters = torch.zeros(N, dtype=torch.int32, device=dev)
    residual = torch.zeros(N, dtype=dt, device=dev)
    points = torch.zeros(N, 3, dtype=dt, device=dev)
    depth = torch.full((N,), inf, dtype=dt, device=dev)
    z = near.clone()
    z_lo, f_lo, z_hi, f_hi = (torch.zeros(N, dtype=dt, device=dev) for _ in range(4))
    refine = torch.zeros(N, dtype=torch.bool, device=dev)
    status[~(far > near)] = MISS

    for k in range(1, max_iters + 1):
        idx = torch.nonzero(status == 0).reshape(-1)
        if idx.numel() == 0:
            break
        zi, oi, wi = z[idx], o[idx], w[idx]
        x = oi + zi[:, None] * wi
        f = sdf_fn(x, t[idx][:, None]).reshape(-1).to(dt) - tau_
        iters[idx] = k
        fin = torch.isfinite(f)
        hit = fin & (f.abs() <= eps_)
        pos, neg, ref = fin & ~hit & (f > 0), fin & ~hit & (f < 0), refine[idx]
        st = torch.zeros_like(status[idx])
        st[~fin] = NOT_CONVERGED
        st[hit] = HIT
        dep = torch.where(hit, zi, torch.full_like(zi, inf))
        res, pts = f.clone(), x.clone()
        lo_z, lo_f, hi_z, hi_f = z_lo[idx], f_lo[idx], z_hi[idx], f_hi[idx]
        # MARCH
        mp, mn = pos & ~ref, neg & ~ref
        lo_z, lo_f = torch.where(mp, zi, lo_z), torch.where(mp, f, lo_f)
        z_march = zi + torch.maximum(relax_ * f / s[idx], min_step_)
        st[mp & (z_march > far[idx])] = MISS
        if k == 1:
            st[mn] = OCCUPIED
            dep = torch.where(mn, torch.zeros_like(dep), dep)
            mn = mn & False
        # REFINE (and the step of MARCH that enters it)
        rp, rn = pos & ref, (neg & ref) | mn
        lo_z, lo_f = torch.where(rp, zi, lo_z), torch.where(rp, f, lo_f)
        hi_z, hi_f = torch.where(rn, zi, hi_z), torch.where(rn, f, hi_f)
        z_ref, exhausted = _next(lo_z, lo_f, hi_z, hi_f)
        exhausted = exhausted & (rp | rn)
        st[exhausted] = HIT
        dep = torch.where(exhausted, lo_z, dep)
        res = torch.where(exhausted, lo_f, res)
        pts = torch.where(exhausted[:, None], oi + lo_z[:, None] * wi, pts)
        # back into the rows
        z[idx] = torch.where(mp, z_march, torch.where(rp | rn, z_ref, zi))
        z_lo[idx], f_lo[idx], z_hi[idx], f_hi[idx] = lo_z, lo_f, hi_z, hi_f
        refine[idx] = ref | rn
        status[idx], depth[idx], residual[idx], points[idx] = st, dep, res, pts
    status[status == 0] = NOT_CONVERGED
    return {"depth": depth[:, None], "status": status, "iters": iters, "residual": residual, "points": points}
