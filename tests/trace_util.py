"""Shared by the surface-tracing tests: the cases, their rays, the fp64 / fp32 oracles, the host twin's results on them
(computed once per process) and a second, scalar restatement of the row rule in Python floats."""
import functools
import math

import torch

import weightgen
from oracle import endosurf_oracle as O
from oracle_util import RENDER_CFG

from endosurf_amd import tracing as T

CASES = [("trained", 11), ("trained", 23), ("init", 21)]
N_RAYS = 515
EPS = 1e-5
# The two conditions under which a trajectory in fp32 counts as the fp64 twin's (checked on the CPU for the fp32 oracle twin in
# tests/test_trace_host.py, reused for the device in tests/test_gpu_trace.py): rows whose status differs, rows whose iters differ.
STATUS_CAP, ITERS_CAP = 4, 8


def rays515():
    return torch.from_numpy(weightgen.make_rays(91, N_RAYS))


def oracle_net(state, dtype, use_deform):
    return O.OracleNet({k: torch.tensor(v, dtype=dtype) for k, v in state.items()}, bool(use_deform))


def sdf_fn(net):
    def fn(x, t):
        with torch.no_grad():
            return net.sdf_observed(x, t)
    return fn


@functools.lru_cache(maxsize=None)
def case(mode, seed, use_deform):
    """One state with or without its deformation network: the oracles and the host twin in fp64 and fp32 at the defaults on the 515 rays."""
    state = weightgen.make_state(seed, mode, True)
    rays = rays515()
    net64, net32 = oracle_net(state, torch.float64, use_deform), oracle_net(state, torch.float32, use_deform)
    return dict(state=state, rays=rays, net64=net64, net32=net32, name=f"{mode}{seed}{'' if use_deform else '-static'}",
                twin64=T.trace_surface(sdf_fn(net64), rays.double(), eps=EPS), twin32=T.trace_surface(sdf_fn(net32), rays, eps=EPS))


@functools.lru_cache(maxsize=None)
def marching64(mode, seed, use_deform):
    """The fp64 oracle's ``ray_marching`` depth [N] on the case's rays."""
    c = case(mode, seed, use_deform)
    with torch.no_grad():
        return O.OracleRenderer(c["net64"], RENDER_CFG).ray_marching(c["rays"].double())[:, 0]


def sdf64(c, points, rays):
    """|sdf| is asked of the fp64 oracle at fp32 or fp64 ``points`` with the rays' times."""
    with torch.no_grad():
        return c["net64"].sdf_observed(points.double(), rays[:, 8:9].double())[:, 0]


def sqrt64(v):
    """torch's own fp64 square root of a Python float: on some CPUs its last bit is not the correctly rounded one that ``math.sqrt``
    gives, and the comparison of the twin with ``trace_scalar`` is about the row rule, not about how a platform rounds a root."""
    return float(torch.sqrt(torch.tensor(v, dtype=torch.float64)))


def trace_scalar(field, ray, tau=0.0, eps=1e-5, relax=1.0, min_step=1e-3, max_iters=128):
    """The row rule of DESIGN.md 7j for ONE ray, in Python floats (IEEE double, one operation at a time): a second restatement, written
    from the rule and sharing no code with ``tracing.trace_surface``.  ``field(x0, x1, x2, t) -> float``.  Returns (depth, status, iters,
    residual, (p0, p1, p2), entered_refine)."""
    o, d, t = [float(v) for v in ray[:3]], [float(v) for v in ray[3:6]], float(ray[8])
    dot = lambda a, b: a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
    dd = dot(d, d)
    d1 = -dot(d, o) / dd
    p = [o[i] + d1 * d[i] for i in range(3)]
    d2 = sqrt64(max(1.0 - dot(p, p), 0.0)) / sqrt64(dd)
    near, far = max(d1 - d2, 0.0), d1 + d2
    w = [d[i] / (d[2] + 1e-6) for i in range(3)]
    s = sqrt64(dot(w, w))
    at = lambda z: tuple(o[i] + z * w[i] for i in range(3))
    inf = float("inf")
    if not far > near:
        return inf, T.MISS, 0, 0.0, (0.0, 0.0, 0.0), False
    z, refine, z_lo, f_lo, z_hi, f_hi = near, False, 0.0, 0.0, 0.0, 0.0
    for k in range(1, max_iters + 1):
        x = at(z)
        f = field(*x, t) - tau
        if not math.isfinite(f):
            return inf, T.NOT_CONVERGED, k, f, x, refine
        if abs(f) <= eps:
            return z, T.HIT, k, f, x, refine
        if not refine and f > 0:
            z_lo, f_lo = z, f
            z = z + max(relax * f / s, min_step)
            if z > far:
                return inf, T.MISS, k, f, x, refine
            continue
        if not refine:
            if k == 1:
                return 0.0, T.OCCUPIED, k, f, x, refine
            refine = True
            z_hi, f_hi = z, f
        elif f > 0:
            z_lo, f_lo = z, f
        else:
            z_hi, f_hi = z, f
        z = z_lo - f_lo * (z_hi - z_lo) / (f_hi - f_lo)
        if not z_lo < z < z_hi:
            z = 0.5 * (z_lo + z_hi)
            if not z_lo < z < z_hi:
                return z_lo, T.HIT, k, f_lo, at(z_lo), refine
    return inf, T.NOT_CONVERGED, max_iters, f, x, refine


def bits(a):
    """A float tensor as its bit pattern, so that comparisons treat NaNs and signed zeros as the values they are."""
    a = a.contiguous()
    return a.view(torch.int32 if a.dtype == torch.float32 else torch.int64)


def same(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all()) if a.is_floating_point() else torch.equal(a, b)


KEYS = ("depth", "status", "iters", "residual", "points")
