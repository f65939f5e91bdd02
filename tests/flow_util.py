"""Shared by the pixel-track tests: the synthetic camera of ``weightgen.make_rays``, the three kinds of segments built on
the tracer's cases, the host twin's results on them (computed once per process), a second, scalar restatement of the segment rule in
Python floats, and the cycle-consistency measurement."""
import functools
import math

import numpy as np
import torch

import weightgen
from trace_util import case, sdf_fn, sqrt64
from track_util import deform_fn

from endosurf_amd import flow as FL
from endosurf_amd import tracing as T

# The camera of weightgen.make_rays: 640 x 512, f = 800, principal point (319.5, 255.5), at (0, 0, -1.5) looking along +z.
HEIGHT, WIDTH = 512, 640
K = np.array([[800.0, 0.0, 319.5], [0.0, 800.0, 255.5], [0.0, 0.0, 1.0]])
POSE = np.eye(4)
POSE[:3, 3] = (0.0, 0.0, -1.5)
MARGIN = 5e-3
KINDS = ("hit", "past", "mid")
PAST = 0.05


def rotated_pose(angle=0.1, shift=0.2):
    """The second target camera of the tests: POSE rotated by ``angle`` rad about y and shifted by ``shift`` along x."""
    c, s = math.cos(angle), math.sin(angle)
    P = POSE.copy()
    P[:3, :3] = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
    P[0, 3] += shift
    return P


def segments(c):
    """(a [N,3], {kind: b [N,3]}, t [N], hit [N] bool) in fp64 for a case of ``trace_util``: from each ray's origin (a) to the fp64
    twin's traced point, (b) to the point 0.05 past it along the ray, (c) to the midpoint.  Rows whose ray did not HIT keep the point
    the tracer reports for them (the last one it evaluated, or 0): segments like any other, of which the tests assert nothing but
    that the twins agree on them."""
    rays = c["rays"].double()
    a, d, t = rays[:, :3].contiguous(), rays[:, 3:6], rays[:, 8].contiguous()
    p = c["twin64"]["points"]
    return a, {"hit": p, "past": p + PAST * d, "mid": 0.5 * (a + p)}, t, c["twin64"]["status"] == T.HIT


@functools.lru_cache(maxsize=None)
def visible_case(mode, seed, use_deform):
    """Per kind of segment: the host twin in fp64 and in fp32 (the fp32 oracle on the fp32-rounded segments) at the defaults."""
    c = case(mode, seed, use_deform)
    a, ends, t, hit = segments(c)
    out = {"a": a, "t": t, "hit": hit, "ends": ends, "name": c["name"], "case": c}
    for kind in KINDS:
        out[kind, 64] = FL.segment_visible(sdf_fn(c["net64"]), a, ends[kind], t)
        out[kind, 32] = FL.segment_visible(sdf_fn(c["net32"]), a.float(), ends[kind].float(), t.float())
    return out


def visible_scalar(field, a, b, t, margin=5e-3, tau=0.0, relax=1.0, min_step=1e-3, max_iters=128):
    """The segment rule of DESIGN.md 7o for ONE row, in Python floats (IEEE double, one operation at a time): a second restatement,
    written from the rule and sharing no code with ``flow.segment_visible``.  ``field(x0, x1, x2, t) -> float``.  Returns (status,
    iters, blocker, clearance, free_to)."""
    inf = float("inf")
    a, b, t = [float(v) for v in a], [float(v) for v in b], float(t)
    if not all(math.isfinite(v) for v in a + b + [t]):
        return 3, 0, inf, inf, -inf
    d = [b[i] - a[i] for i in range(3)]
    dot = lambda p, q: p[0] * q[0] + p[1] * q[1] + p[2] * q[2]
    L = sqrt64(dot(d, d))
    if not L > 0:
        return 3, 0, inf, inf, -inf
    u = [d[i] / L for i in range(3)]
    uu = dot(u, u)
    d1 = -dot(u, a) / uu
    p = [a[i] + d1 * u[i] for i in range(3)]
    d2 = sqrt64(max(1.0 - dot(p, p), 0.0)) / sqrt64(uu)
    s_in, s_out = max(d1 - d2, 0.0), d1 + d2
    s_end = L - margin if L - margin < s_out else s_out
    if not s_end > s_in:
        return 1, 0, inf, inf, -inf
    s, last, clearance, free_to = s_in, False, inf, -inf
    for k in range(1, max_iters + 1):
        f = field(a[0] + s * u[0], a[1] + s * u[1], a[2] + s * u[2], t) - tau
        if f < clearance:
            clearance = f
        if not math.isfinite(f):
            return 3, k, inf, clearance, free_to
        if f <= 0:
            return 2, k, s, clearance, free_to
        free_to = s
        if last:
            return 1, k, inf, clearance, free_to
        s = s + max(relax * f, min_step)
        if s >= s_end:
            s, last = s_end, True
    return 3, max_iters, inf, clearance, free_to


class Recorded:
    """A torch field that remembers every value it returned, and the same field point by point on Python floats: the value recorded
    for that point and time, else a one-row evaluation.  Two restatements of one rule then see the same numbers, whatever the batch a
    GEMM ran in."""
    def __init__(self, fn, dtype=torch.float64):
        self.fn, self.dtype, self.seen, self.misses = fn, dtype, {}, 0

    def torch_fn(self, x, t):
        v = self.fn(x, t)
        for row, tt, val in zip(x.tolist(), t.reshape(-1).tolist(), v.reshape(-1).tolist()):
            self.seen[(*row, tt)] = val
        return v

    def float_fn(self, x0, x1, x2, t):
        key = (x0, x1, x2, t)
        if key not in self.seen:
            self.misses += 1
            self.seen[key] = float(self.fn(torch.tensor([[x0, x1, x2]], dtype=self.dtype), torch.tensor([[t]], dtype=self.dtype)))
        return self.seen[key]


def cycle_error(track, pixels, t_a, t_b, height=HEIGHT, width=WIDTH):
    """Pixels tracked a -> b -> a in one camera: ``track(pixels [P,2], t_from, times [1]) -> track_pixels' dict``.  Returns (the return
    error in pixels [P], rows valid both ways [P] bool)."""
    there = track(pixels, t_a, [t_b])
    back = track(there["pixels"][0], t_b, [t_a])
    both = there["valid"][0] & back["valid"][0]
    e = back["pixels"][0].double() - torch.as_tensor(pixels).double().to(back["pixels"].device)
    return torch.sqrt((e * e).sum(-1)), both


def oracle_fns(c, bits):
    net = c["net64"] if bits == 64 else c["net32"]
    return sdf_fn(net), (deform_fn(net) if net.use_deform else None)


CYCLE_T = (0.3, 0.6)


def cycle_pixels():
    """The 97 pixels of the cycle-consistency measurement, fp64 [97,2]."""
    rng = np.random.default_rng(97)
    return torch.from_numpy(np.stack([rng.uniform(0, WIDTH - 1, 97), rng.uniform(0, HEIGHT - 1, 97)], -1))


@functools.lru_cache(maxsize=None)
def twin_cycle(bits):
    """(worst return error in pixels over rows valid both ways, their number) of the host twin on the trained weights, seed 11, in
    fp64 (tol 1e-6) or on the fp32 oracle (tol 1e-5, the device's default), eps 1e-5, t = 0.3 -> 0.6 -> 0.3 in the one camera."""
    c = case("trained", 11, True)
    dt = torch.float64 if bits == 64 else torch.float32
    sdf, dfm = oracle_fns(c, bits)
    args = dict(trace_args=dict(eps=1e-5), track_args=dict(tol=1e-6 if bits == 64 else 1e-5))
    track = lambda p, t_from, times: FL.track_pixels(sdf, dfm, torch.as_tensor(p, dtype=dt), K, POSE, t_from, times, HEIGHT, WIDTH, **args)
    err, both = cycle_error(track, cycle_pixels().to(dt), *CYCLE_T)
    return float(err[both].max()), int(both.sum())
