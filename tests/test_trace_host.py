"""CPU: ``tracing.trace_surface``, the host specification and twin of the surface tracer -- on analytic fields in fp64
against closed forms and against a scalar restatement of the row rule, and on the fp64 / fp32 oracles of the test weights.  Every test
prints the figures it asserts on."""
import math

import numpy as np
import pytest
import torch

import weightgen
from trace_util import CASES, EPS, ITERS_CAP, KEYS, N_RAYS, STATUS_CAP, case, marching64, same, sdf64, sqrt64, trace_scalar

from endosurf_amd import tracing as T

RADIUS = 0.5


def sphere(scale=1.0, radius=RADIUS):
    """scale (|x| - radius) as a torch field and as the same operations on Python floats."""
    def torch_fn(x, t):
        return (scale * (torch.sqrt(x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2]) - radius))[:, None]

    def float_fn(x0, x1, x2, t):
        return scale * (sqrt64(x0 * x0 + x1 * x1 + x2 * x2) - radius)
    return torch_fn, float_fn


def rays64():
    return torch.from_numpy(weightgen.make_rays(91, 64)).double()


def closed_form(rays, radius=RADIUS):
    """Per ray against the sphere |x| = radius along o + z w: (meets [N] bool, z_first [N], chord [N] in z, slope [N] = |d|x|/dz| there)."""
    o, w, s, near, far, t = T.ray_geometry(rays)
    a, b, c = (w * w).sum(-1), 2.0 * (o * w).sum(-1), (o * o).sum(-1) - radius * radius
    disc = b * b - 4.0 * a * c
    root = torch.sqrt(disc.clamp(min=0.0))
    z0, z1 = (-b - root) / (2.0 * a), (-b + root) / (2.0 * a)
    x = o + z0[:, None] * w
    slope = ((x * w).sum(-1) / x.norm(dim=-1)).abs()
    return disc > 0, z0, z1 - z0, slope


def assert_twin_is_the_rule(field, rays, **args):
    """``trace_surface`` on the batch against ``trace_scalar`` ray by ray: every output, exactly (fp64).  Returns (twin, entered_refine)."""
    torch_fn, float_fn = field
    out = T.trace_surface(torch_fn, rays, **args)
    refine = []
    for i in range(rays.shape[0]):
        depth, status, iters, res, p, ref = trace_scalar(float_fn, rays[i].tolist(), **args)
        got = (float(out["depth"][i, 0]), int(out["status"][i]), int(out["iters"][i]), float(out["residual"][i]), tuple(out["points"][i].tolist()))
        want = (depth, status, iters, res, p)
        assert got == want or (math.isnan(res) and got[:3] == want[:3] and math.isnan(got[3]) and got[4] == want[4]), (i, got, want)
        refine.append(ref)
    assert out["depth"].shape == (rays.shape[0], 1) and out["status"].dtype == torch.int32 and out["iters"].dtype == torch.int32
    return out, torch.tensor(refine)


# min_step below eps / s (s = |w| < 1.2 on these rays): a marching step is then always the field's own value, which cannot overshoot a
# field of unit gradient, so the phase REFINE is never needed; at the default min_step = 1e-3 a row whose value lies between eps and
# 1e-3 s takes the minimum step and may cross the surface by it.
NO_OVERSHOOT = dict(min_step=1e-6)


def test_unit_gradient_sphere_against_the_closed_form():
    rays = rays64()
    meets, z_first, chord, slope = closed_form(rays)
    out, refine = assert_twin_is_the_rule(sphere(), rays, **NO_OVERSHOOT)
    hit = out["status"] == T.HIT
    assert int(meets.sum()) >= 20 and int((~meets).sum()) >= 5, int(meets.sum())          # the camera sees the sphere and past it
    assert torch.equal(hit, meets)
    assert bool((out["status"][~meets] == T.MISS).all())
    err = (out["depth"][:, 0] - z_first)[hit].abs()
    bound = EPS / slope[hit] + 1e-12
    print(f"\nunit sphere: {int(hit.sum())} hits, |depth - closed form| max {float(err.max()):.3e} (bound eps / cos, worst ratio "
          f"{float((err / bound).max()):.3f}), iters max {int(out['iters'][hit].max())}, entered REFINE {int(refine.sum())}")
    assert bool((err <= bound).all())
    assert not bool(refine.any())
    assert bool((out["residual"][hit].abs() <= EPS).all()) and bool((out["residual"][hit] >= 0).all())          # approached from outside


def test_a_field_that_overshoots_goes_through_refine():
    """2.5 (|x| - 0.5) with relax = 0.6: a marching step is 1.5 times the distance to the sphere, so it crosses the surface wherever the
    ray meets it steeper than cos = 2/3, and the minimum step crosses it elsewhere -- but no step crosses the whole chord.  With b the
    ray's distance from the centre, h = sqrt(0.25 - b^2) half its chord and v the distance along the ray to the chord's middle, a step
    from v jumps the chord iff  1.5 (sqrt(b^2 + v^2) - 0.5) > v + h.  The left side is convex in v; at v = h (on the surface) it is
    0 <= 2 h, at v = sqrt(1 - b^2) (where the ray enters the unit sphere and starts) it is 0.75 <= 0.866 <= v + h; so it holds nowhere
    between.  The minimum step, 1e-3 s in space with s < 1.2, jumps no chord longer than that: the rays of this test have none shorter
    (asserted).  Hence the hits are the rays that meet the sphere, and each is found in a bracket: through REFINE, on the first crossing.
    At relax = 1 a step is 2.5 times the distance and rays with short chords are jumped: those hits are a subset."""
    rays = rays64()
    meets, z_first, chord, slope = closed_form(rays)
    assert not bool((meets & (chord <= 2 * 1.2e-3)).any())
    out, refine = assert_twin_is_the_rule(sphere(scale=2.5), rays, relax=0.6)
    hit = out["status"] == T.HIT
    err = (out["depth"][:, 0] - z_first)[hit].abs()
    print(f"\n2.5 x sphere, relax 0.6: {int(hit.sum())} hits of {int(meets.sum())} rays that meet it, through REFINE {int(refine[hit].sum())}, "
          f"|residual| max {float(out['residual'][hit].abs().max()):.3e}, |depth - closed form| max {float(err.max()):.3e}, iters max "
          f"{int(out['iters'][hit].max())}")
    assert torch.equal(hit, meets)
    assert bool(refine[hit].all())
    assert bool((out["residual"][hit].abs() <= EPS).all())
    # a residual of eps where the field's slope along the ray is 2.5 cos (1 % for the slope's change within eps of the surface)
    assert bool((err <= 1.01 * EPS / (2.5 * slope[hit]) + 1e-12).all())
    full, refine1 = assert_twin_is_the_rule(sphere(scale=2.5), rays)
    hit1 = full["status"] == T.HIT
    print(f"relax 1: {int(hit1.sum())} hits, through REFINE {int(refine1[hit1].sum())}")
    assert bool((meets[hit1]).all()) and int(hit1.sum()) >= 10 and bool(refine1[hit1].all())
    assert bool(((full["depth"][:, 0] - z_first)[hit1].abs() <= 1.01 * EPS / (2.5 * slope[hit1]) + 1e-12).all())


def test_special_rays():
    f = sphere()
    inside = [0.0, 0.0, -0.2, 0.0, 0.0, 1.0, 0.0, 0.0, 0.3]
    past = [0.0, 3.0, -1.5, 0.0, 0.0, 1.0, 0.0, 0.0, 0.3]              # misses the unit sphere
    graze = [RADIUS + 1e-4, 0.0, -1.5, 0.0, 0.0, 1.0, 0.0, 0.0, 0.3]    # passes the surface at a distance of 1e-4
    head_on = [0.0, 0.0, -1.5, 0.0, 0.0, 1.0, 0.0, 0.0, 0.3]
    rays = torch.tensor([inside, past, graze, head_on], dtype=torch.float64)
    out, _ = assert_twin_is_the_rule(f, rays)
    print(f"\nspecial rays: status {out['status'].tolist()} iters {out['iters'].tolist()} depth {out['depth'][:, 0].tolist()}")
    assert int(out["status"][0]) == T.OCCUPIED and float(out["depth"][0]) == 0.0 and int(out["iters"][0]) == 1
    assert int(out["status"][1]) == T.MISS and int(out["iters"][1]) == 0 and float(out["depth"][1]) == float("inf")
    assert bool((out["points"][1] == 0).all()) and float(out["residual"][1]) == 0.0
    assert int(out["status"][2]) in (T.MISS, T.HIT) and 1 <= int(out["iters"][2]) <= 128
    assert int(out["status"][2]) == T.MISS          # 1e-4 > eps: the surface is never within eps
    assert int(out["status"][3]) == T.HIT and abs(float(out["depth"][3]) - 1.0 / (1.0 / (1.0 + 1e-6))) <= 2 * EPS


def test_a_row_of_nans_stops_alone():
    torch_fn, float_fn = sphere(scale=2.5)
    rays = rays64()
    rays[3, 8] = 0.75          # the marked row's time
    bad_t = lambda x, t: torch.where(t == 0.75, torch.full_like(t, float("nan")), torch_fn(x, t))
    bad_f = lambda x0, x1, x2, t: float("nan") if t == 0.75 else float_fn(x0, x1, x2, t)
    clean = T.trace_surface(torch_fn, rays)
    out, _ = assert_twin_is_the_rule((bad_t, bad_f), rays)
    assert int(clean["status"][3]) == T.HIT
    assert int(out["status"][3]) == T.NOT_CONVERGED and int(out["iters"][3]) == 1 and float(out["depth"][3]) == float("inf")
    assert math.isnan(float(out["residual"][3])) and bool(torch.isfinite(out["points"][3]).all())
    keep = torch.arange(64) != 3
    for k in KEYS:
        assert same(out[k][keep], clean[k][keep]), k
    # an infinite value likewise
    inf_t = lambda x, t: torch.where(t == 0.75, torch.full_like(t, float("inf")), torch_fn(x, t))
    assert int(T.trace_surface(inf_t, rays)["status"][3]) == T.NOT_CONVERGED


@pytest.mark.parametrize("args", [dict(max_iters=1), dict(max_iters=3), dict(eps=0.0), dict(eps=0.0, max_iters=40), dict(tau=0.05),
                                  dict(relax=0.5), dict(min_step=0.02)], ids=lambda a: ",".join(f"{k}={v}" for k, v in a.items()))
@pytest.mark.parametrize("scale", [1.0, 2.5])
def test_caps_and_arguments_follow_the_rule(args, scale):
    rays = rays64()
    out, refine = assert_twin_is_the_rule(sphere(scale=scale), rays, **args)
    cap = args.get("max_iters", 128)
    st, it = out["status"], out["iters"]
    print(f"\nscale {scale} {args}: status counts {torch.bincount(st, minlength=5).tolist()[1:]} iters max {int(it.max())}")
    assert bool((it <= cap).all()) and bool(((st >= 1) & (st <= 4)).all())
    assert bool((it[st == T.NOT_CONVERGED] == cap).all())          # a finite field stops such a row at the cap only
    dep = out["depth"][:, 0]
    assert bool(torch.isfinite(dep[st == T.HIT]).all()) and bool((dep[st == T.OCCUPIED] == 0).all())
    assert bool((dep[(st == T.MISS) | (st == T.NOT_CONVERGED)] == float("inf")).all())
    if "max_iters" in args and "eps" not in args:
        assert int((st == T.NOT_CONVERGED).sum()) > 0          # the cap does bite
    if args.get("eps") == 0.0:
        # no row can stop by |f| <= 0 short of an exact zero: a hit is an exhausted bracket, reported at its low end, outside the surface
        hit = st == T.HIT
        assert bool((out["residual"][hit] >= 0).all())
        if cap == 128 and scale == 2.5:
            assert int(hit.sum()) > 0
    if "tau" in args:
        # the level set tau of scale (|x| - R) is the sphere of radius R + tau / scale; at scale 2.5 and relax 1 short chords are jumped
        meets, z_first, chord, slope = closed_form(rays, RADIUS + args["tau"] / scale)
        hit = st == T.HIT
        assert not bool((meets & (chord <= 2 * 1.2e-3)).any())
        assert torch.equal(hit, meets) if scale == 1.0 else bool(meets[hit].all()) and int(hit.sum()) >= 10
        assert bool(((dep - z_first)[hit].abs() <= 1.01 * EPS / (scale * slope[hit]) + 1e-12).all())


def test_argument_refusals():
    f, rays = sphere()[0], rays64()
    bad = [("tau", float("nan")), ("tau", float("inf")), ("eps", -1e-9), ("eps", float("inf")), ("eps", float("nan")), ("relax", 0.0),
           ("relax", 1.0001), ("relax", float("nan")), ("min_step", 0.0), ("min_step", -1.0), ("min_step", float("inf")),
           ("min_step", float("nan")), ("max_iters", 0), ("max_iters", 1025), ("max_iters", 2.5)]
    for name, value in bad:
        with pytest.raises(ValueError, match=name):
            T.trace_surface(f, rays, **{name: value})
        with pytest.raises(ValueError, match=name):
            T.check_trace_args(**{name: value})
    assert T.check_trace_args(0.05, 0.0, 1.0, 1e-3, 1024) == (0.05, 0.0, 1.0, 1e-3, 1024)
    with pytest.raises(ValueError, match="rays"):
        T.trace_surface(f, rays[:, :8])
    assert (T.HIT, T.MISS, T.OCCUPIED, T.NOT_CONVERGED) == (1, 2, 3, 4)
    empty = T.trace_surface(f, rays[:0])
    assert empty["depth"].shape == (0, 1) and empty["points"].shape == (0, 3) and empty["status"].numel() == 0


def test_any_float_dtype_and_row_independence():
    f, rays = sphere(scale=2.5)[0], rays64()
    full = T.trace_surface(f, rays)
    perm = torch.from_numpy(np.random.default_rng(5).permutation(64).copy())
    shuffled = T.trace_surface(f, rays[perm])
    for k in KEYS:
        assert same(full[k][perm], shuffled[k]) and same(full[k][9:10], T.trace_surface(f, rays[9:10])[k]), k
    out32 = T.trace_surface(f, rays.float())
    assert out32["depth"].dtype == torch.float32 and out32["points"].dtype == torch.float32 and out32["residual"].dtype == torch.float32
    assert torch.equal(out32["status"], full["status"])
    assert float((out32["depth"].double() - full["depth"])[full["status"] == T.HIT].abs().max()) <= 2 * EPS


# ---- the oracle's fields ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_deform", [True, False], ids=["deform", "static"])
@pytest.mark.parametrize("mode,seed", CASES, ids=lambda v: str(v))
def test_oracle_fields(mode, seed, use_deform):
    c = case(mode, seed, use_deform)
    rays, t64, t32 = c["rays"], c["twin64"], c["twin32"]
    hit = t64["status"] == T.HIT
    res = sdf64(c, t64["points"], rays).abs()
    march = marching64(mode, seed, use_deform)
    march_hit = torch.isfinite(march) & (march != 0)
    differ = int((hit != march_hit).sum())
    lost = int((t64["status"] == T.NOT_CONVERGED).sum())
    o, w, _, _, _, _ = T.ray_geometry(rays.double())
    at_march = sdf64(c, o + torch.where(march_hit, march, torch.zeros_like(march))[:, None] * w, rays).abs()[march_hit]
    d_status, d_iters = int((t32["status"] != t64["status"]).sum()), int((t32["iters"] != t64["iters"]).sum())
    it = t64["iters"].double()
    print(f"\n[{c['name']}] hits {int(hit.sum())}/{N_RAYS}  |sdf| at hits max {float(res[hit].max()):.3e}  HIT != ray_marching's hit on {differ} rays  "
          f"NOT_CONVERGED {lost}  evaluations per ray mean {float(it.mean()):.2f} max {int(it.max())}  |sdf| at ray_marching's depth: median "
          f"{float(at_march.median()):.3e} max {float(at_march.max()):.3e}  fp32 twin: status differs on {d_status} rows, iters on {d_iters}")
    assert int(hit.sum()) >= 300
    assert bool((res[hit] <= EPS).all())
    # the residual is the field at the reported point (up to the fp64 GEMM's dependence on the batch it runs in)
    assert float((t64["residual"] - sdf64(c, t64["points"], rays))[hit].abs().max()) <= 1e-12
    assert differ <= 8 and lost <= 4
    if mode == "trained":
        assert float(at_march.median()) > 100 * EPS          # the finding: ray_marching's depth is not on the surface
    assert d_status <= STATUS_CAP and d_iters <= ITERS_CAP
    assert float(it.mean()) < 136 / 4          # against ray_marching's 136 evaluations per ray
