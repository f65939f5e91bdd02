"""GPU, kernel level through the C ABI: es_trace_surface (csrc/trace.hip) against the row rule of ``tracing.trace_surface`` (DESIGN.md
7j), against es_query_sdf_tiles -- the value a row saw, bit for bit -- and against the fp64 oracle.  Budgets come from the fp32 oracle's
own error and from the two caps checked on the CPU for the fp32 twin (tests/test_trace_host.py); every test prints the figures it
asserts on, and they go to trace_shapes.json in the log directory of test_gpu_backward.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import weightgen
from test_gpu_backward import LOG
from test_gpu_forward_shapes import _sampling_rays
from trace_util import CASES, EPS, ITERS_CAP, KEYS, N_RAYS, STATUS_CAP, case, same, sdf64

from endosurf_amd import tracing as T

pytestmark = pytest.mark.gpu

MARGIN = 4.0          # the device against the fp32 oracle's own error: the forward-parity precedent of test_gpu_track.py
INF = float("inf")
_REPORT, _DEVS = {}, {}


def _note(name, **values):
    _REPORT.setdefault(name, {}).update(values)
    os.makedirs(LOG, exist_ok=True)
    with open(os.path.join(LOG, "trace_shapes.json"), "w") as f:
        json.dump(_REPORT, f, indent=1, sort_keys=True)


class Dev:
    """Weights of one state on the device; the tracer and the tiled SDF query on them, inputs and results as host tensors."""
    def __init__(self, state):
        from endosurf_amd import _lib, params
        self._lib, self.lib = _lib, _lib.load()
        _lib.check(self.lib.es_init(), "es_init")
        flat = torch.from_numpy(params.flatten_state(state)).cuda()
        self.weff = torch.zeros(self.lib.es_weff_floats(), device="cuda")
        self.packed = torch.zeros(self.lib.es_packed_floats(), device="cuda")
        _lib.check(self.lib.es_weightnorm_pack(_lib.ptr(flat), _lib.ptr(self.weff), _lib.ptr(self.packed), 1, _lib.stream_ptr()))
        torch.cuda.synchronize()

    def trace(self, rays, use_deform, tau=0.0, eps=EPS, relax=1.0, min_step=1e-3, max_iters=128, tile_points=0, optional=True):
        n, ptr = rays.shape[0], self._lib.ptr
        r = rays.cuda().contiguous()
        out = {"depth": torch.full((n, 1), float("nan"), device="cuda"), "status": torch.full((n,), -7, device="cuda", dtype=torch.int32)}
        if optional:
            out.update(iters=torch.full((n,), -7, device="cuda", dtype=torch.int32), residual=torch.full((n,), float("nan"), device="cuda"),
                       points=torch.full((n, 3), float("nan"), device="cuda"))
        self._lib.check(self.lib.es_trace_surface(ptr(r), n, tau, eps, relax, min_step, max_iters, tile_points, ptr(self.packed), ptr(self.weff),
                                                  int(use_deform), ptr(out["depth"]), ptr(out["status"]), ptr(out.get("iters")),
                                                  ptr(out.get("residual")), ptr(out.get("points")), self._lib.stream_ptr()), "es_trace_surface")
        torch.cuda.synchronize()
        return {k: v.cpu() for k, v in out.items()}

    def query(self, x, t, use_deform, tile_points=32):
        p = self._lib.es_points()
        xd, td = x.cuda().contiguous(), t.reshape(-1).cuda().contiguous()
        p.x, p.t, p.mode, p.t_scalar, p.n_per_ray, p.ldz, p.M = self._lib.ptr(xd), self._lib.ptr(td), 0, 0, 1, 1, x.shape[0]
        out = torch.full((x.shape[0],), float("nan"), device="cuda")
        self._lib.check(self.lib.es_query_sdf_tiles(C.byref(p), self._lib.ptr(self.packed), self._lib.ptr(self.weff), self._lib.ptr(out),
                                                    int(use_deform), tile_points, self._lib.stream_ptr()), "es_query_sdf_tiles")
        torch.cuda.synchronize()
        return out.cpu()


def dev_for(mode, seed):
    if (mode, seed) not in _DEVS:
        _DEVS[(mode, seed)] = Dev(weightgen.make_state(seed, mode, True))
    return _DEVS[(mode, seed)]


@pytest.fixture(scope="module", params=[(m, s, d) for m, s in CASES for d in (True, False)], ids=lambda p: f"{p[0]}{p[1]}{'' if p[2] else '-static'}")
def tc(request):
    """One state with or without its deformation network: device weights, the oracles, the host twins and the device's result on the 515
    rays at the defaults."""
    mode, seed, use_deform = request.param
    c = dict(case(mode, seed, use_deform))
    c["dev"], c["use_deform"] = dev_for(mode, seed), use_deform
    c["full"] = c["dev"].trace(c["rays"], use_deform)
    return c


def host_points(rays, depth):
    """o + depth w in fp32, product by product."""
    o, d = rays[:, :3], rays[:, 3:6]
    w = d / (d[:, 2:] + 1e-6)
    return o + depth.reshape(-1, 1) * w


def e32_on(c, points, rays):
    """The fp32 oracle's worst error against the fp64 oracle at ``points``."""
    with torch.no_grad():
        s32 = c["net32"].sdf_observed(points, rays[:, 8:9])[:, 0]
    return float((s32.double() - sdf64(c, points, rays)).abs().max())


def assert_rule_outputs(out, cap=128, finite_points=True):
    """What the row rule says of any result, whatever the trajectory."""
    st, it, dep = out["status"], out["iters"], out["depth"][:, 0]
    assert bool(((st >= 1) & (st <= 4)).all()) and bool(((it >= 0) & (it <= cap)).all())
    assert bool(torch.isfinite(dep[st == T.HIT]).all()) and bool((dep[st == T.OCCUPIED] == 0).all())
    assert bool((dep[(st == T.MISS) | (st == T.NOT_CONVERGED)] == INF).all())
    assert bool((it[st == T.OCCUPIED] == 1).all()) and bool((it[st != T.MISS] >= 1).all())
    never = it == 0
    assert bool((out["points"][never] == 0).all()) and bool((out["residual"][never] == 0).all()) and bool((st[never] == T.MISS).all())
    assert not finite_points or bool(torch.isfinite(out["points"]).all())


def test_rows_do_not_depend_on_the_batch_or_the_tile(tc):
    """Prefixes of the 515 rays -- 1 row, the edges of the 32- and 64-row tiles, several workgroups -- and both tile heights: every output
    of a row as in the 515-ray run, bit for bit."""
    dev, rays, full, ud = tc["dev"], tc["rays"], tc["full"], tc["use_deform"]
    assert_rule_outputs(full)
    assert len(set(full["iters"].tolist())) > 4          # rows do need different numbers of evaluations
    for n in (1, 31, 32, 33, 63, 64, 65, N_RAYS):
        for tile in ((0,) if n < N_RAYS else (32, 64)):
            part = dev.trace(rays[:n], ud, tile_points=tile)
            for k in KEYS:
                assert same(part[k], full[k][:n]), (n, tile, k)
    for tile in (32, 64):
        part = dev.trace(rays[:65], ud, tile_points=tile)
        for k in KEYS:
            assert same(part[k], full[k][:65]), (tile, k)
    again = dev.trace(rays, ud)
    perm = torch.from_numpy(np.random.default_rng(3).permutation(N_RAYS).copy())
    shuffled = dev.trace(rays[perm], ud)
    for k in KEYS:
        assert same(again[k], full[k]) and same(shuffled[k], full[k][perm]), k


@pytest.mark.parametrize("tau", [0.0, 0.05])
def test_the_value_the_tracer_saw_and_the_contract(tc, tau):
    """residual + tau is es_query_sdf_tiles at ``points`` on 32-point tiles (and on 64-point tiles), bit for bit; a HIT's point is
    o + depth w; and, whatever the trajectory, the fp64 oracle at a HIT's point is within eps + 4 e32 of tau."""
    dev, rays, ud = tc["dev"], tc["rays"], tc["use_deform"]
    out = tc["full"] if tau == 0.0 else dev.trace(rays, ud, tau=tau)
    assert_rule_outputs(out)
    seen = out["iters"] >= 1
    q32, q64 = (dev.query(out["points"], rays[:, 8], ud, tile) for tile in (32, 64))
    assert same(q32, q64)
    want = q32 - torch.tensor(tau, dtype=torch.float32)          # the same fp32 subtraction (exact at tau = 0)
    off = seen & (out["residual"].view(torch.int32) != want.view(torch.int32))
    assert int(seen.sum()) >= N_RAYS - 8 and not bool(off.any()), (int(off.sum()), out["status"][off].tolist()[:8], out["residual"][off].tolist()[:4],
                                                                     want[off].tolist()[:4], q32[off].tolist()[:4])
    hit = out["status"] == T.HIT
    assert int(hit.sum()) >= 300
    assert bool((out["residual"][hit].abs() <= np.float32(EPS)).all())          # (no bracket ran out of interior at this eps)
    assert same(out["points"][hit], host_points(rays, out["depth"])[hit])
    e32 = e32_on(tc, out["points"][hit], rays[hit])
    worst = float((sdf64(tc, out["points"], rays)[hit] - tau).abs().max())
    print(f"\n[{tc['name']} tau {tau}] hits {int(hit.sum())}  |sdf64(points) - tau| max {worst:.3e}  bound eps + 4 e32 = {EPS + MARGIN * e32:.3e} (e32 {e32:.3e})")
    _note(f"{tc['name']}/tau{tau}", hits=int(hit.sum()), contract_worst=worst, contract_bound=EPS + MARGIN * e32, e32=e32)
    assert worst <= EPS + MARGIN * e32


def test_against_the_fp64_twin(tc):
    """The device's trajectory is the fp64 twin's under the two caps the fp32 oracle twin meets on the CPU; the depths of rows that hit in
    both are within 4 x the fp32 twin's own worst plus 2 eps, the width of the stopping interval at unit slope."""
    full, t64, t32 = tc["full"], tc["twin64"], tc["twin32"]
    d_status, d_iters = int((full["status"] != t64["status"]).sum()), int((full["iters"] != t64["iters"]).sum())
    both_twins = (t32["status"] == T.HIT) & (t64["status"] == T.HIT)
    yard = float((t32["depth"].double() - t64["depth"])[both_twins].abs().max())
    both = (full["status"] == T.HIT) & (t64["status"] == T.HIT)
    err = float((full["depth"].double() - t64["depth"])[both].abs().max())
    it = full["iters"].double()
    print(f"\n[{tc['name']}] status differs on {d_status} rows (cap {STATUS_CAP}), iters on {d_iters} (cap {ITERS_CAP}); |depth - fp64 twin| max {err:.3e} "
          f"(bound {MARGIN * yard + 2 * EPS:.3e}: fp32 twin {yard:.3e}); evaluations per ray mean {float(it.mean()):.2f} max {int(it.max())}")
    _note(tc["name"], status_differs=d_status, iters_differ=d_iters, depth_err=err, depth_bound=MARGIN * yard + 2 * EPS, depth_fp32_twin=yard,
          iters_mean=float(it.mean()), iters_max=int(it.max()), hits=int((full["status"] == T.HIT).sum()))
    assert d_status <= STATUS_CAP and d_iters <= ITERS_CAP
    assert err <= MARGIN * yard + 2 * EPS


@pytest.mark.parametrize("cap", [1, 3])
def test_the_cap(tc, cap):
    """The trajectory does not know the cap: a row that needs at most ``cap`` evaluations comes out as in the full run, every other row
    is NOT_CONVERGED after ``cap`` evaluations with depth inf."""
    dev, rays, full, ud = tc["dev"], tc["rays"], tc["full"], tc["use_deform"]
    out = dev.trace(rays, ud, max_iters=cap)
    assert_rule_outputs(out, cap)
    done = full["iters"] <= cap
    assert int(done.sum()) < N_RAYS
    for k in KEYS:
        assert same(out[k][done], full[k][done]), k
    assert bool((out["status"][~done] == T.NOT_CONVERGED).all()) and bool((out["iters"][~done] == cap).all())
    assert same(out["residual"][~done], dev.query(out["points"], rays[:, 8], ud)[~done])
    if cap == 1:          # the statuses of the first evaluation, from the value itself
        st, res = out["status"], out["residual"]
        one = out["iters"] == 1
        assert bool((res[one & (st == T.HIT)].abs() <= np.float32(EPS)).all()) and bool((res[st == T.OCCUPIED] < -np.float32(EPS)).all())
        assert bool((res[one & ((st == T.NOT_CONVERGED) | (st == T.MISS))] > np.float32(EPS)).all())


def test_eps_zero_stops_on_its_own(tc):
    """eps = 0: a row ends by an exact zero, by a bracket without interior (reported at its low end, where the value is positive) or at
    the cap; the value it reports is still the query's, and the point is on the surface to the precision of the evaluation."""
    dev, rays, ud = tc["dev"], tc["rays"], tc["use_deform"]
    out = dev.trace(rays, ud, eps=0.0)
    assert_rule_outputs(out)
    hit, seen = out["status"] == T.HIT, out["iters"] >= 1
    assert same(out["residual"][seen], dev.query(out["points"], rays[:, 8], ud)[seen])
    assert bool((out["residual"][hit] >= 0).all()) and int(hit.sum()) >= 250
    assert same(out["points"][hit], host_points(rays, out["depth"])[hit])
    e32 = e32_on(tc, out["points"][hit], rays[hit])
    # a bracket without interior: the value changes sign between two neighbouring depths, so the exact field at the low end is within
    # the evaluation's error (4 e32, as above) of a value whose own size is at most that error plus the field's change over one ulp of z
    worst, res = float(sdf64(tc, out["points"], rays)[hit].abs().max()), float(out["residual"][hit].max())
    print(f"\n[{tc['name']} eps 0] hits {int(hit.sum())} NOT_CONVERGED {int((out['status'] == T.NOT_CONVERGED).sum())}  residual max {res:.3e}  "
          f"|sdf64(points)| max {worst:.3e} (e32 {e32:.3e})  iters max {int(out['iters'].max())}")
    _note(f"{tc['name']}/eps0", hits=int(hit.sum()), residual_max=res, sdf64_max=worst, e32=e32, iters_max=int(out["iters"].max()))
    assert float((sdf64(tc, out["points"], rays) - out["residual"].double())[hit].abs().max()) <= MARGIN * e32


def test_special_rays_and_rows_that_are_not_finite():
    """An origin inside the sphere, a ray that misses it, a camera looking back.  Then three bad rows between valid ones, whose
    neighbours keep their bits: a ray of nine NaNs (``far > near`` is false: MISS without an evaluation, by the rule's first line); a ray
    with d.z = -1e-6, whose w = d / (d.z + 1e-6) is infinite while near and far are not -- its first point and value are not finite:
    NOT_CONVERGED after one evaluation, depth inf; and a ray whose time is NaN: the deformation network's ReLUs (v_max_f32) drop a NaN, in
    the tracer as in es_query_sdf, so the row sees the finite value the query returns for that point and time, bit for bit."""
    mode, seed = CASES[0]
    dev = dev_for(mode, seed)
    rays, _ = _sampling_rays()
    base = dev.trace(rays, True)
    assert_rule_outputs(base)
    o_inside = dev.query(rays[30:31, :3].contiguous(), rays[30:31, 8], True)
    print(f"\nspecial rays: status {base['status'][30:].tolist()} iters {base['iters'][30:].tolist()} depth {base['depth'][30:, 0].tolist()} "
          f"(sdf at the inside origin {float(o_inside):.4f})")
    assert same(base["points"][30], rays[30, :3]) and same(base["residual"][30:31], o_inside)          # near clamps to 0: the origin itself
    if float(o_inside) < -EPS:
        assert int(base["status"][30]) == T.OCCUPIED and float(base["depth"][30]) == 0.0
    assert int(base["status"][31]) == T.MISS and int(base["iters"][31]) == 0 and float(base["depth"][31]) == INF
    assert int(base["iters"][32]) >= 1          # d.z < 0: w still points to +z (the reference's convention), the row runs and stops
    head = dev.trace(rays[:30], True)
    for k in KEYS:
        assert same(base[k][:30], head[k]), k
    bad = rays.clone()
    bad[5, 8] = float("nan")
    bad[12, :] = float("nan")
    bad[20, :6] = torch.tensor([-1.5, 0.1, 0.0, 1.0, 0.05, -1e-6])
    assert float(bad[20, 5] + np.float32(1e-6)) == 0.0
    out = dev.trace(bad, True)
    assert_rule_outputs(out, finite_points=False)
    keep = torch.ones(33, dtype=torch.bool)
    keep[[5, 12, 20]] = False
    for k in KEYS:
        assert same(out[k][keep], base[k][keep]), k
    assert bool(torch.isfinite(out["points"][keep]).all())
    assert int(out["status"][12]) == T.MISS and int(out["iters"][12]) == 0 and float(out["depth"][12]) == INF
    assert int(out["status"][20]) == T.NOT_CONVERGED and int(out["iters"][20]) == 1 and float(out["depth"][20]) == INF
    assert not bool(torch.isfinite(out["residual"][20])) and not bool(torch.isfinite(out["points"][20]).any())
    seen5 = dev.query(out["points"][5:6], bad[5:6, 8], True)
    print(f"bad rows: status {out['status'][[5, 12, 20]].tolist()} iters {out['iters'][[5, 12, 20]].tolist()}; the NaN-time row's value {float(seen5):.3e}")
    assert bool(torch.isfinite(seen5).all()) and same(out["residual"][5:6], seen5) and bool(torch.isfinite(out["points"][5]).all())
    # the static field does not read the time at all
    static, static_bad = dev.trace(rays, False), dev.trace(bad, False)
    for k in KEYS:
        assert same(static_bad[k][5], static[k][5]), k


def test_empty_batches_null_outputs_and_refusals():
    """N = 0 is status 0 without a launch; the three optional outputs may be null; each bad argument is status 1 with its name in
    es_last_error() before anything is launched (the addresses are host numpy's and never dereferenced)."""
    from endosurf_amd import _lib
    lib = _lib.load()
    mode, seed = CASES[0]
    dev = dev_for(mode, seed)
    rays = case(mode, seed, True)["rays"][:70]
    full, lean = dev.trace(rays, True), dev.trace(rays, True, optional=False)
    assert sorted(lean) == ["depth", "status"] and same(lean["depth"], full["depth"]) and same(lean["status"], full["status"])
    buf = np.zeros(64, np.float32)
    b = buf.ctypes.data

    def call(N=4, tau=0.0, eps=1e-5, relax=1.0, min_step=1e-3, max_iters=128, tile_points=0, rays=b, packed=b, depth=b, status=b):
        return lib.es_trace_surface(rays, N, tau, eps, relax, min_step, max_iters, tile_points, packed, b, 1, depth, status, None, None, None, None)

    assert call(N=0, rays=None, packed=None, depth=None, status=None) == 0
    bad = [("N", dict(N=-1)), ("tau", dict(tau=float("nan"))), ("tau", dict(tau=float("inf"))), ("eps", dict(eps=-1e-9)),
           ("eps", dict(eps=float("inf"))), ("eps", dict(eps=float("nan"))), ("relax", dict(relax=0.0)), ("relax", dict(relax=1.5)),
           ("relax", dict(relax=float("nan"))), ("min_step", dict(min_step=0.0)), ("min_step", dict(min_step=float("inf"))),
           ("min_step", dict(min_step=float("nan"))), ("max_iters", dict(max_iters=0)), ("max_iters", dict(max_iters=1025)),
           ("tile_points", dict(tile_points=16)), ("null buffer", dict(rays=None)), ("null buffer", dict(packed=None)),
           ("null buffer", dict(depth=None)), ("null buffer", dict(status=None))]
    for name, kw in bad:
        assert call(**kw) == 1 and name.encode() in lib.es_last_error(), (name, kw, lib.es_last_error())
        if name != "N":          # the arguments are checked before N == 0 returns; the buffers only when N > 0 needs them
            assert call(N=0, **kw) == (0 if name == "null buffer" else 1)
