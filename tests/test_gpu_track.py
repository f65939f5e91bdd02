"""GPU, kernel level through the C ABI: es_deform_forward / es_deform_inverse (csrc/deform.hip) against the fp64 oracle and against
the row rule of ``tracking.inverse_deform``.  Budgets come from the fp32 oracle's own error and from the contraction
bound rho < 0.75 asserted on each case's points; every test prints the figures it asserts on."""
import ctypes as C

import numpy as np
import pytest
import torch

import weightgen
from track_util import (CASES, FLT_MAX, TOL, assert_contraction, budget, deform_fn, draw, fixed_point64, oracle_net, rownorm)

from endosurf_amd import tracking

pytestmark = pytest.mark.gpu

M = 200


class Dev:
    """Weights of one state on the device and the two deformation entries on them, inputs and results as host tensors."""
    def __init__(self, state):
        from endosurf_amd import _lib, params
        self._lib, self.lib = _lib, _lib.load()
        _lib.check(self.lib.es_init(), "es_init")
        flat = torch.from_numpy(params.flatten_state(state)).cuda()
        self.weff = torch.zeros(self.lib.es_weff_floats(), device="cuda")
        self.packed = torch.zeros(self.lib.es_packed_floats(), device="cuda")
        _lib.check(self.lib.es_weightnorm_pack(_lib.ptr(flat), _lib.ptr(self.weff), _lib.ptr(self.packed), 1, _lib.stream_ptr()))
        torch.cuda.synchronize()

    def _pts(self, x, t):
        p = self._lib.es_points()
        xd, td = x.cuda().contiguous(), t.reshape(-1).cuda().contiguous()
        p.x, p.t, p.mode, p.n_per_ray, p.ldz, p.M = self._lib.ptr(xd), self._lib.ptr(td), 0, 1, 1, x.shape[0]
        p.t_scalar = 1 if td.numel() == 1 and x.shape[0] != 1 else 0
        assert td.numel() in (1, x.shape[0])
        p._keep = (xd, td)
        return p

    def forward(self, x, t):
        """(x + D, D) at fp32 host points; ``t`` [M] or [1] (read as t_scalar)."""
        n = x.shape[0]
        xc, d = (torch.full((n, 3), float("nan"), device="cuda") for _ in range(2))
        p, ptr = self._pts(x, t), self._lib.ptr
        self._lib.check(self.lib.es_deform_forward(C.byref(p), ptr(self.packed), ptr(self.weff), ptr(xc), ptr(d), self._lib.stream_ptr()),
                        "es_deform_forward")
        torch.cuda.synchronize()
        return xc.cpu(), d.cpu()

    def inverse(self, c, t, init=None, max_iters=64, tol=TOL):
        n = c.shape[0]
        y, step = torch.full((n, 3), float("nan"), device="cuda"), torch.full((n,), float("nan"), device="cuda")
        iters = torch.full((n,), -1, device="cuda", dtype=torch.int32)
        p, ptr = self._pts(c, t), self._lib.ptr
        ini = None if init is None else init.cuda().contiguous()
        self._lib.check(self.lib.es_deform_inverse(C.byref(p), ptr(ini), ptr(self.packed), ptr(self.weff), int(max_iters), float(tol), ptr(y), ptr(step),
                                                   ptr(iters), self._lib.stream_ptr()), "es_deform_inverse")
        torch.cuda.synchronize()
        return y.cpu(), step.cpu(), iters.cpu()


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"{c[1]}{c[0]}")
def case(request):
    """One state: device weights, the oracles, 200 points with the contraction asserted, the canonical points of (x, t_from) in fp32, and
    e_fwd: the largest error of the device's D against the fp64 oracle on these points at t_from and at t_to (the row 2-norm)."""
    seed, mode = request.param
    state = weightgen.make_state(seed, mode, True)
    dev, net64, net32 = Dev(state), oracle_net(state, torch.float64), oracle_net(state, torch.float32)
    x, t_from, t_to = draw(seed, M)
    rho = assert_contraction(net64, x, t_from, t_to)
    fn64 = deform_fn(net64)
    e_fwd = 0.0
    for t in (t_from, t_to):
        e_fwd = max(e_fwd, float(rownorm(dev.forward(x, t)[1].double() - fn64(x.double(), t.double())).max()))
    c = (x.double() + fn64(x.double(), t_from.double())).float()          # the device's input: fp32 values
    print(f"\n[{mode}{seed}] rho {rho:.3f}  e_fwd {e_fwd:.3e}  budget {budget(e_fwd):.3e}")
    return dict(dev=dev, net64=net64, net32=net32, fn64=fn64, x=x, t_from=t_from, t_to=t_to, c=c, e_fwd=e_fwd, name=f"{mode}{seed}")


@pytest.mark.parametrize("scalar_t", [False, True], ids=["t_rows", "t_scalar"])
def test_forward_parity(case, scalar_t):
    """x + D and D against the fp64 oracle for M in {1, 63, 64, 65, 200} and the edges of the 32-point tiles these batches run on, {31, 32,
    33} (prefixes of the case's 200 points; the 64-point tiles of large batches: ``test_both_tile_heights_give_the_same_bits``).  The yardstick is the
    error of the fp32 oracle against the fp64 oracle on the case's points -- its largest over the 200, one figure per case, so that the
    one-point batch is not held to the luck of one point's rounding; the device may be off by at most 4 times that: the two differ in
    the summation order of 256-term fp32 dot products only, while a misplaced weight shows at 1e-3 or more."""
    dev, x, fn64 = case["dev"], case["x"], case["fn64"]
    t = case["t_from"][:1] if scalar_t else case["t_from"]
    tM = t.expand(M) if scalar_t else t
    if scalar_t:
        assert_contraction(case["net64"], x, t)
    d64 = fn64(x.double(), tM.double())
    xc64 = x.double() + d64
    d32 = deform_fn(case["net32"])(x, tM.contiguous())
    yard_d, yard_xc = float((d32.double() - d64).abs().max()), float(((x + d32).double() - xc64).abs().max())
    for m in (1, 31, 32, 33, 63, 64, 65, 200):
        xc, d = dev.forward(x[:m], t if scalar_t else t[:m])
        e_d, e_xc = float((d.double() - d64[:m]).abs().max()), float((xc.double() - xc64[:m]).abs().max())
        print(f"[{case['name']}] M {m:3d} scalar_t {scalar_t}: device D {e_d:.3e} x+D {e_xc:.3e} | fp32 oracle D {yard_d:.3e} x+D {yard_xc:.3e}")
        assert e_d <= 4 * yard_d, (m, e_d, yard_d)
        assert e_xc <= 4 * yard_xc, (m, e_xc, yard_xc)
        # xc_out - x is d_out within one ulp of x (of the larger of |x| and |x + D|: the one rounding of the sum)
        ulp = torch.from_numpy(np.spacing(torch.maximum(x[:m].abs(), xc.abs()).numpy()))
        assert bool((((xc.double() - x[:m].double()) - d.double()).abs() <= ulp.double()).all())


def test_inverse_against_the_fp64_fixed_point(case):
    dev, c, t_to, e_fwd = case["dev"], case["c"], case["t_to"], case["e_fwd"]
    ystar = fixed_point64(case["net64"], c, t_to)
    y, step, iters = dev.inverse(c, t_to, max_iters=64, tol=TOL)
    assert bool((step <= TOL).all()), float(step.max())          # every row converges
    err = float(rownorm(y.double() - ystar).max())
    _, _, it_twin = tracking.inverse_deform(case["fn64"], c.double(), t_to.double(), max_iters=64, tol=TOL)
    di = int((iters - it_twin).abs().max())
    res = float(rownorm(y.double() + dev.forward(y, t_to)[1].double() - c.double()).max())
    print(f"[{case['name']}] |y - y*| {err:.3e} (budget {budget(e_fwd):.3e})  iters max {int(iters.max())} mean {float(iters.float().mean()):.2f} "
          f"|iters - twin| {di}  residual {res:.3e} (bound {TOL + 2 * e_fwd:.3e})")
    assert err <= budget(e_fwd), (err, budget(e_fwd))
    assert di <= 1
    assert res <= TOL + 2 * e_fwd, res


def test_rows_are_independent_bit_for_bit(case):
    dev, c, t = case["dev"], case["c"], case["t_to"]
    full = dev.inverse(c, t)
    assert len(set(full[2].tolist())) > 1          # rows do need different iteration counts
    again = dev.inverse(c, t)
    perm = torch.from_numpy(np.random.default_rng(3).permutation(M).copy())
    shuffled = dev.inverse(c[perm], t[perm])
    first = dev.inverse(c[:65], t[:65])
    alone = dev.inverse(c[117:118], t[117:118])
    for a, b, s, f, o in zip(full, again, shuffled, first, alone):
        assert torch.equal(a, b) and torch.equal(a[perm], s) and torch.equal(a[:65], f) and torch.equal(a[117:118], o)


def test_both_tile_heights_give_the_same_bits(case):
    """Up to 16 384 rows a launch runs 32-point tiles, above it 64-point tiles: the case's 200 rows repeated to 16 384 (the last batch of
    the small tiles, 512 of them) and to 16 385 rows (the first of the large ones, its last tile one row long) come out as in the
    200-row batch, bit for bit -- forward and inverse, so the oracle parity shown on the small tiles holds on the large ones."""
    dev, x, c, t_from, t_to = case["dev"], case["x"], case["c"], case["t_from"], case["t_to"]
    fwd, inv = dev.forward(x, t_from), dev.inverse(c, t_to)
    for n in (16384, 16385):
        idx = torch.arange(n) % M
        for a, b in zip(fwd, dev.forward(x[idx], t_from[idx])):
            assert torch.equal(a[idx], b), n
        for a, b in zip(inv, dev.inverse(c[idx], t_to[idx])):
            assert torch.equal(a[idx], b), n


def test_uniform_exit_with_mixed_tiles(case):
    """192 rows: rows 0-63 arrive with their first update (t_to = t_from, started at x: the step is the fp32 rounding of (x + D) - D), rows
    64-127 take several evaluations, rows 128-191 mix the two kinds row by row; each row as in a launch that holds its own kind only.
    Once on the 32-point tiles of a batch this small, once as the head of a 16 576-row batch on 64-point tiles."""
    dev, x, t_from, t_to = case["dev"], case["x"][:192], case["t_from"][:192], case["t_to"][:192]
    c = dev.forward(x, t_from)[0]          # the device's own x + D
    easy = torch.zeros(192, dtype=torch.bool)
    easy[:64] = True
    easy[128:] = torch.arange(64) % 2 == 0
    t = torch.where(easy, t_from, t_to)
    init = torch.where(easy[:, None], x, c)
    y, step, iters = dev.inverse(c, t, init)
    assert bool((iters[easy] == 1).all()) and bool((step[easy] <= TOL).all())
    assert bool((step <= TOL).all()) and int(iters[~easy].max()) >= 3, iters[~easy].tolist()
    print(f"[{case['name']}] easy step max {float(step[easy].max()):.3e}; hard iters {int(iters[~easy].min())}..{int(iters[~easy].max())}")
    for sel in (easy, ~easy):
        for a, b in zip((y, step, iters), dev.inverse(c[sel], t[sel], init[sel])):
            assert torch.equal(a[sel], b)
    big = torch.cat([torch.arange(192), torch.arange(16384) % 192])          # 16 576 rows: 64-point tiles, the first three as above
    for a, b in zip((y, step, iters), dev.inverse(c[big], t[big], init[big])):
        assert torch.equal(a[big], b)


def test_tol_zero_the_cap_and_a_given_start(case):
    dev, c, t, e_fwd = case["dev"], case["c"], case["t_to"], case["e_fwd"]
    y, step, iters = dev.inverse(c, t, max_iters=5, tol=0.0)
    assert bool((iters == 5).all()) and bool(torch.isfinite(y).all()) and bool(torch.isfinite(step).all())
    y, step, iters = dev.inverse(c, t, max_iters=3, tol=1e-7)
    assert bool((iters == 3).all()) and bool((step > 1e-7).all()) and bool(torch.isfinite(y).all()) and bool(torch.isfinite(step).all())
    # a start 0.05 away from the solution: the same fixed point, within the budget
    ystar = fixed_point64(case["net64"], c, t)
    off = torch.from_numpy(np.random.default_rng(7).normal(size=(M, 3)))
    init = (ystar + 0.05 * off / rownorm(off)[:, None]).float()
    y, step, iters = dev.inverse(c, t, init)
    err = float(rownorm(y.double() - ystar).max())
    print(f"[{case['name']}] perturbed start: |y - y*| {err:.3e} (budget {budget(e_fwd):.3e}), iters max {int(iters.max())}")
    assert bool((step <= TOL).all()) and err <= budget(e_fwd)


def test_the_refused_update():
    """A last-layer bias of 3e38 makes D finite and the squared step overflow: every row refuses its first update -- iters 1, step
    FLT_MAX, y bitwise its start -- with and without ``init``, and so does the fp32 host twin over the device's own D."""
    state = weightgen.make_state(11, "trained", True)
    state["deform_network.net.8.bias"] = np.full(3, 3e38, np.float32)
    dev = Dev(state)
    x, t_from, t_to = draw(11, 70)
    start = (x + 0.01).contiguous()
    twin_fn = lambda y, t: dev.forward(y.contiguous(), t.contiguous())[1] if y.shape[0] else y
    for init in (None, start):
        y, step, iters = dev.inverse(x, t_to, init)
        assert bool((iters == 1).all()) and bool((step == FLT_MAX).all())
        assert torch.equal(y, x if init is None else start)
        ty, ts, ti = tracking.inverse_deform(twin_fn, x, t_to, init)
        assert torch.equal(y, ty) and torch.equal(step, ts) and torch.equal(iters, ti)


def test_refusals():
    """Status 1 with a message before anything is launched (the addresses are host numpy's and never dereferenced); M = 0 is status 0."""
    from endosurf_amd import _lib
    lib = _lib.load()
    buf = np.zeros(64, np.float32)
    b = buf.ctypes.data

    def pts(M=4, mode=0):
        p = _lib.es_points()
        p.M, p.mode, p.t_scalar, p.n_per_ray, p.ldz = M, mode, 1, 1, 1
        p.x, p.t, p.rays, p.z = b, b, b, b
        return p

    inv = lambda p, y=b, max_iters=8, tol=1e-5: lib.es_deform_inverse(C.byref(p), None, b, b, max_iters, tol, y, b, b, None)
    assert inv(pts(mode=1)) == 1 and b"mode 0" in lib.es_last_error()
    assert lib.es_deform_forward(C.byref(pts(mode=1)), b, b, b, b, None) == 1 and b"mode 0" in lib.es_last_error()
    assert inv(pts(), y=None) == 1 and b"null buffer" in lib.es_last_error()
    assert inv(pts(), max_iters=0) == 1 and b"max_iters" in lib.es_last_error()
    for tol in (-1.0, float("nan"), float("inf")):
        assert inv(pts(), tol=tol) == 1 and b"tol" in lib.es_last_error()
    assert lib.es_deform_forward(C.byref(pts()), b, b, None, None, None) == 1 and b"both outputs" in lib.es_last_error()
    assert lib.es_deform_forward(C.byref(pts()), None, b, b, b, None) == 1 and b"null buffer" in lib.es_last_error()
    empty = _lib.es_points()
    assert lib.es_deform_forward(C.byref(empty), None, None, None, None, None) == 0
    assert lib.es_deform_inverse(C.byref(empty), None, None, None, 8, 1e-5, None, None, None, None) == 0
