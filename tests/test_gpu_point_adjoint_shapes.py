"""The second-order half of the point chain -- the code behind the reference's ``autograd.grad(..., create_graph=True)`` -- row by row
against the fp64 oracle (point_adjoint_ref.py, checked on the CPU by test_point_adjoint_ref_host.py) at the point counts where tiles and
pad rows change: 1, 63, 64, 65, 127, 128, 129, 777 with the deformation network, 1, 65, 129 without it.

  A  ES_WS_CURV as es_point_forward leaves it (the curvature sums for c = g_c)
  B  es_point_vjp for a covector of the caller's: ES_WS_GO / ES_WS_CURV / ES_WS_TBAR on the three workspace layouts, a second sweep on the
     same workspace, NaN in the pad rows of ES_WS_GC
  C  ES_WS_XCBAR / ES_WS_VBAR as es_point_backward leaves them, and a sweep on the consumed workspace (the mask words survive the backward)
  D  the assembled adjoints: Engine.point_input_adjoint, the canonical query, EndoSurfNet.forward's backward to [x, d, t]
  E  split-precision mode: the point adjoint stays on the fp32 kernels (fp32_only), bit for bit; the refusals

Error of a buffer: per row, max_j |got - ref64| / max(max_j |ref64| of the row, 1e-3 max |ref64| of the batch), maximum over ALL rows
[0, M) (point_adjoint_ref.row_error).  Gate: MARGIN = 4 x the yardstick, the same figure of the oracle's own fp32 run against its fp64
run on the same rows, computed here (the convention of test_gpu_track.py: the device and the fp32 oracle differ in the summation order
of 256-term dot products; a misplaced row, a missing term or a wrong mask shows at 1e-2 or more).  Points from shapes_util.inputs:
screened away from the ReLU kinks.  Every case's worst error and yardstick go to point_adjoint_shapes.json in the log directory of
test_gpu_backward.py.

The yardstick is NOT the error of one fp32 run, for two reasons found while measuring (MI355X; with one run per case 4 of 106 cases
missed the gate, none by a fault of the kernels):
  * The worst-row error of ONE fp32 run is a draw, not a bound.  The adjoint of the time input is a 13-term sum whose terms cancel
    (2^i cos / sin against the encoding adjoints, deform_vjp_tile in point_fwd_bodies.h forms it the same way), and the measure divides by
    the row's own |tbar| down to 1e-3 of the batch's: the oracle's fp32 run with the hidden units of its layers permuted -- the same
    function, another summation order (point_adjoint_ref.reordered) -- moves its own worst row of the t column between 1.9e-4 and 2.6e-3
    at M = 64 (13 orders), and one host's BLAS gave 1.8e-4 where another's gave 2.6e-3 for the SAME run.  The device sat inside that
    range (7.4e-4 at M = 64, 1.4e-3 at M = 129: 4.2 and 4.5 x the one draw it was held against).  So the yardstick is the MAXIMUM over
    ORDERS = 6 summation orders of the fp32 oracle: still the oracle's own fp32 error on the case's rows, less dependent on the draw.
  * One row cannot estimate a worst row.  The colour network encodes x_c with 2^9: its adjoint of x_c moves by 0.7 ... 1.4e-5 (relative)
    per fp32 ulp of x_c (3e-8), whichever kernel computes it.  At the M = 1 point the device's x_c is 4.5e-8 from the fp64 value (its
    neighbours in test_gpu_forward_shapes.py: up to 9.1e-8, gate 1e-6), the fp32 oracle's 1.7e-8 in EVERY summation order (the final
    rounding of x + dx decides it): xcbar 2.8e-5 against a yardstick of 6.6e-6 (4.3 x), and 1.4e-6 against the fp64 reference evaluated
    AT the device's x_c.  At M = 63 the same figures are 3.1e-5 / 2.0e-5 / 7.1e-6: over many rows the oracle's draws cover the
    device's.  So a case with fewer than 63 rows takes the larger of its own yardstick and that of the 63- (without the deformation
    network: 65-) row case of the same weights.
The margin stays 4."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from gpu_util import renderer_for
from point_adjoint_ref import cast_net, input_adjoints, leaf_adjoints, reordered, row_error, sweep, through_go_only
from shapes_util import SEED, inputs, oracle_net, routes_split, split_chain
from test_gpu_backward import LOG

pytestmark = pytest.mark.gpu
MS = (1, 63, 64, 65, 127, 128, 129, 777)
MS_NODEFORM = (1, 65, 129)
SHAPES = [(True, M) for M in MS] + [(False, M) for M in MS_NODEFORM]
MARGIN = 4.0
ORDERS = 6                                  # summation orders of the fp32 oracle behind a yardstick (the module's docstring)
POPULATION = {True: 63, False: 65}          # the case whose yardstick a case of fewer rows shares
_REPORT, _SETUP, _CASES, _NETS = {}, {}, {}, {}


def _note(case, **values):
    _REPORT.setdefault(case, {}).update(values)
    os.makedirs(LOG, exist_ok=True)
    with open(os.path.join(LOG, "point_adjoint_shapes.json"), "w") as f:
        json.dump(_REPORT, f, indent=1, sort_keys=True)


def _setup(use_deform):
    """One renderer (one engine, one caching-allocator history) per weight set for the whole module:
    (renderer, engine, weff, packed, fp64 oracle net)."""
    if use_deform not in _SETUP:
        r = renderer_for(SEED, "trained", use_deform)
        with torch.no_grad():
            weff, packed = r._weights()
        _SETUP[use_deform] = (r, r.engine, weff.detach(), packed, oracle_net("trained", use_deform))
    return _SETUP[use_deform]


class _Case:
    """The inputs of one (use_deform, M) and its references, each computed once: fp64, and the fp32 run's error against it."""

    def __init__(self, use_deform, M):
        n = [0]
        self.use_deform, self.M = use_deform, M
        self.x, self.d, self.t, self.ws, self.wg, self.wc = inputs(M, 6000 + M, use_deform, count=n)
        self.redrawn = n[0]
        rng = np.random.default_rng(6100 + M)
        self.c, self.c2 = (torch.from_numpy(rng.normal(size=(M, 3)).astype(np.float32)) for _ in range(2))
        self.refs = {}

    def errors(self, key, fn):
        """``fn(net, case, dtype)`` -> {name: tensor}; returns ({name: fp64 ndarray}, {name: the worst row error of the oracle's fp32
        run over ORDERS summation orders}) on this case's rows."""
        if key not in self.refs:
            net = _setup(self.use_deform)[4]
            r64 = {k: v.double().numpy() for k, v in fn(net, self, torch.float64).items()}
            yard = dict.fromkeys(r64, 0.0)
            for order in range(ORDERS):
                if (self.use_deform, order) not in _NETS:
                    _NETS[(self.use_deform, order)] = cast_net(reordered(net, order) if order else net, torch.float32)
                r32 = fn(_NETS[(self.use_deform, order)], self, torch.float32)
                yard = {k: max(yard[k], float(row_error(r32[k].double().numpy(), r64[k]).max())) for k in r64}
            self.refs[key] = (r64, yard)
        return self.refs[key]

    def ref(self, key, fn):
        """The fp64 reference and the yardstick of every buffer (the module's docstring)."""
        r64, yard = self.errors(key, fn)
        if self.M < POPULATION[self.use_deform]:
            big = _case(self.use_deform, POPULATION[self.use_deform]).errors(key, fn)[1]
            yard = {k: max(yard[k], big[k]) for k in yard}
        return r64, yard


def _case(use_deform, M):
    if (use_deform, M) not in _CASES:
        _CASES[(use_deform, M)] = _Case(use_deform, M)
    return _CASES[(use_deform, M)]


def _dev(a):
    return None if a is None else a.cuda().contiguous()


def _flags(use_deform, color=False, save=True):
    from endosurf_amd import _lib
    return (_lib.PF_DEFORM if use_deform else 0) | (_lib.PF_COLOR if color else 0) | (_lib.PF_SAVE if save else 0)


def _forward(cs, flags):
    eng, weff, packed = _setup(cs.use_deform)[1:4]
    return eng.point_forward(eng.points(x=_dev(cs.x), t=_dev(cs.t), dirs=_dev(cs.d)), weff, packed, flags)


def _vjp(cs, ctx, c):
    """es_point_vjp for the covector ``c`` (a device tensor [M,3]) -> {go, curv, tbar}, own storage."""
    eng, weff, packed = _setup(cs.use_deform)[1:4]
    ctx.view("gc").copy_(c)
    eng.point_vjp(ctx, weff, packed)
    return {k: ctx.view(k).clone() for k in ("go", "curv", "tbar")}


def _compare(case, cs, got, ref64, yard, names=None):
    """Every row of every buffer of ``got`` ({name: device tensor [M, w]}) against ``ref64`` under MARGIN x ``yard``."""
    bad, out = {}, {}
    for k in (names or got):
        g = got[k].detach().double().cpu().numpy().reshape(cs.M, -1)
        assert np.isfinite(g).all(), (case, k, "non-finite rows", np.nonzero(~np.isfinite(g).all(1))[0][:8])
        err = row_error(g, ref64[k])
        worst = float(err.max())
        out[k] = [worst, yard[k]]
        print(f"{case} {k}: device {worst:.3e}  fp32 oracle {yard[k]:.3e}  ratio {worst / max(yard[k], 1e-300):.2f}")
        if not worst < MARGIN * yard[k]:
            bad[k] = (worst, "gate", MARGIN * yard[k], "rows", [int(i) for i in np.argsort(-err)[:6]])
    _note(case, redrawn=cs.redrawn, **out)
    assert not bad, (case, bad)


def _sweep_ref(net, cs, c, dtype, prefix=""):
    go, curv, tbar = sweep(net, cs.x, cs.t, c, dtype)
    return {prefix + "go": go, prefix + "curv": curv, prefix + "tbar": tbar}


# The references, as ``fn(net, case, dtype)`` of _Case.errors (one function per key: a small case evaluates it on a larger one as well).
def _ref_forward_curvature(net, cs, dtype):
    with torch.no_grad():
        g_c = cast_net(net, dtype).point_eval(cs.x.to(dtype), None, cs.t.to(dtype)[:, None], with_color=False)["g_c"]
    return {"curv": sweep(net, cs.x, cs.t, g_c, dtype)[1]}


def _ref_foreign(net, cs, dtype):
    return _sweep_ref(net, cs, cs.c, dtype)


def _ref_leaf(color):
    def ref(net, cs, dtype):
        xcbar, vbar = leaf_adjoints(net, cs.x, cs.d, cs.t, cs.ws, cs.wg, cs.wc, color, dtype)
        out = {"xcbar": xcbar, **({"vbar": vbar} if color else {})}
        if cs.use_deform:
            out.update(_sweep_ref(net, cs, xcbar, dtype, "sweep_"))
        return out
    return ref


def _ref_through_go(canonical):
    return lambda net, cs, dtype: {"xbar": through_go_only(net, cs.x, cs.t, cs.wg, canonical=canonical, dtype=dtype)}


def _ref_model_forward(net, cs, dtype):
    xbar, dbar, tbar = input_adjoints(net, cs.x, cs.d, cs.t, cs.ws, None, cs.wc, True, dtype)
    return {"x": xbar, "d": dbar, "t": tbar}


# ------------------------------------------------------------------------------------------------------------------------------
# A. the forward's own ES_WS_CURV
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("color", [True, False])
def test_forward_curvature(M, color):
    """ES_WS_CURV after es_point_forward (ES_PF_DEFORM | ES_PF_SAVE, with and without ES_PF_COLOR) against sweep(g_c): the curvature
    sums for the forward's own covector, which Engine.point_input_adjoint reads before its sweep overwrites them."""
    cs = _case(True, M)
    ref64, yard = cs.ref("A", _ref_forward_curvature)
    ctx = _forward(cs, _flags(True, color))
    _compare(f"A_curv_{M}_{int(color)}", cs, {"curv": ctx.view("curv")}, ref64, yard)


# ------------------------------------------------------------------------------------------------------------------------------
# B. es_point_vjp with a covector of the caller's
# ------------------------------------------------------------------------------------------------------------------------------
LAYOUTS = {"plain": (False, False), "save": (False, True), "save_colour": (True, True)}          # (ES_PF_COLOR, ES_PF_SAVE)


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_vjp_foreign_covector(M, layout):
    """A random normal covector c written to ES_WS_GC behind a forward: ES_WS_GO / ES_WS_CURV / ES_WS_TBAR against sweep(c) on the
    no-grad layout, the saving layout and the saving layout with colour.  Then a second sweep with another covector on the SAME
    workspace: bit for bit the sweep with that covector on a fresh forward of the same points (the sweep reads the forward's mask words
    and leaves them alone)."""
    cs = _case(True, M)
    color, save = LAYOUTS[layout]
    ref64, yard = cs.ref("B", _ref_foreign)
    ctx = _forward(cs, _flags(True, color, save))
    got = _vjp(cs, ctx, _dev(cs.c))
    _compare(f"B_vjp_{M}_{layout}", cs, got, ref64, yard)
    second = _vjp(cs, ctx, _dev(cs.c2))
    fresh = _vjp(cs, _forward(cs, _flags(True, color, save)), _dev(cs.c2))
    torch.cuda.synchronize()
    for k in second:
        assert torch.equal(second[k], fresh[k]), (k, "the second sweep on one workspace differs from a sweep on a fresh forward")
        assert not torch.equal(second[k], got[k])


@pytest.mark.parametrize("M", [65, 129])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_vjp_ignores_pad_rows_of_the_covector(M, layout):
    """Rows [M, Mp) of ES_WS_GC hold NaN when the sweep starts: rows [0, M) of its three outputs are bit for bit those of the run
    without (63 NaN rows share the second 64-row tile with row 64 at M = 65; 127 of them follow row 128 at M = 129)."""
    from endosurf_amd import _lib
    cs = _case(True, M)
    eng = _setup(True)[1]
    color, save = LAYOUTS[layout]
    flags = _flags(True, color, save)
    clean = _vjp(cs, _forward(cs, flags), _dev(cs.c))
    ctx = _forward(cs, flags)
    off = int(eng.lib.es_point_workspace_offset(M, flags, _lib.WS_GC))          # as PointCtx.view, without its [:M] cut
    assert ctx.Mp > M
    ctx.ws[off:off + ctx.Mp * 3].view(ctx.Mp, 3)[M:] = float("nan")
    got = _vjp(cs, ctx, _dev(cs.c))
    torch.cuda.synchronize()
    assert bool(torch.isnan(ctx.ws[off:off + ctx.Mp * 3].view(ctx.Mp, 3)[M:]).all())
    for k in got:
        assert bool(torch.isfinite(got[k]).all()) and torch.equal(got[k], clean[k]), (k, "pad rows of the covector reached rows [0, M)")


# ------------------------------------------------------------------------------------------------------------------------------
# C. what the backward leaves in the workspace
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_deform,M", SHAPES)
@pytest.mark.parametrize("color", [True, False])
def test_backward_leaf_adjoints(use_deform, M, color):
    """ES_WS_XCBAR (and, with colour, ES_WS_VBAR) after es_point_backward(d_sdf = ws, d_go = wg, d_rgb = wc) against the adjoints of the
    leaves x_c and v = J d.  Then, with a deformation network, xcbar is copied to ES_WS_GC of the CONSUMED workspace and swept: against
    sweep(xcbar64) -- the forward's ReLU mask words are still there after the backward has written its adjoint buffers."""
    cs = _case(use_deform, M)
    eng, weff, packed = _setup(use_deform)[1:4]
    ref64, yard = cs.ref(("C", color), _ref_leaf(color))
    ctx = _forward(cs, _flags(use_deform, color))
    eng.point_backward(ctx, weff, packed, _dev(cs.ws), _dev(cs.wg), _dev(cs.wc) if color else None)
    got = {"xcbar": ctx.view("xcbar").clone(), **({"vbar": ctx.view("vbar").clone()} if color else {})}
    if use_deform:
        got.update({"sweep_" + k: v for k, v in _vjp(cs, ctx, got["xcbar"]).items()})
    _compare(f"C_leaf_{int(use_deform)}_{M}_{int(color)}", cs, got, ref64, yard)


# ------------------------------------------------------------------------------------------------------------------------------
# D. the assembled adjoints
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_deform,M", SHAPES)
@pytest.mark.parametrize("with_sdf", [True, False])
def test_point_input_adjoint(use_deform, M, with_sdf):
    """Engine.point_input_adjoint behind es_point_backward(d_sdf, d_go = wg) against grad_x <g_o, wg>: with d_sdf = ws the share
    ws * g_o of the sdf path has to cancel out of J^T xcbar, with d_sdf = None there is none."""
    cs = _case(use_deform, M)
    eng, weff, packed = _setup(use_deform)[1:4]
    ref64, yard = cs.ref("D_go", _ref_through_go(False))
    d_sdf = _dev(cs.ws) if with_sdf else None
    ctx = _forward(cs, _flags(use_deform))
    eng.point_backward(ctx, weff, packed, d_sdf, _dev(cs.wg))
    xbar = eng.point_input_adjoint(ctx, weff, packed, d_sdf, _dev(cs.wg))
    _compare(f"D_go_{int(use_deform)}_{M}_{int(with_sdf)}", cs, {"xbar": xbar}, ref64, yard)


def test_canonical_gradient_query_wrt_points():
    """model.get_sdf_grad_from_canonical_space(x.requires_grad_()) and a backward of <g, wg>: the SDF network's Hessian-vector product on a
    model that HAS a deformation network (the query switches it off), M = 65."""
    cs = _case(True, 65)
    r = _setup(True)[0]
    ref64, yard = cs.ref("D_canonical", _ref_through_go(True))
    x = _dev(cs.x).requires_grad_(True)
    g = r.model.get_sdf_grad_from_canonical_space(x)
    (g * _dev(cs.wg)).sum().backward()
    _compare("D_canonical_65", cs, {"xbar": x.grad}, ref64, yard)


@pytest.mark.parametrize("use_deform,M", SHAPES)
def test_model_forward_input_adjoints(use_deform, M):
    """model.forward(inputs.requires_grad_()) and a backward with the adjoints (ws, wc) of (sdf, rgb): the x, d and t columns of
    inputs.grad, each against plain autograd through the oracle and under its own yardstick (functions._NetForwardFn: two sweeps on one
    consumed workspace).  Without a deformation network the t column is exactly 0."""
    cs = _case(use_deform, M)
    r = _setup(use_deform)[0]
    ref64, yard = cs.ref("D_forward", _ref_model_forward)
    inp = torch.cat([cs.x, cs.d, cs.t[:, None]], -1).cuda().requires_grad_(True)
    out = r.model.forward(inp)
    assert tuple(out.shape) == (M, 4)
    out.backward(torch.cat([cs.ws, cs.wc], -1).cuda())
    got = {"x": inp.grad[:, :3], "d": inp.grad[:, 3:6], "t": inp.grad[:, 6:7]}
    if not use_deform:
        assert bool((ref64["t"] == 0).all()) and bool((got["t"] == 0).all()), "without a deformation network nothing depends on t"
    _compare(f"D_forward_{int(use_deform)}_{M}", cs, got, ref64, yard, names=["x", "d"] + (["t"] if use_deform else []))


# ------------------------------------------------------------------------------------------------------------------------------
# E. split-precision mode: the routing of the point adjoint, the refusals
# ------------------------------------------------------------------------------------------------------------------------------
def _recorded(eng, fn):
    """``fn()`` with every context that Engine.point_forward hands out recorded: (result, contexts)."""
    seen, plain = [], eng.point_forward

    def recording(*a, **k):
        seen.append(plain(*a, **k))
        return seen[-1]
    eng.point_forward = recording
    try:
        return fn(), seen
    finally:
        del eng.point_forward


@pytest.mark.parametrize("M", [65, 129])
def test_split_precision_keeps_the_point_adjoint_on_the_fp32_kernels(M):
    """With engine.split_precision on (and the threshold at 1 point, so that a saving forward of these sizes WOULD go to
    es_point_forward_x3) the gradient query and model.forward, each with a backward to its inputs, give input adjoints bit for bit
    those of the mode off: their forwards are pinned to the fp32 kernels (fp32_only -- the sweep reads that family's mask words, and
    ES_WS_CURV of the other family's workspace is undefined), and ES_PF_X3 in es_point_backward selects the weight-gradient GEMMs only."""
    cs = _case(True, M)
    r, eng = _setup(True)[:2]

    def query():
        x = _dev(cs.x).requires_grad_(True)
        g = r.model.get_sdf_grad_from_observed_space(x, _dev(cs.t))
        (g * _dev(cs.wg)).sum().backward()
        return x.grad.clone()

    def forward():
        inp = torch.cat([cs.x, cs.d, cs.t[:, None]], -1).cuda().requires_grad_(True)
        r.model.forward(inp).backward(torch.cat([cs.ws, cs.wc], -1).cuda())
        return inp.grad.clone()
    for name, fn in (("query", query), ("forward", forward)):
        off, ctxs_off = _recorded(eng, fn)
        with split_chain(eng, True, infer_min=1):
            assert routes_split(eng, M, True), "a saving forward of this size would not be routed to the split-precision chain"
            on, ctxs_on = _recorded(eng, fn)
        torch.cuda.synchronize()
        assert len(ctxs_off) >= 1 and len(ctxs_on) == len(ctxs_off)
        for ctx in ctxs_on + ctxs_off:
            assert not ctx.x3_chain and ctx.px3 is None, (name, "the point adjoint's forward ran on the split-precision kernels")
        assert bool(torch.isfinite(on).all()) and float(on.abs().max()) > 0
        assert torch.equal(on, off), (name, float((on - off).abs().max()))


def test_point_adjoint_refuses_a_split_precision_workspace():
    """A context of a saving split-precision forward is marked (ctx.x3_chain); Engine.point_input_adjoint on it raises before any
    library call, and the workspace is untouched."""
    from endosurf_amd import _lib
    cs = _case(True, 65)
    eng, weff, packed = _setup(True)[1:4]
    with split_chain(eng, True, infer_min=1):
        ctx = _forward(cs, _flags(True))
    torch.cuda.synchronize()
    assert ctx.x3_chain and ctx.px3 is not None
    before, calls = ctx.ws.clone(), _lib.calls
    with pytest.raises(_lib.EndoSurfHipError, match="fp32 kernels"):
        eng.point_input_adjoint(ctx, weff, packed, None, _dev(cs.wg))
    torch.cuda.synchronize()
    assert _lib.calls == calls and torch.equal(ctx.ws.view(torch.int32), before.view(torch.int32))


def test_vjp_refuses_a_workspace_without_deformation_network():
    """es_point_vjp without ES_PF_DEFORM: status 1 with its message before anything is launched (the addresses are host numpy's and
    never dereferenced)."""
    from endosurf_amd import _lib
    lib = _lib.load()
    buf = np.zeros(64, np.float32)
    b = buf.ctypes.data
    p = _lib.es_points()
    p.M, p.mode, p.t_scalar, p.n_per_ray, p.ldz = 4, 0, 0, 1, 1
    p.x, p.t = b, b
    for flags in (0, _lib.PF_SAVE, _lib.PF_SAVE | _lib.PF_COLOR):
        assert lib.es_point_vjp(C.byref(p), b, b, b, flags, None) == 1 and b"ES_PF_DEFORM" in lib.es_last_error(), flags
    assert not buf.any()
