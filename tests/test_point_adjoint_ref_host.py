"""The references of test_gpu_point_adjoint_shapes.py (point_adjoint_ref.py) checked against each other on the CPU in fp64, so that a
failure of the GPU comparison is not the reference's: the identity of include/endosurf_hip.h that Engine.point_input_adjoint and
functions._NetForwardFn.backward assemble,
    xbar = J^T xcbar - wg * CURV(g_c) - d * CURV(vbar),   dbar = J^T vbar,   tbar = <xcbar, d x_c / d t>,
between the leaf adjoints, the sweeps and plain autograd to the inputs; the diagonal Hessian; and the header's closed form of CURV
against its definition as -diag Hessian."""
import pytest
import torch

from oracle import endosurf_oracle as O
from point_adjoint_ref import input_adjoints, leaf_adjoints, reordered, sweep, through_go_only
from shapes_util import inputs, oracle_net

TOL = 1e-10


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-300))


@pytest.mark.parametrize("use_deform,M", [(True, 65), (False, 33)])
@pytest.mark.parametrize("color", [True, False])
def test_identity_between_the_references(use_deform, M, color):
    net = oracle_net("trained", use_deform)
    x, d, t, ws, wg, wc = inputs(M, 1300 + M, use_deform)
    xcbar, vbar = leaf_adjoints(net, x, d, t, ws, wg, wc, color)
    xbar, dbar, tbar = input_adjoints(net, x, d, t, ws, wg, wc, color)
    with torch.no_grad():
        g_c = net.point_eval(x.double(), d.double(), t.double()[:, None], with_color=False)["g_c"]
    H = []
    jx, _, tb = sweep(net, x, t, xcbar, hessian=H)
    _, curv_g, _ = sweep(net, x, t, g_c, hessian=H)
    want = jx - wg.double() * curv_g
    if color:
        jv, curv_v, _ = sweep(net, x, t, vbar, hessian=H)
        want = want - d.double() * curv_v
        assert _rel(jv, dbar) < TOL, _rel(jv, dbar)
    else:
        assert vbar is None and bool((dbar == 0).all())
    assert _rel(want, xbar) < TOL, _rel(want, xbar)
    if use_deform:
        assert _rel(tb, tbar) < TOL, _rel(tb, tbar)
        assert float(curv_g.abs().max()) > 1e-2 * float(xbar.abs().max())          # (the curvature term takes part in this check)
        for h in H:
            off = h - torch.diag_embed(torch.diagonal(h, dim1=1, dim2=2))
            assert bool((off == 0).all()) and float(h.abs().max()) > 0
    else:
        assert not H and bool((tbar == 0).all()) and bool((tb == 0).all()) and bool((curv_g == 0).all()) and torch.equal(jx, xcbar)
    # the adjoint through g_o alone is the same L without the sdf and colour terms
    only = through_go_only(net, x, t, wg)
    assert _rel(only, input_adjoints(net, x, d, t, None, wg, None, False)[0]) < TOL


def test_through_go_only_canonical_is_the_sdf_network_alone():
    M = 33
    x, d, t, ws, wg, wc = inputs(M, 1400, False)
    net = oracle_net("trained", False)
    a = through_go_only(net, x, t, wg, canonical=True)
    b = through_go_only(net, x, t, wg)                                       # without a deformation network x_c = x
    c = leaf_adjoints(net, x, d, t, None, wg, None, False)[0]               # ... and the adjoint of x_c is the adjoint of x
    assert float(a.abs().max()) > 0 and _rel(a, b) < TOL and _rel(a, c) < TOL


@pytest.mark.parametrize("use_deform", [True, False])
def test_reordered_networks_are_the_same_function(use_deform):
    """point_adjoint_ref.reordered: in fp64 every reference agrees with the unpermuted network's to rounding (1e-12), and the weights
    did move."""
    M = 33
    net = oracle_net("trained", use_deform)
    other = reordered(net, 1)
    assert not torch.equal(other.p["sdf_network.net.3.bias"], net.p["sdf_network.net.3.bias"])
    x, d, t, ws, wg, wc = inputs(M, 1500, use_deform)
    for a, b in zip(input_adjoints(net, x, d, t, ws, wg, wc, True), input_adjoints(other, x, d, t, ws, wg, wc, True)):
        assert torch.equal(a, b) or _rel(a, b) < 1e-12, _rel(a, b)
    a, b = leaf_adjoints(net, x, d, t, ws, wg, wc, True), leaf_adjoints(other, x, d, t, ws, wg, wc, True)
    assert _rel(a[0], b[0]) < 1e-12 and _rel(a[1], b[1]) < 1e-12
    if use_deform:
        for a, b in zip(sweep(net, x, t, wg), sweep(other, x, t, wg)):
            assert _rel(a, b) < 1e-12, _rel(a, b)


def test_closed_form_of_the_curvature():
    """ES_WS_CURV[j] = sum_i 4^i (e_sin(i,j) sin(2^i x_j) + e_cos(i,j) cos(2^i x_j)) with e the adjoint of the deformation MLP's encoding
    input (include/endosurf_hip.h es_point_vjp) equals -diag Hessian_x <x_c, c>.  e is taken at the encoding tensor itself: the position
    encoding that OracleNet.deform hands to its MLP (layer 0 and the skip) is picked up on its way in and differentiated against."""
    M = 65
    net = oracle_net("trained", True)
    x, d, t, ws, wg, wc = inputs(M, 1300 + M, True)
    c = wg.double()
    enc, plain = [], O.freq_encode

    def recording(a, L):
        enc.append(plain(a, L))
        return enc[-1]
    x64 = x.double().requires_grad_(True)
    O.freq_encode = recording
    try:
        dx, _ = net.deform(x64, t.double()[:, None], with_jac=False)
    finally:
        O.freq_encode = plain
    assert len(enc) == 2 and enc[0].shape == (M, 39) and enc[1].shape == (M, 13)          # position (L = 6), time
    e = torch.autograd.grad((dx * c).sum(), enc[0])[0]
    closed = torch.zeros(M, 3, dtype=torch.float64)
    for i in range(6):
        f = float(2 ** i)
        e_sin, e_cos = e[:, 3 + 6 * i:6 + 6 * i], e[:, 6 + 6 * i:9 + 6 * i]          # freq_encode: [x, sin(2^0 x), cos(2^0 x), sin(2^1 x), ...]
        closed += f * f * (e_sin * torch.sin(f * x.double()) + e_cos * torch.cos(f * x.double()))
    _, curv, _ = sweep(net, x, t, c)
    assert float(curv.abs().max()) > 1e-3 and _rel(closed, curv) < TOL, _rel(closed, curv)
