"""References for the second-order half of the point chain -- what the reference gets from ``autograd.grad(..., create_graph=True)``
(endosurf.py:581-619) and from a backward through EndoSurfNet.forward to its inputs -- by autograd through the oracle's pieces
(OracleNet.deform, sdf_net, color, point_eval) and nothing else: no kernel, no endosurf_amd arithmetic.

  sweep            one reverse sweep of the deformation network for a covector c: (J^T c, CURV(c), tbar(c)), what es_point_vjp writes to
                   ES_WS_GO / ES_WS_CURV / ES_WS_TBAR (include/endosurf_hip.h), with CURV(c) := -diag(Hessian_x <x_c(x, t), c>)
  leaf_adjoints    (xcbar, vbar): the adjoints of x_c and v = J d that es_point_backward leaves in ES_WS_XCBAR / ES_WS_VBAR
  input_adjoints   (xbar, dbar, tbar): the adjoints of the inputs [x, d, t], plain autograd through point_eval
  through_go_only  d <g_o, wg> / d x: Engine.point_input_adjoint
  reordered        the same networks with every dot product summed in another order (a second draw of the fp32 run's rounding error)

Every function takes a ``dtype``: the weights and the inputs are cast to it, so that a test takes its yardstick from the fp32 run of the
same reference on the same rows.  Results are detached tensors of that dtype.  ``row_error`` is the error measure of the comparisons."""
import numpy as np
import torch

from oracle import endosurf_oracle as O


def cast_net(net, dtype):
    if all(v.dtype == dtype and not v.requires_grad for v in net.p.values()):
        return net
    return O.OracleNet({k: v.detach().to(dtype) for k, v in net.p.items()}, net.use_deform)


def reordered(net, seed):
    """The same networks with the hidden units of every layer permuted (rows of layer l, the matching columns of layer l + 1; at the
    skip layer only the columns that belong to layer 3's outputs): the same function in fp64 up to rounding, every 256-term dot
    product summed in another order.  Its fp32 run is another draw of the fp32 oracle's rounding error."""
    rng = np.random.default_rng(seed)
    p = {k: v.detach().clone() for k, v in net.p.items()}
    for name in (("deform_network",) if net.use_deform else ()) + ("sdf_network", "color_network"):
        for l in range(8):
            n = p[f"{name}.net.{l}.bias"].shape[0]
            perm = torch.from_numpy(rng.permutation(n))
            for k in ("bias", "weight_g", "weight_v"):
                p[f"{name}.net.{l}.{k}"] = p[f"{name}.net.{l}.{k}"][perm]
            cols = torch.arange(p[f"{name}.net.{l + 1}.weight_v"].shape[1])
            cols[:n] = perm
            p[f"{name}.net.{l + 1}.weight_v"] = p[f"{name}.net.{l + 1}.weight_v"][:, cols]
    return O.OracleNet(p, net.use_deform)


def _leaf(a, dtype, width):
    return a.detach().to(dtype).reshape(-1, width).clone().requires_grad_(True)


def _const(a, dtype, width):
    return None if a is None else a.detach().to(dtype).reshape(-1, width)


def sweep(net, x, t, c, dtype=torch.float64, hessian=None):
    """(J^T c [M,3], CURV(c) [M,3], tbar(c) [M,1]) from f = <x + deform(x, t), c>: grad_x f, minus the diagonal of the Hessian of f
    w.r.t. x (three autograd.grad calls on a first derivative taken with create_graph=True) and grad_t f.  In fp64 the off-diagonal
    entries of that Hessian must be exactly 0 -- the deformation MLP is piecewise linear in its encodings and the encodings act per
    coordinate ("the second term is diagonal", include/endosurf_hip.h) -- which is a condition on the inputs: asserted here.
    ``hessian``: a list that receives the full [M,3,3] Hessian.  Without a deformation network: (c, 0, 0)."""
    net = cast_net(net, dtype)
    x, t, c = _leaf(x, dtype, 3), _leaf(t, dtype, 1), _const(c, dtype, 3)
    M = x.shape[0]
    if not net.use_deform:
        return c.clone(), torch.zeros(M, 3, dtype=dtype), torch.zeros(M, 1, dtype=dtype)
    dx, _ = net.deform(x, t, with_jac=False)
    f = ((x + dx) * c).sum()
    g, tbar = torch.autograd.grad(f, (x, t), create_graph=True)
    H = torch.stack([torch.autograd.grad(g[:, j].sum(), x, retain_graph=True)[0] for j in range(3)], 1)          # H[m, j, k] = d2 f / dx_j dx_k
    diag = torch.diagonal(H, dim1=1, dim2=2)
    if dtype == torch.float64:
        off = H - torch.diag_embed(diag)
        assert bool((off == 0).all()), ("the Hessian of <x_c, c> is not diagonal", float(off.abs().max()))
    if hessian is not None:
        hessian.append(H.detach())
    return g.detach(), -diag.detach(), tbar.detach()


def _loss(sdf, g, rgb, ws, wg, wc):
    L = (sdf * ws).sum() if ws is not None else sdf.sum() * 0
    if wg is not None:
        L = L + (g * wg).sum()
    if rgb is not None:
        L = L + (rgb * wc).sum()
    return L


def leaf_adjoints(net, x, d, t, ws, wg, wc, color, dtype=torch.float64):
    """(xcbar [M,3], vbar [M,3] or None without colour): x_c = x + deform(x, t) and v = J d are made leaves, J is a constant, and
    L = <sdf, ws> + <J^T g_c, wg> (+ <rgb, wc>) formed on them is differentiated.  ``ws`` / ``wg`` may be None (no such term)."""
    net = cast_net(net, dtype)
    x, d, t = _const(x, dtype, 3), _const(d, dtype, 3), _const(t, dtype, 1)
    ws, wg, wc = _const(ws, dtype, 1), _const(wg, dtype, 3), _const(wc, dtype, 3)
    with torch.no_grad():
        dx, J = net.deform(x, t, with_jac=True)
    xc = (x + dx).detach().requires_grad_(True)
    sdf, feat, gc = net.sdf_net(xc, with_grad=True)
    go = torch.einsum("mik,mi->mk", J, gc)                                  # as OracleNet.point_eval
    if not color:
        return torch.autograd.grad(_loss(sdf, go, None, ws, wg, None), xc)[0].detach(), None
    v = torch.einsum("mik,mk->mi", J, d).detach().requires_grad_(True)
    d_c = v / (v.norm(dim=-1, keepdim=True) + 1e-10)                        # as OracleNet.point_eval
    rgb = net.color(xc, gc, d_c, feat)
    xcbar, vbar = torch.autograd.grad(_loss(sdf, go, rgb, ws, wg, wc), (xc, v))
    return xcbar.detach(), vbar.detach()


def input_adjoints(net, x, d, t, ws, wg, wc, color, dtype=torch.float64):
    """(xbar [M,3], dbar [M,3], tbar [M,1]): autograd of the same L through OracleNet.point_eval to its inputs.  An input that L does
    not depend on (d without colour, t without a deformation network) has the adjoint 0."""
    net = cast_net(net, dtype)
    x, d, t = _leaf(x, dtype, 3), _leaf(d, dtype, 3), _leaf(t, dtype, 1)
    ws, wg, wc = _const(ws, dtype, 1), _const(wg, dtype, 3), _const(wc, dtype, 3)
    pe = net.point_eval(x, d, t, with_color=color)
    grads = torch.autograd.grad(_loss(pe["sdf"], pe["g_o"], pe["rgb"] if color else None, ws, wg, wc), (x, d, t), allow_unused=True)
    return tuple(torch.zeros_like(a) if g is None else g.detach() for g, a in zip(grads, (x, d, t)))


def through_go_only(net, x, t, wg, canonical=False, dtype=torch.float64):
    """grad_x <g_o, wg> [M,3]; ``canonical``: x are canonical points and g_o is g_c of the SDF network alone."""
    net = cast_net(net, dtype)
    x, wg = _leaf(x, dtype, 3), _const(wg, dtype, 3)
    if canonical:
        g = net.sdf_net(x, with_grad=True)[2]
    else:
        g = net.point_eval(x, None, _const(t, dtype, 1), with_color=False)["g_o"]
    return torch.autograd.grad((g * wg).sum(), x)[0].detach()


def row_error(got, ref64):
    """Per row: max_j |got - ref64| / max(max_j |ref64| of the row, 1e-3 * max |ref64| of the batch) -> float64 ndarray [M].  A reference
    that is 0 everywhere gives 0 where ``got`` is exactly 0 and inf elsewhere."""
    got = np.asarray(got, np.float64).reshape(len(ref64), -1)
    ref = np.asarray(ref64, np.float64).reshape(len(ref64), -1)
    diff = np.abs(got - ref).max(1)
    den = np.maximum(np.abs(ref).max(1), 1e-3 * np.abs(ref).max())
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(diff == 0, 0.0, diff / den)
