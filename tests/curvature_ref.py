"""References for the curvature tests: value, gradient and Hessian of the SDF, by autograd through the oracle's ``sdf_net`` /
``sdf_observed`` and nothing else -- no kernel, no endosurf_amd arithmetic.  Results are detached tensors of ``dtype``."""
import torch

from point_adjoint_ref import cast_net


def _hessian(f, x):
    sdf = f(x)
    g = torch.autograd.grad(sdf.sum(), x, create_graph=True)[0]
    H = torch.stack([torch.autograd.grad(g[:, j].sum(), x, retain_graph=True)[0] for j in range(3)], 1)          # H[m, j, k] = d2 sdf / dx_j dx_k
    return sdf.detach().reshape(-1, 1), g.detach(), H.detach()


def hessian_canonical(net, xc, dtype=torch.float64):
    """(sdf [M,1], g_c [M,3], H_c [M,3,3]) of the SDF network at canonical points."""
    net = cast_net(net, dtype)
    x = xc.detach().to(dtype).reshape(-1, 3).clone().requires_grad_(True)
    return _hessian(lambda p: net.sdf_net(p, with_grad=False)[0], x)


def hessian_observed(net, x, t, dtype=torch.float64):
    """(sdf [M,1], g_o [M,3], H_o [M,3,3]) of  sdf(x + D(x, t))  with respect to x."""
    net = cast_net(net, dtype)
    x = x.detach().to(dtype).reshape(-1, 3).clone().requires_grad_(True)
    t = t.detach().to(dtype).reshape(-1, 1)
    return _hessian(lambda p: net.sdf_observed(p, t), x)
