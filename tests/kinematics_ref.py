"""Shared by the kinematics tests: the fp64 reference for J = I + dD/dx, D_t = dD/dt and the second derivatives of the deformation map,
by autograd through ``OracleNet.deform(X, T, with_jac=False)`` -- the oracle's forward pass and torch's double backward, nothing of
``endosurf_amd``.  The rows of a batch are independent, so the gradient of a column's sum over the batch is that column's gradient
per row; autograd differentiates the ReLU as 0 / 1 with no second derivative, i.e. inside the linear region of each row."""
import torch


def derivatives(net, x, t, full=False):
    """dict(d [M,3] = D, jac [M,3,3], d_t [M,3], dd [M,3,3] with dd[m,i,k] = d2 D_i / d x_k^2) of ``net`` (an ``OracleNet``) at ``x`` [M,3],
    ``t`` [M], in their dtype; ``full``: also hess [M,3,3,3] = d2 D_i / d x_j d x_k and d_xt [M,3,3] = d2 D_i / d x_k dt."""
    X = x.detach().clone().requires_grad_(True)
    T = t.detach().clone().requires_grad_(True)
    D = net.deform(X, T, with_jac=False)[0]
    M = X.shape[0]
    jac, d_t = torch.zeros(M, 3, 3, dtype=X.dtype), torch.zeros(M, 3, dtype=X.dtype)
    hess, d_xt = torch.zeros(M, 3, 3, 3, dtype=X.dtype), torch.zeros(M, 3, 3, dtype=X.dtype)
    for i in range(3):
        gx, gt = torch.autograd.grad(D[:, i].sum(), (X, T), create_graph=True)
        jac[:, i], d_t[:, i] = gx.detach(), gt.detach()
        for j in range(3):
            hx, ht = torch.autograd.grad(gx[:, j].sum(), (X, T), retain_graph=True, allow_unused=True)
            if hx is not None:
                hess[:, i, j] = hx
            if ht is not None:
                d_xt[:, i, j] = ht
    out = {"d": D.detach(), "jac": jac + torch.eye(3, dtype=X.dtype), "d_t": d_t, "dd": torch.diagonal(hess, dim1=2, dim2=3).clone()}
    if full:
        out.update(hess=hess, d_xt=d_xt)
    return out


def derivs_fn(net):
    """``kinematics``' ``derivs_fn`` over the reference."""
    def fn(x, t):
        d = derivatives(net, x, t)
        return {k: d[k] for k in ("jac", "d_t", "dd")}
    return fn


def jacobian_fn(net):
    """``strain``'s ``jacobian_fn`` over the oracle's closed form."""
    def fn(x, t):
        with torch.no_grad():
            return net.deform(x, t)[1]
    return fn
