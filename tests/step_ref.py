"""fp64 references of the small launches that hold a training step together (csrc/aux.hip, rays.hip k_train_aux_points, loss.hip,
step.hip k_render_finish, optim.hip): plain torch / python in double precision on fp32 inputs promoted exactly, one function per
kernel, each the formula the kernel's comment cites.  No GPU, no library.  Pinned against the oracle's own code
(oracle/endosurf_oracle.py) and torch.optim.Adam by tests/test_step_ref_host.py; the gates of tests/test_gpu_step_kernels.py are
measured against these."""
import math

import numpy as np
import torch

U = 2.0 ** -24          # unit round-off of fp32
F64 = torch.float64
LOSS_KEYS = ("color", "depth", "sdf", "angle", "eikonal", "surf_neig")


def d64(a):
    """``a`` (ndarray / tensor / scalar) as a detached fp64 CPU tensor: fp32 values are promoted exactly."""
    if torch.is_tensor(a):
        return a.detach().cpu().to(F64)
    return torch.as_tensor(np.asarray(a)).to(F64)


def fl32(x):
    """A python number rounded to fp32 and back: what a ``float`` argument of the C ABI carries."""
    return float(np.float32(x))


# ---- points ---------------------------------------------------------------------------------------------------------------------
def aux_points(rays, depth_gt, mask, d_i, u, rad):
    """The 3N auxiliary points of a training step (endosurf.py:297-300, :323-332):
         rows [0,N)    o + d / (d.z + 1e-6) * depth_gt
         rows [N,2N)   o + d / (d.z + 1e-6) * (d_i if valid else 0)
         rows [2N,3N)  the row above + (u - 0.5) * rad
       valid = isfinite(d_i) & (d_i != 0) & (mask == 1);  inside = (|x_eod| < 1) * mask (endosurf.py:306-309);  t = rays[:, 8] thrice.
    -> x [3N,3], t [3N], valid [N] (bool), inside [N].  es_sn_points is rows [N,3N), es_eod_points rows [0,N) of this."""
    rays, u = d64(rays), d64(u)
    N = rays.shape[0]
    dg, m, di = d64(depth_gt).reshape(N, 1), d64(mask).reshape(N, 1), d64(d_i).reshape(N, 1)
    o, d = rays[:, :3], rays[:, 3:6]
    dz = d / (d[:, 2:3] + 1e-6)
    valid = torch.isfinite(di) & (di != 0) & (m == 1)
    x_eod = o + dz * dg
    x_s = o + dz * torch.where(valid, di, torch.zeros_like(di))
    x_n = x_s + (u - 0.5) * fl32(rad)
    inside = (x_eod.norm(dim=-1, keepdim=True) < 1.0).to(F64) * m
    return torch.cat([x_eod, x_s, x_n], 0), rays[:, 8].repeat(3), valid[:, 0], inside[:, 0]


# ---- errorondepth's reductions (endosurf.py:302-317) ---------------------------------------------------------------------------------
def eod_formula(rays, pts, mask, sdf, go):
    """sdf_error, angle_error, inside, denominator in the dtype of the inputs (the relu(cos) sum is NOT masked, like the reference)."""
    inside = (torch.linalg.norm(pts, dim=-1, keepdim=True) < 1.0).to(pts.dtype) * mask
    den = inside.sum() + 1e-6
    sdf_err = (inside * sdf).abs().sum() / den
    ang_err = torch.relu((rays[:, 3:6] * go).sum(-1, keepdim=True)).abs().sum() / den
    return sdf_err, ang_err, inside, den


def eod_loss(rays, pts, mask, sdf, go, g_sdf_err=0.0, g_ang_err=0.0):
    """es_eod_loss and its backward: {sdf_err, ang_err, den, inside [N], d_sdf [N], d_go [N,3]}; the adjoints are those of
    g_sdf_err * sdf_err + g_ang_err * ang_err by fp64 autograd."""
    rays, pts = d64(rays), d64(pts)
    N = rays.shape[0]
    mask = d64(mask).reshape(N, 1)
    sdf, go = d64(sdf).reshape(N, 1).requires_grad_(True), d64(go).reshape(N, 3).requires_grad_(True)
    a, b, inside, den = eod_formula(rays, pts, mask, sdf, go)
    (float(g_sdf_err) * a + float(g_ang_err) * b).backward()
    z = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    return dict(sdf_err=a.detach(), ang_err=b.detach(), den=den.detach(), inside=inside[:, 0].detach(), d_sdf=z(sdf)[:, 0], d_go=z(go))


# ---- surface_neighbour_error's reduction (endosurf.py:334-339) -----------------------------------------------------------------------
def sn_formula(g, valid):
    """mean over the valid rays of |n - n'|, n = g / (|g| + 1e-10), rows [0,N) the surface points and [N,2N) their neighbours; 0 with the
    denominator 1 when no ray is valid."""
    N = valid.shape[0]
    normal = g / (torch.linalg.norm(g, dim=-1, keepdim=True) + 1e-10)
    diff = (normal[:N] - normal[N:]).abs() * valid[:, None].to(g.dtype)
    den = torch.clamp(valid.sum() * 3, min=1).to(g.dtype)
    return diff.sum() / den, den


def sn_loss(g, valid, g_loss=1.0):
    """es_sn_loss and its backward: {loss, den, d_g [2N,3]}."""
    g = d64(g).requires_grad_(True)
    valid = torch.as_tensor(np.asarray(valid.cpu() if torch.is_tensor(valid) else valid)).bool()
    loss, den = sn_formula(g, valid)
    (float(g_loss) * loss).backward()
    return dict(loss=loss.detach(), den=den, d_g=g.grad)


# ---- the training loss (trainer_endosurf.py:133-162) -----------------------------------------------------------------------------------
def loss_formula(color_map, depth_map, eik, a_sdf, a_go, rays, eod_pts, color_gt, depth_gt, mask, cmask, valid_sn, w, den_global=None, world=1.0):
    """compute_loss with errorondepth's and surface_neighbour_error's reductions written out, in the dtype of the inputs:
    -> total, {term: value}, the four local normalisers {sum cmask, sum inside, sum inside * mask, n_valid}.  ``den_global`` [4] replaces
    the local normalisers and every batch term is scaled by ``world`` (exact data-parallel mode, include/endosurf_hip.h)."""
    N = rays.shape[0]
    dt = color_map.dtype
    inside = (torch.linalg.norm(eod_pts, dim=-1, keepdim=True) < 1.0).to(dt) * mask
    vm = inside * mask
    nv = valid_sn.sum()
    dens = [cmask.sum(), inside.sum(), vm.sum(), nv.to(dt)]
    dg = dens if den_global is None else [den_global[i] for i in range(4)]
    color_loss = ((color_map - color_gt) * cmask).abs().sum() / (dg[0] + 1e-10)
    cos = (rays[:, 3:6] * a_go[:N]).sum(-1, keepdim=True)
    den = dg[1] + 1e-6
    sdf_loss = (inside * a_sdf[:N]).abs().sum() / den
    angle_loss = torch.relu(cos).abs().sum() / den
    depth_loss = ((depth_map - depth_gt) * vm).abs().sum() / (dg[2] + 1e-10)
    g = a_go[N:]
    normal = g / (torch.linalg.norm(g, dim=-1, keepdim=True) + 1e-10)
    diff = (normal[:N] - normal[N:]).abs() * valid_sn[:, None].to(dt)
    sn = diff.sum() / torch.clamp(dg[3] * 3, min=1).to(dt)
    terms = dict(color=color_loss * world, depth=depth_loss * world, sdf=sdf_loss * world, angle=angle_loss * world, eikonal=eik,
                 surf_neig=sn * world)
    return sum(w[k] * terms[k] for k in terms), terms, dens


def torch_loss(color_map, depth_map, eik, a_sdf, a_go, rays, eod_pts, color_gt, depth_gt, mask, cmask, valid_sn, w):
    """(total, terms) of ``loss_formula`` on tensors of any dtype and device (tests/test_gpu_loss.py runs it in fp32 on the GPU)."""
    total, terms, _ = loss_formula(color_map, depth_map, eik, a_sdf, a_go, rays, eod_pts, color_gt, depth_gt, mask, cmask, valid_sn, w)
    return total, terms


def train_loss(color_map, depth_map, eik, a_sdf, a_go, rays, eod_pts, color_gt, depth_gt, mask, cmask, valid_sn, w, den_global=None, world=1.0):
    """es_train_loss: {terms: {name: value}, total, n_valid, den [4], g_color [N,3], g_depth [N,1], g_eik, g_aux_sdf [3N,1],
    g_aux_go [3N,3]} in fp64; the adjoints are d total by autograd.  The weights are rounded to fp32 (they are ``float`` members)."""
    rays = d64(rays)
    N = rays.shape[0]
    outs = [d64(color_map).reshape(N, 3), d64(depth_map).reshape(N, 1), d64(eik).reshape(()), d64(a_sdf).reshape(3 * N, 1), d64(a_go).reshape(3 * N, 3)]
    outs = [t.requires_grad_(True) for t in outs]
    valid = torch.as_tensor(np.asarray(valid_sn.cpu() if torch.is_tensor(valid_sn) else valid_sn)).bool()
    w = {k: fl32(w[k]) for k in LOSS_KEYS}
    dg = None if den_global is None else d64(den_global)
    total, terms, dens = loss_formula(*outs, rays, d64(eod_pts).reshape(N, 3), d64(color_gt).reshape(N, 3), d64(depth_gt).reshape(N, 1),
                                      d64(mask).reshape(N, 1), d64(cmask).reshape(N, 1), valid, w, dg, float(world))
    total.backward()
    g = [torch.zeros_like(t) if t.grad is None else t.grad for t in outs]
    den = [float(x) for x in dens]
    return dict(terms={k: terms[k].detach() for k in LOSS_KEYS}, total=total.detach(), n_valid=float(valid.sum()), den=den,
                den_used=den if dg is None else [float(x) for x in dg],
                g_color=g[0], g_depth=g[1], g_eik=g[2], g_aux_sdf=g[3], g_aux_go=g[4], w=w)


# ---- the render forward's epilogue (endosurf.py:187-190) -------------------------------------------------------------------------------
def render_finish(eik_acc):
    """gradient_o_error = sum(relax * err) / (sum(relax) + 1e-6) from the two batch sums -> (eik, den) in double."""
    acc = d64(eik_acc)
    den = float(acc[1]) + 1e-6
    return float(acc[0]) / den, den


# ---- schedule and optimiser -------------------------------------------------------------------------------------------------------------
def schedule(step, t, lr_init, n_iter, warm_up_end, lr_alpha, beta1, beta2, grad_scale, anneal_end):
    """The four scalars es_train_schedule writes at global step ``step`` and Adam step ``t`` (both already incremented):
      lr = lr_init * (step / warm_up_end if step < warm_up_end else (cos(pi (step - warm) / (n_iter - warm)) + 1) / 2 (1 - alpha) + alpha)
                                                                                 (update_learning_rate, trainer_endosurf.py:183-203)
      [lr / (1 - beta1^t), sqrt(1 - beta2^t), grad_scale, 1 if anneal_end == 0 else min(1, step / anneal_end)]   (torch.optim.Adam's
      bias corrections; get_cos_anneal_ratio, endosurf.py:215-219), all in double."""
    if step < warm_up_end:
        f = step / warm_up_end
    else:
        f = (math.cos(math.pi * (step - warm_up_end) / (n_iter - warm_up_end)) + 1.0) * 0.5 * (1.0 - lr_alpha) + lr_alpha
    return [lr_init * f / (1.0 - beta1 ** t), math.sqrt(1.0 - beta2 ** t), float(grad_scale), 1.0 if anneal_end == 0 else min(1.0, step / anneal_end)]


def adam(p, g, m, v, beta1, beta2, eps, step_size, bc2_sqrt, grad_scale=1.0, extra=None, extra_index=0):
    """One es_adam_step in fp64 -> (p, m, v, update).  The betas and eps are rounded to fp32 first and 1 - beta is taken from the rounded
    value: that is the Adam the C ABI's ``float`` arguments define (an exact Adam with beta2 = fl32(0.999)).  step_size, bc2_sqrt and
    grad_scale are ``float`` arguments too."""
    p, g, m, v = d64(p), d64(g).clone(), d64(m), d64(v)
    b1, b2, eps = fl32(beta1), fl32(beta2), fl32(eps)
    if extra is not None:
        g[extra_index] += float(d64(extra).reshape(-1)[0])
    g = g * fl32(grad_scale)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    upd = fl32(step_size) * (m / (v.sqrt() / fl32(bc2_sqrt) + eps))
    return p - upd, m, v, upd
