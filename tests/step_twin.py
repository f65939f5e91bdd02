"""numpy fp32 twins of the training-step glue kernels: the same operations in the same order as the HIP source, once with every
``a * b + c`` rounded twice and once with the multiply-adds fused (what -ffp-contract=fast allows the compiler to do; the fused result is
formed in double, where the product of two fp32 numbers is exact, and rounded to fp32: a double rounding that differs from a true fma
about once in 2^29).  Sums follow the kernels' order: per-thread stride of 1024, six butterfly levels, sixteen partials.

The twins are NOT references.  tests/test_step_ref_host.py uses them to prove that the gates of step_cases.py can be met by the
kernels' own arithmetic: a twin must stay below half of every gate on every input set."""
import numpy as np

F = np.float32
E6, E10, HALF, ONE, ZERO = F(1e-6), F(1e-10), F(0.5), F(1.0), F(0.0)


class Ops:
    def __init__(self, fused):
        self.fused = fused

    def fma(self, a, b, c):
        """a * b + c"""
        if self.fused:
            return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)
        return (np.asarray(a, F) * np.asarray(b, F)).astype(F) + np.asarray(c, F)

    def dot3(self, a, b):
        """a0 b0 + a1 b1 + a2 b2, left to right"""
        return self.fma(a[..., 2], b[..., 2], self.fma(a[..., 1], b[..., 1], a[..., 0] * b[..., 0]))


def sgn(x):
    return np.sign(x).astype(F)


def block_sum(vals):
    """vals [N] or [N, K] (K adds per row, in order): the sum as a 1024-thread workgroup forms it."""
    vals = np.asarray(vals, F)
    if vals.ndim == 1:
        vals = vals[:, None]
    N, K = vals.shape
    trips = max((N + 1023) // 1024, 1)
    pad = np.zeros((trips * 1024, K), F)
    pad[:N] = vals
    pad = pad.reshape(trips, 1024, K)
    s = np.zeros(1024, F)
    for t in range(trips):
        for k in range(K):
            s = s + pad[t, :, k]
    w = s.reshape(16, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[:, lane ^ o]
    tot = F(0.0)
    for i in range(16):
        tot = tot + w[i, 0]
    return F(tot)


# ---- points -----------------------------------------------------------------------------------------------------------------------------
def aux_points(op, rays, depth_gt, mask, d_i, u, rad):
    """k_train_aux_points -> x [3N,3], valid [N], inside [N] (k_eod_points' optional output, from its own fp32 point)."""
    r = np.asarray(rays, F)
    N = r.shape[0]
    inv = r[:, 5:6] + E6
    dz = r[:, 3:6] / inv
    di = np.asarray(d_i, F).reshape(N, 1)
    m = np.asarray(mask, F).reshape(N, 1)
    ok = np.isfinite(di) & (di != 0) & (m == 1)
    ds = np.where(ok, di, ZERO).astype(F)
    ps = op.fma(ds, dz, r[:, :3])
    xe = op.fma(dz, np.asarray(depth_gt, F).reshape(N, 1), r[:, :3])
    xn = op.fma(np.asarray(u, F) - HALF, F(rad), ps)
    nrm2 = op.fma(xe[:, 2], xe[:, 2], op.fma(xe[:, 1], xe[:, 1], xe[:, 0] * xe[:, 0]))
    inside = (np.sqrt(nrm2) < ONE).astype(F) * m[:, 0]
    return np.concatenate([xe, ps, xn], 0), ok[:, 0], inside


# ---- errorondepth ---------------------------------------------------------------------------------------------------------------------------
def _inside(op, pts, mask):
    p = np.asarray(pts, F)
    nrm2 = op.fma(p[:, 2], p[:, 2], op.fma(p[:, 1], p[:, 1], p[:, 0] * p[:, 0]))
    return (np.sqrt(nrm2) < ONE).astype(F) * np.asarray(mask, F).reshape(-1)


def eod_loss(op, rays, pts, mask, sdf, go):
    r, go = np.asarray(rays, F), np.asarray(go, F)
    inside = _inside(op, pts, mask)
    s0 = block_sum(np.abs(inside * np.asarray(sdf, F).reshape(-1)))
    s1 = block_sum(inside)
    s2 = block_sum(np.maximum(op.dot3(r[:, 3:6], go), ZERO))
    den = s1 + E6
    return dict(sdf_err=s0 / den, ang_err=s2 / den, den=den, inside=inside)


def eod_loss_bwd(op, rays, inside, sdf, go, den, gs, ga):
    r, go = np.asarray(rays, F), np.asarray(go, F)
    gs, ga = F(gs), F(ga)
    d_sdf = gs * sgn(inside * np.asarray(sdf, F).reshape(-1)) * inside / den
    cs = op.dot3(r[:, 3:6], go)
    k = np.where(cs > 0, ga / den, ZERO).astype(F)
    return dict(d_sdf=d_sdf, d_go=k[:, None] * r[:, 3:6])


# ---- surface neighbours ---------------------------------------------------------------------------------------------------------------------
def _norm(op, g):
    return np.sqrt(op.fma(g[:, 2], g[:, 2], op.fma(g[:, 1], g[:, 1], g[:, 0] * g[:, 0])))


def sn_sums(op, g, valid):
    g = np.asarray(g, F)
    N = g.shape[0] // 2
    v = np.asarray(valid).astype(bool)
    n1, n2 = _norm(op, g[:N]) + E10, _norm(op, g[N:]) + E10
    diff = np.abs(g[:N] / n1[:, None] - g[N:] / n2[:, None]) * v[:, None].astype(F)
    return block_sum(diff), block_sum(v.astype(F))


def sn_loss(op, g, valid):
    s0, s1 = sn_sums(op, g, valid)
    den = np.maximum(F(3.0) * s1, ONE)
    return dict(loss=s0 / den, den=den)


def sn_bwd_rows(op, g, valid, scale):
    """The rows [0,2N) of the surface-neighbour adjoint for nbar = scale * sgn(n1 - n2) (scale in fp32, formed by the caller)."""
    g = np.asarray(g, F)
    N = g.shape[0] // 2
    v = np.asarray(valid).astype(bool)[:, None]
    g1, g2 = g[:N], g[N:]
    r1, r2 = _norm(op, g1)[:, None], _norm(op, g2)[:, None]
    d1, d2 = r1 + E10, r2 + E10
    n1, n2 = g1 / d1, g2 / d2
    nb = scale(sgn(n1 - n2))
    dot1 = np.zeros(N, F)
    dot2 = np.zeros(N, F)
    for k in range(3):
        dot1 = op.fma(n1[:, k], nb[:, k], dot1)
        dot2 = op.fma(n2[:, k], nb[:, k], dot2)
    with np.errstate(divide="ignore", invalid="ignore"):
        a1 = op.fma(-(n1 * dot1[:, None]), d1 / r1, nb) / d1
        a2 = -(op.fma(-(n2 * dot2[:, None]), d2 / r2, nb)) / d2
    o1 = np.where(r1 > 0, a1, nb / d1)
    o2 = np.where(r2 > 0, a2, -nb / d2)
    return np.concatenate([np.where(v, o1, ZERO), np.where(v, o2, ZERO)], 0).astype(F)


def sn_loss_bwd(op, g, valid, den, g_loss):
    s = F(g_loss) / F(den)
    return sn_bwd_rows(op, g, valid, lambda sg: s * sg)


# ---- the training loss ---------------------------------------------------------------------------------------------------------------------
def train_loss(op, inp, w, den_global=None, world=1.0):
    """k_train_loss -> {terms [8], den [4], g_color, g_depth, g_aux_sdf, g_aux_go}"""
    N = inp["rays"].shape[0]
    f = lambda k: np.asarray(inp[k], F)
    r, go, sdf = f("rays"), f("aux_go"), f("aux_sdf").reshape(-1)
    cm, m = f("cmask").reshape(-1), f("mask").reshape(-1)
    cerr = (f("color_map") - f("color_gt")) * cm[:, None]
    inside = _inside(op, inp["eod_pts"], m)
    cs = op.dot3(r[:, 3:6], go[:N])
    v = inside * m
    derr = (f("depth_map").reshape(-1) - f("depth_gt").reshape(-1)) * v
    s7, s8 = sn_sums(op, go[N:], inp["valid_sn"])
    sums = [block_sum(np.abs(cerr)), block_sum(cm), block_sum(np.abs(inside * sdf[:N])), block_sum(inside), block_sum(np.maximum(cs, ZERO)),
            block_sum(np.abs(derr)), block_sum(v), s7, s8]
    den = [sums[1], sums[3], sums[6], sums[8]]
    dg = den if den_global is None else [F(x) for x in den_global]
    ws = F(world if den_global is not None else 1.0)
    den_c, den_i, den_d = (dg[0] + E10) / ws, (dg[1] + E6) / ws, (dg[2] + E10) / ws
    den_sn = np.maximum(F(3.0) * dg[3], ONE) / ws
    wf = {k: F(w[k]) for k in w}
    t = [sums[0] / den_c, sums[5] / den_d, sums[2] / den_i, sums[4] / den_i, F(f("eik").reshape(-1)[0]), sums[7] / den_sn]
    tot = wf["color"] * t[0]
    for k, i in (("depth", 1), ("sdf", 2), ("angle", 3), ("eikonal", 4), ("surf_neig", 5)):
        tot = op.fma(wf[k], t[i], tot)
    g_color = wf["color"] * sgn(cerr) * cm[:, None] / den_c
    g_sdf = np.zeros(3 * N, F)
    g_sdf[:N] = wf["sdf"] * sgn(inside * sdf[:N]) * inside / den_i
    ga = np.where(cs > 0, wf["angle"] / den_i, ZERO).astype(F)
    g_depth = wf["depth"] * sgn(derr) * v / den_d
    g_go = np.concatenate([ga[:, None] * r[:, 3:6], sn_bwd_rows(op, go[N:], inp["valid_sn"], lambda sg: wf["surf_neig"] * sg / den_sn)], 0)
    return dict(terms=np.asarray(t + [tot, s8], F), den=np.asarray(den, F), g_color=g_color, g_depth=g_depth[:, None], g_aux_sdf=g_sdf[:, None],
                g_aux_go=g_go)


# ---- Adam --------------------------------------------------------------------------------------------------------------------------------
def adam(op, p, g, m, v, beta1, beta2, eps, step_size, bc2_sqrt, grad_scale, extra=None, extra_index=0):
    p, g, m, v = (np.asarray(a, F).copy() for a in (p, g, m, v))
    b1, b2 = F(beta1), F(beta2)
    if extra is not None:
        g[extra_index] = g[extra_index] + F(np.asarray(extra).reshape(-1)[0])
    g = g * F(grad_scale)
    mi = op.fma(b1, m, (ONE - b1) * g)
    vi = op.fma(b2, v, (ONE - b2) * g * g)
    denom = np.sqrt(vi) / F(bc2_sqrt) + F(eps)
    return op.fma(-F(step_size), mi / denom, p), mi, vi
