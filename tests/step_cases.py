"""Input sets and derived gates of the training-step glue kernels' parity tests.  tests/test_gpu_step_kernels.py runs the kernels on
these inputs; tests/test_step_ref_host.py runs the numpy fp32 twins of the kernels on the SAME inputs and requires them to stay below
half of every gate (a gate the kernel's own arithmetic cannot meet is a wrong derivation).  No GPU, no library.

Gates are derived from the arithmetic, not measured.  Unit: u = 2^-24.  Every function returns the ALLOWED absolute error, elementwise,
from fp64 reference quantities only."""
import math

import numpy as np
import torch

import step_ref as R

U = R.U
F32 = np.float32

POINT_N = (1, 255, 256, 257, 1000)
LOSS_N = (1, 37, 1023, 1024, 1025, 3000)
ADAM_N = (1, 255, 256, 257, 100003)
FINISH_N = (0, 1, 85, 86, 3072)
COPY2 = ((0, 0), (0, 5), (777, 3 * 777), (256, 255), (1, 100000))
LOSS_W = dict(color=1.0, depth=0.7, sdf=0.3, angle=0.2, eikonal=0.1, surf_neig=0.05)
ONE_IN = float(np.nextafter(F32(1), F32(0)))          # the largest fp32 below 1


def depth_c(N, k):
    """Gate B's factor: summation depth of a single-workgroup kernel (ceil(N/1024) strided trips per thread, 6 butterfly levels, 16
    partials) + k roundings inside one term."""
    return (N + 1023) // 1024 + 22 + k


# ---- points -------------------------------------------------------------------------------------------------------------------------
def points_inputs(N, seed=0):
    """Rays with |d.z| >= 0.3 (d.z < 0 on every third row), d_i over {+inf, -inf, nan, 0, -0, negative, hits}, mask over {0, 1, 0.5,
    nextafter(1, 2)}, origins exactly on and just inside the unit sphere with depth_gt == 0.  Drawn errorondepth points within 1e-5 of
    the sphere are redrawn (the count is returned): fp32 and fp64 may disagree about |x| < 1 there."""
    rng = np.random.default_rng(1000 + 7 * N + seed)
    o = rng.uniform(-0.5, 0.5, (N, 3))
    d = np.concatenate([0.3 * rng.standard_normal((N, 2)), rng.uniform(0.3, 1.0, (N, 1))], 1)
    d[::3] *= -1.0
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([o, d, np.zeros((N, 2)), rng.uniform(0, 1, (N, 1))], 1).astype(F32)
    depth = rng.uniform(-0.2, 1.6, N).astype(F32)
    d_i = rng.uniform(0.1, 1.5, N).astype(F32)
    special = [np.inf, -np.inf, np.nan, 0.0, -0.0, -0.7]
    for j, v in enumerate(special):
        d_i[(2 + j)::11] = v
    mask = np.ones(N, F32)
    for j, v in enumerate([0.0, 0.5, float(np.nextafter(F32(1), F32(2)))]):
        mask[(1 + j)::5] = v
    sphere = [(1, 0, 0), (0, -1, 0), (0, 0, 1), (ONE_IN, 0, 0), (0, -ONE_IN, 0), (0, 0, ONE_IN)]
    rows = [0] if N == 1 else [r for r in (0, 6, 12, 18, 24, 30) if r < N]
    for r, s in zip(rows, sphere):
        rays[r, :3] = s
        depth[r] = 0.0
        mask[r] = 1.0
        d_i[r] = 0.8
    redraws = 0
    for _ in range(100):
        x = R.aux_points(rays, depth, mask, d_i, np.zeros((N, 3), F32), 0.0)[0][:N]
        near = (x.norm(dim=-1) - 1.0).abs().numpy() < 1e-5
        near[rows] = False
        if not near.any():
            break
        redraws += int(near.sum())
        depth[near] = rng.uniform(-0.2, 1.6, int(near.sum())).astype(F32)
    else:
        raise AssertionError("screening did not converge")
    u = rng.uniform(0, 1, (N, 3)).astype(F32)
    return dict(rays=rays, depth_gt=depth, mask=mask, d_i=d_i, u=u, rad=0.1, redraws=redraws, sphere_rows=rows)


def gate_points(inp):
    """Gate A.  x = o + (d / (d.z + 1e-6)) * s: the sum of d.z and 1e-6 (no cancellation: |d.z| >= 0.3), the quotient, the product and the
    final sum round once each, fused or not: <= u |x| + 3 u |dz s| to first order; with the fp32 constant 1e-6f and second-order terms,
    2 u (|x| + 4 |dz s|).
    A neighbour row is the ROUNDED surface point plus (u - 0.5) * rad.  It inherits the surface row's allowance (the surface point can be
    larger than the neighbour: its rounding does not shrink with |x_n|); the offset rounds twice (the difference: u has a finer grid than
    u - 0.5; the product), 2 u |off| on its own and 4 u |off| with the same factor two of headroom; the new sum rounds once: 2 u |x_n|.
    (The first form of this gate, 2 u (|x_n| + 4 |dz s|) + 2 u |off|, counted one rounding of the offset and none of the surface point:
    the fp32 twin reaches 0.76 of it on an invalid ray, whose surface point is the origin itself, and 0.64 on ordinary ones.)"""
    rays, N = R.d64(inp["rays"]), inp["rays"].shape[0]
    x, _, valid, _ = R.aux_points(inp["rays"], inp["depth_gt"], inp["mask"], inp["d_i"], inp["u"], inp["rad"])
    dz = rays[:, 3:6] / (rays[:, 5:6] + 1e-6)
    s_eod = R.d64(inp["depth_gt"]).reshape(N, 1)
    s_sn = torch.where(valid[:, None], R.d64(inp["d_i"]).reshape(N, 1), torch.zeros(N, 1, dtype=R.F64))
    off = ((R.d64(inp["u"]) - 0.5) * R.fl32(inp["rad"])).abs()
    steps = torch.cat([dz * s_eod, dz * s_sn, dz * s_sn], 0).abs()
    g = 2 * U * (x.abs() + 4 * steps)
    g[2 * N:] = g[N:2 * N] + 2 * U * x[2 * N:].abs() + 4 * U * off
    return g


# ---- errorondepth's reductions ---------------------------------------------------------------------------------------------------------
def eod_inputs(N, variant="mixed", seed=0):
    """variant: mixed | none_inside (denominator 1e-6, the sdf term and its adjoint exactly 0) | all_inside."""
    rng = np.random.default_rng(2000 + 7 * N + seed)
    rays = rng.standard_normal((N, 9)).astype(F32)
    pts = (0.7 * rng.standard_normal((N, 3))).astype(F32)
    if variant == "none_inside":
        pts = (pts + np.sign(pts + 1e-3) * 1.0).astype(F32)
    if variant == "all_inside":
        pts = (0.3 * np.tanh(pts)).astype(F32)
    redraws = 0
    while True:
        near = np.abs(np.linalg.norm(pts.astype(np.float64), axis=1) - 1.0) < 1e-5
        if not near.any():
            break
        redraws += int(near.sum())
        pts[near] = (1.3 * pts[near]).astype(F32)
    mask = (rng.uniform(size=(N, 1)) < 0.8).astype(F32)
    mask[3::17] = 0.5
    if variant == "all_inside":
        mask[:] = 1.0
    sdf = rng.standard_normal((N, 1)).astype(F32)
    go = rng.standard_normal((N, 3)).astype(F32)
    if variant != "none_inside" and N >= 4:
        pts[1] = (0.1, 0.2, 0.3); mask[1] = 1.0; sdf[1] = 0.0                 # sdf exactly 0 on an inside row: sgn(0) = 0
        rays[2, 3:6] = (1, 0, 0); go[2] = (0, 1, 0)                           # d . g_o exactly 0: relu'(0) = 0
        pts[3] = (-0.2, 0.1, 0.0); mask[3] = 1.0; sdf[3] = -0.75              # inside * sdf negative
    return dict(rays=rays, pts=pts, mask=mask, sdf=sdf, go=go, redraws=redraws)


def _cos_parts(rays, go):
    """cos = d . g_o in fp64 and sum_k |d_k g_k|, the magnitude its three roundings (two when fused) are relative to."""
    p = R.d64(rays)[:, 3:6] * R.d64(go)
    return p.sum(-1), p.abs().sum(-1)


def gate_eod(inp, ref):
    """Gate B for es_eod_loss's out[3] = {sdf_err, ang_err, den}.  den = sum(inside) + 1e-6f: the sum is exact (multiples of 0.5 below
    2^24), the constant and the addition round: 2 u.  sdf term |inside * sdf|: one product, k = 1, + 2 for den + 1 for the division.
    angle term relu(cos): the three products and two sums of cos are relative to sum_k |d_k g_k|, not to cos (cancellation), so that part
    is 3 u sum_i sum_k |d_k g_k| / den on its own, and k = 3 (den, division) for the rest."""
    N = inp["rays"].shape[0]
    _, mag = _cos_parts(inp["rays"], inp["go"])
    den = float(ref["den"])
    return dict(sdf_err=depth_c(N, 4) * U * float(ref["sdf_err"]),
                ang_err=depth_c(N, 3) * U * float(ref["ang_err"]) + 3 * U * float(mag.sum()) / den,
                den=2 * U * den)


def gate_eod_bwd(inp, ref, gs, ga):
    """Gate C.  d_sdf = gs * sgn(inside * sdf) * inside / den: the products are exact (inside in {0, 0.5, 1}; the sign of a product of two
    floats is exact), den carries 2 u and the division 1 u: 4 u |d_sdf|.  d_go = (ga / den) * d where cos > 0: 2 u (den) + the division +
    the product: 5 u |ga / den| |d_k|; a row whose |cos| is below the 3 u sum_k |d_k g_k| its own rounding can reach may take either
    branch, so there the allowance is the whole |ga / den| |d_k|."""
    cs, mag = _cos_parts(inp["rays"], inp["go"])
    den = float(ref["den"])
    full = abs(ga) / den * R.d64(inp["rays"])[:, 3:6].abs()
    either = (cs.abs() <= 3 * U * mag) & (mag > 0) & (cs != 0)
    return dict(d_sdf=4 * U * ref["d_sdf"].abs(), d_go=5 * U * ref["d_go"].abs() + either[:, None].to(R.F64) * full)


# ---- surface_neighbour_error's reduction -----------------------------------------------------------------------------------------------
def sn_inputs(N, variant="mixed", seed=0):
    """variant: mixed | none_valid | all_valid.  Zero gradient rows: one on the surface side, one on the neighbour side, one row with
    both zero (all three valid)."""
    rng = np.random.default_rng(3000 + 7 * N + seed)
    g = (rng.standard_normal((2 * N, 3)) * 10.0 ** rng.uniform(-2, 1, (2 * N, 1))).astype(F32)
    valid = rng.uniform(size=N) < 0.6
    if variant == "none_valid":
        valid[:] = False
    if variant == "all_valid":
        valid[:] = True
    if variant != "none_valid" and N >= 8:
        g[5] = 0.0; g[N + 6] = 0.0; g[7] = 0.0; g[N + 7] = 0.0
        valid[5:8] = True
    if variant != "none_valid" and N >= 2:
        valid[0] = True
        valid[1] = variant == "all_valid"               # an invalid row next to a valid one
    if variant == "mixed" and N == 1:
        valid[0] = True
    return dict(g=g, valid=valid)


def _normals(g1, g2):
    q1 = g1 / (g1.norm(dim=-1, keepdim=True) + 1e-10)
    q2 = g2 / (g2.norm(dim=-1, keepdim=True) + 1e-10)
    return q1, q2


def sn_term_gate(g, valid, N, den, extra_k=0, N_depth=None):
    """Gate B for the surface-neighbour sum.  One quotient q = g_k / (|g| + 1e-10f): the sum of squares carries <= 3 u (three products, two
    sums, all terms positive), its root 1.5 u + 1 u, the fp32 constant and its addition 2 u, the division 1 u: <= 5.5 u |q|, say 6.  The
    difference q1 - q2 cancels, so these 6 u are relative to |q1| + |q2|, not to the term; the difference itself rounds once more
    (k = 1), the denominator max(3 n, 1) is exact, the final division rounds once (k = 2)."""
    gg = R.d64(g)
    q1, q2 = _normals(gg[:N], gg[N:])
    v = torch.as_tensor(np.asarray(valid)).bool()[:, None].to(R.F64)
    mag = float(((q1.abs() + q2.abs()) * v).sum())
    S = float(((q1 - q2).abs() * v).sum())
    return (depth_c(N if N_depth is None else N_depth, 2 + extra_k) * U * S + 6 * U * mag) / den


def sn_bwd_gate(g, valid, N, scale, sign_k=1):
    """Gate C for gbar = (nbar - n (n . nbar) d / r) / d with n = g / d, d = r + 1e-10f, nbar_k = scale * sgn(n1_k - n2_k), gated on
    |nbar|_1 / d (|n| <= 1, so both terms of the numerator are below |nbar|_1):
      scale (one division, ``sign_k`` roundings) and n_k (6 u, above); the dot product's three products and two sums: 6 + 1 + 2 u;
      d / r: 3.5 u + 2.5 u + 1 u; the two products of n (n . nbar) (d / r): 2 u  => the second term carries <= (6 + 9 + 7 + 2) u |nbar|_1;
      the subtraction 1 u of both terms (2 u |nbar|_1), the final division 1 u + d's 3.5 u on both terms (9 u |nbar|_1)
    => 36 u |nbar|_1 / d with scale's own rounding.  A component whose |q1 - q2| is below the 6 u (|q1| + |q2|) its rounding can reach
    may get either sign: there nbar_k may be off by 2 |scale|, which reaches every component of the row through the dot product:
    + 2 |scale| (1 + 1) / d."""
    gg = R.d64(g)
    q1, q2 = _normals(gg[:N], gg[N:])
    v = torch.as_tensor(np.asarray(valid)).bool()[:, None].to(R.F64)
    nb1 = (scale * torch.sign(q1 - q2)).abs().sum(-1, keepdim=True)
    flip = (((q1 - q2).abs() <= 6 * U * (q1.abs() + q2.abs())) & (q1 != q2)).any(-1, keepdim=True).to(R.F64)
    d = torch.cat([gg[:N].norm(dim=-1, keepdim=True), gg[N:].norm(dim=-1, keepdim=True)], 0) + 1e-10
    per_row = ((35 + sign_k) * U * nb1 + flip * 4 * abs(scale)) * v
    return torch.cat([per_row, per_row], 0) / d * torch.ones(1, 3, dtype=R.F64)


# ---- the training loss ---------------------------------------------------------------------------------------------------------------------
def loss_inputs(N, variant="mixed", seed=0):
    """All inputs of es_train_loss.  variant: mixed (every degenerate population of the stand-alone kernels in one launch, colour errors
    exactly 0 on some entries) | masks_zero (cmask and mask all zero) | none_valid | all_valid."""
    rng = np.random.default_rng(4000 + 7 * N + seed)
    e = eod_inputs(N, "mixed", seed + 1)
    s = sn_inputs(N, {"none_valid": "none_valid", "all_valid": "all_valid"}.get(variant, "mixed"), seed + 2)
    color_map, color_gt = rng.uniform(size=(N, 3)).astype(F32), rng.uniform(size=(N, 3)).astype(F32)
    color_gt[::4, 1] = color_map[::4, 1]                                    # sgn(0) = 0
    depth_map, depth_gt = (1.2 + 0.3 * rng.standard_normal((N, 1))).astype(F32), (1.2 + 0.3 * rng.standard_normal((N, 1))).astype(F32)
    depth_gt[::5] = depth_map[::5]
    cmask = (rng.uniform(size=(N, 1)) < 0.6).astype(F32)
    mask = e["mask"].copy()
    if variant == "masks_zero":
        cmask[:] = 0.0; mask[:] = 0.0
    a_sdf = np.concatenate([e["sdf"], (0.1 * rng.standard_normal((2 * N, 1))).astype(F32)], 0)
    a_go = np.concatenate([e["go"], s["g"]], 0)
    return dict(color_map=color_map, depth_map=depth_map, eik=np.asarray([0.0371], F32), aux_sdf=a_sdf, aux_go=a_go, rays=e["rays"], eod_pts=e["pts"],
                color_gt=color_gt, depth_gt=depth_gt, mask=mask, cmask=cmask, valid_sn=s["valid"], redraws=e["redraws"])


LOSS_ARGS = ("color_map", "depth_map", "eik", "aux_sdf", "aux_go", "rays", "eod_pts", "color_gt", "depth_gt", "mask", "cmask", "valid_sn")


def loss_ref(inp, w=LOSS_W, den_global=None, world=1.0):
    return R.train_loss(*[inp[k] for k in LOSS_ARGS], w, den_global, world)


def cat3(a, b):
    """[3Na, ...] and [3Nb, ...] auxiliary rows -> the [3 (Na + Nb), ...] rows of the concatenated batch (block by block)."""
    na, nb = a.shape[0] // 3, b.shape[0] // 3
    cat = torch.cat if torch.is_tensor(a) else np.concatenate
    return cat([a[:na], b[:nb], a[na:2 * na], b[nb:2 * nb], a[2 * na:], b[2 * nb:]], 0)


def concat_parts(a, b):
    out = {}
    for k in LOSS_ARGS:
        if k == "eik":
            out[k] = a[k]
        elif k in ("aux_sdf", "aux_go"):
            out[k] = cat3(a[k], b[k])
        else:
            out[k] = np.concatenate([a[k], b[k]], 0)
    return out


def gate_loss_terms(inp, ref, N_depth=None, world=1.0):
    """Gate B for the six terms and the total (``ref``: step_ref.train_loss of the same inputs).  Normalisers: sum + constant, 2 u, one more
    division by the world size in exact mode (exact for a power of two, counted anyway): den_k = 3.
      color  |(a - b) * cm|: the difference rounds (cm is 0 or 1): k = 1 + den_k + 1 (division)
      sdf    k = 1 + den_k + 1;   depth |(a - b) * v|: k = 2 + den_k + 1
      angle  as in gate_eod;  surf_neig as in sn_term_gate (its denominator is exact but for the world division: extra_k = 1)
      eikonal is copied: 0.  total = sum_k w_k term_k: six products and five sums, each below u sum |w_k term_k|: + 12 u sum |w_k term_k|
    on top of sum_k |w_k| gate_k."""
    N = inp["rays"].shape[0]
    Nd = N if N_depth is None else N_depth
    t = {k: float(v) for k, v in ref["terms"].items()}
    _, mag = _cos_parts(inp["rays"], inp["aux_go"][:N])
    gate = dict(color=depth_c(Nd, 5) * U * t["color"], sdf=depth_c(Nd, 5) * U * t["sdf"], depth=depth_c(Nd, 6) * U * t["depth"], eikonal=0.0)
    den_i = ref["den_used"][1] + 1e-6
    gate["angle"] = depth_c(Nd, 4) * U * t["angle"] + 3 * U * world * float(mag.sum()) / den_i
    gate["surf_neig"] = world * sn_term_gate(inp["aux_go"][N:], inp["valid_sn"], N, max(3.0 * ref["den_used"][3], 1.0), extra_k=1, N_depth=Nd)
    w = ref["w"]
    gate["total"] = sum(abs(w[k]) * gate[k] for k in R.LOSS_KEYS) + 12 * U * sum(abs(w[k] * t[k]) for k in R.LOSS_KEYS)
    return gate


def gate_loss_grads(inp, ref, world=1.0):
    """Gate C for the adjoints of es_train_loss.  g_color = w sgn((a - b) cm) cm / den_c, g_depth, g_aux_sdf[:N]: exact products, den 3 u,
    one division: 5 u |ref|.  g_aux_go[:N] = (w / den_i) d_k: 6 u, either branch where |cos| is within its own rounding (gate_eod_bwd).
    Rows [N, 3N) of g_aux_go: sn_bwd_gate with scale = w_sn / den_sn (two roundings).  g_eik and rows [N, 3N) of g_aux_sdf are exact."""
    N = inp["rays"].shape[0]
    w = ref["w"]
    cs, mag = _cos_parts(inp["rays"], inp["aux_go"][:N])
    den_i = ref["den_used"][1] + 1e-6
    full = world * abs(w["angle"]) / den_i * R.d64(inp["rays"])[:, 3:6].abs()
    either = ((cs.abs() <= 3 * U * mag) & (mag > 0) & (cs != 0))[:, None].to(R.F64)
    scale = world * w["surf_neig"] / max(3.0 * ref["den_used"][3], 1.0)
    g_go = torch.cat([6 * U * ref["g_aux_go"][:N].abs() + either * full, sn_bwd_gate(inp["aux_go"][N:], inp["valid_sn"], N, scale, sign_k=2)], 0)
    return dict(g_color=5 * U * ref["g_color"].abs(), g_depth=5 * U * ref["g_depth"].abs(), g_aux_sdf=5 * U * ref["g_aux_sdf"].abs(), g_aux_go=g_go)


# ---- Adam ------------------------------------------------------------------------------------------------------------------------------
ADAM_HP = dict(beta1=0.9, beta2=0.999, eps=1e-8, lr=3e-4)


def adam_inputs(n, seed=0):
    """p, and seven gradients with scales 1e-4 ... 10; a block of exactly-zero gradients at step 3; per-step grad_scale 0.25 / 1; one extra
    scalar per step."""
    rng = np.random.default_rng(5000 + n + seed)
    p = rng.standard_normal(n).astype(F32)
    scales = [1e-4, 1e-3, 1e-2, 1e-1, 1.0, 10.0, 3e-2]
    grads = [(rng.standard_normal(n) * s).astype(F32) for s in scales]
    grads[2][(n // 3):(n // 3) + 70] = 0.0
    if n == 1:
        grads[2][:] = 0.0
    extras = [np.asarray([rng.standard_normal()], F32) for _ in scales]
    gscale = [0.25 if t % 2 else 1.0 for t in range(1, 8)]
    return dict(p=p, grads=grads, extras=extras, grad_scale=gscale)


def adam_scalars(t, hp=ADAM_HP):
    return hp["lr"] / (1.0 - hp["beta1"] ** t), math.sqrt(1.0 - hp["beta2"] ** t)


def gate_adam(ref_p, ref_m, ref_v, upd, g_eff, beta1):
    """Gate D (per step, both sides start from the same fp32 state):
      v = b2 v + (1 - b2) g g: at most four roundings of positive terms            => 8 u |v|
      m = b1 m + (1 - b1) g: three roundings, relative to the larger operand       => 8 u max(|m|, |(1 - b1) g|)
      update = step (m / (sqrt(v) / bc2 + eps)): m 3 u (when it does not cancel), v/2 2 u, root, division, sum, division, product 5 u
      p - update: u |p|                                                              => 2 u (|p| + 8 |update|)"""
    b1 = R.fl32(beta1)
    return (2 * U * (ref_p.abs() + 8 * upd.abs()), 8 * U * torch.maximum(ref_m.abs(), ((1.0 - b1) * g_eff).abs()), 8 * U * ref_v.abs())


# ---- schedule ------------------------------------------------------------------------------------------------------------------------------
def schedule_cases():
    """(name, start state, steps, kwargs): every step of two short schedules x three anneal_end, the saturated bias corrections, a start
    with different counters."""
    out = []
    for warm in (4, 0):
        for anneal in (0, 6, 50000):
            out.append((f"w{warm}_a{anneal}", (0.0, 0.0), 45, dict(lr_init=1e-3, n_iter=40, warm_up_end=warm, lr_alpha=0.05, anneal_end=anneal)))
    out.append(("saturated", (99998.0, 99998.0), 3, dict(lr_init=5e-4, n_iter=100000, warm_up_end=5000, lr_alpha=0.05, anneal_end=50000)))
    out.append(("split_counters", (10.0, 3.0), 5, dict(lr_init=1e-3, n_iter=40, warm_up_end=12, lr_alpha=0.05, anneal_end=6)))
    return out
