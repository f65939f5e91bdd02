"""The hand-written backward against autograd on the fp64 oracle AWAY from the two shapes of test_gpu_backward.py (M = 200 points,
48 rays x 64 samples): the shapes at which its launch geometry changes.

  A  dense point-count sweep of the point backward (chains + weight gradients): every pad-row count of a 128-row workspace, the
     weight-gradient row-chunk counts 8 / 16 (paired layout only), 9 / 18 and 11 / 22 (paired + remainder) in atomic and deterministic
     mode, and a small launch into a workspace that is not fresh memory
  B  the launch sizes the oracle cannot be given (20 031 points; the fused training launch 65 536 + 3 072 with a colour-less tail): the
     upstream adjoints are non-zero on a few hundred rows only, so the full-size gradient must equal the oracle's on those rows alone
  C  compositing forward + backward at S = 32 ... 256 samples per ray (one to four 64-lane chunks) on synthetic per-sample inputs
  D  render-level parameter gradients at 64 + 64 samples (config 3) and at 32 samples before importance sampling starts
  E  up-sampling / stable merge on tied and flat inputs

The reference of every comparison is the oracle in fp64, never a second run of the kernels."""
import numpy as np
import pytest
import torch

import weightgen
from gpu_util import renderer_for
from oracle import endosurf_oracle as O
from oracle_util import RENDER_CFG
from shapes_util import SEED, inputs as _inputs, split_chain
from test_gpu_backward import FLOOR, POINT_TOL, _dump, _grad_table

pytestmark = pytest.mark.gpu

_RENDERERS, _ORACLE = {}, {}
# oracle passes that two cases share (atomic + deterministic mode, the workspace-history case): kept; every other one is dropped after use
REUSED = {("dense", True, 65, True), ("dense", True, 1024, True), ("dense", True, 1100, True), ("dense", True, 1400, True),
          ("sparse", "train_68608_deform")}


def _renderer(use_deform):
    """One renderer (one engine, one caching allocator history) per network layout for the whole module: no case but the first sees
    fresh workspace memory."""
    if use_deform not in _RENDERERS:
        _RENDERERS[use_deform] = renderer_for(SEED, "trained", use_deform)
    r = _RENDERERS[use_deform]
    r.engine.deterministic = False
    return r


def _oracle_params(use_deform, dtype=torch.float64):
    state = weightgen.make_state(SEED, "trained", use_deform)
    params = {k: torch.tensor(v, dtype=dtype, requires_grad=True) for k, v in state.items()}
    return O.OracleNet(params, use_deform), params


def _oracle_point_grads(key, use_deform, x, d, t, ws, wg, wc, n_color):
    """fp64 autograd of sum(sdf ws) + sum(g_o wg) + sum(rgb wc): rows [0, n_color) go through the colour network, the rest do not.
    Cached per ``key``: the atomic and the deterministic run of one shape share the oracle's pass."""
    if key in _ORACLE:
        return _ORACLE[key]
    if True:
        net, params = _oracle_params(use_deform)
        f = lambda a: a.double()
        ref = torch.zeros((), dtype=torch.float64)
        for lo, hi, col in ((0, n_color, True), (n_color, x.shape[0], False)):
            if hi <= lo:
                continue
            pe = net.point_eval(f(x[lo:hi]), f(d[lo:hi]), f(t[lo:hi])[:, None], with_color=col)
            ref = ref + (pe["sdf"] * f(ws[lo:hi])).sum() + (pe["g_o"] * f(wg[lo:hi])).sum()
            if col:
                ref = ref + (pe["rgb"] * f(wc[lo:hi])).sum()
        ref.backward()
    if key in REUSED:
        _ORACLE[key] = (float(ref.detach()), params)
    return float(ref.detach()), params


def _hip_point_grads(r, x, d, t, ws, wg, wc, color, m_color=0, poison=None, split=False):
    """Engine.point_forward / point_backward / weightnorm_backward (through the renderer's packing node, so that the parameters' .grad
    are filled) on all rows of (x, d, t).  Returns (loss, pad rows of the x_c adjoint [Mp - M, 3]).  ``split``: forward and backward on
    the split-precision training chain (shapes_util.split_chain, restored behind the call); the context must say that it ran."""
    with split_chain(r.engine, split):
        return _hip_point_grads_on(r, x, d, t, ws, wg, wc, color, m_color, poison, split)


def _hip_point_grads_on(r, x, d, t, ws, wg, wc, color, m_color, poison, split):
    from endosurf_amd import _lib
    eng, M = r.engine, x.shape[0]
    for p in r.parameters():
        p.grad = None
    weff, packed = r._weights()
    assert weff.requires_grad
    flags = r._flags(weff) | (_lib.PF_COLOR if color else 0)
    assert flags & _lib.PF_SAVE
    dev = lambda a: a.cuda().contiguous()
    pts = eng.points(x=dev(x), t=dev(t), dirs=dev(d))
    if poison is not None:          # the workspace of this launch starts from ``poison`` in every word instead of whatever torch.empty returns
        plain = eng.empty
        eng.empty = lambda *s, **k: plain(*s, **k).fill_(poison)
    try:
        ctx = eng.point_forward(pts, weff.detach(), packed, flags, m_color)
    finally:
        if poison is not None:
            del eng.empty
    assert not split or (ctx.x3_chain and ctx.px3 is not None), "the split-precision training chain did not run"
    n_color = (m_color if m_color > 0 else M) if color else 0
    f = lambda a: a.double().cpu()
    loss = (f(ctx.view("sdf")) * ws.double()).sum() + (f(ctx.view("go")) * wg.double()).sum()
    if color:
        loss = loss + (f(ctx.view("rgb"))[:n_color] * wc.double()[:n_color]).sum()
    dweff = eng.point_backward(ctx, weff.detach(), packed, dev(ws), dev(wg), dev(wc[:n_color]) if color else None)
    weff.backward(dweff)
    torch.cuda.synchronize()
    off = int(eng.lib.es_point_workspace_offset(M, flags, _lib.WS_XCBAR))          # as PointCtx.view, without its [:M] cut
    pad = ctx.ws[off:off + ctx.Mp * 3].view(ctx.Mp, 3)[M:].clone()
    return float(loss), pad


def _check_point(r, params, loss, ref, pad, name=None):
    """The gates of test_point_backward (POINT_TOL: 5e-4 per parameter tensor, 1e-4 median, loss 2e-3) + the pad-row promise of
    csrc/workspace.h on the one adjoint buffer Python can see."""
    assert abs(loss - ref) < 2e-3 * max(1.0, abs(ref)), (loss, ref)
    rows = _grad_table(r, params)
    if name:
        _dump("shapes_" + name, rows)
    per_tensor, median = POINT_TOL["fp32"]
    bad = {k: v for k, v in rows.items() if v[0] > per_tensor and v[1] > 1e-7 and k != "deviation_network.variance"}
    assert not bad, bad
    live = [v[0] for v in rows.values() if v[1] > 1e-7]
    assert len(live) >= 20, len(live)          # (the cut excuses tensors without a gradient, not the comparison)
    assert float(np.median(live)) < median, float(np.median(live))
    if pad.numel():
        assert float(pad.abs().max()) == 0.0, ("pad rows of the x_c adjoint are not exact zeros", pad.abs().max(dim=1)[0].nonzero().flatten()[:8])
    return rows


# ------------------------------------------------------------------------------------------------------------------------------
# A. dense point-count sweep
# ------------------------------------------------------------------------------------------------------------------------------
DENSE = [(M, True) for M in (1, 63, 64, 65, 127, 129, 777)] + [(M, False) for M in (1, 65, 129)]


def _dense(use_deform, M, color, deterministic=False, poison=None, r=None, split=False):
    r = r or _renderer(use_deform)
    r.engine.deterministic = deterministic
    try:
        x, d, t, ws, wg, wc = _inputs(M, 1000 + M, use_deform)
        loss, pad = _hip_point_grads(r, x, d, t, ws, wg, wc, color, poison=poison, split=split)
    finally:
        r.engine.deterministic = False
    ref, params = _oracle_point_grads(("dense", use_deform, M, color), use_deform, x, d, t, ws, wg, wc, M if color else 0)
    return _check_point(r, params, loss, ref, pad,
                        name="x3_" * split + f"dense_{int(use_deform)}_{M}_{int(color)}" + ("_det" if deterministic else ""))


@pytest.mark.parametrize("use_deform", [True, False])
@pytest.mark.parametrize("M,color", DENSE)
def test_point_backward_pad_rows(use_deform, M, color):
    """Pad-row counts 127, 65, 64, 63, 1, 127, 119 of the 128-row workspace (and round_up64(M_color) != Mp at M = 65 / 129)."""
    _dense(use_deform, M, color)


@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("M", [1024, 1100, 1400])
def test_point_backward_row_chunks(M, deterministic):
    """8 / 16, 9 / 18 and 11 / 22 row chunks of 128 rows for the Mp- and 2 Mp-row weight-gradient problems: the paired task layout alone,
    paired + remainder; the deterministic reduce walks the same encoding.  Both modes against the oracle, not against each other."""
    _dense(True, M, True, deterministic=deterministic)


@pytest.mark.parametrize("poison", [None, float("nan")])
def test_point_backward_workspace_history(poison):
    """M = 65 right behind M = 1400 on one engine: the small launch's workspace is recycled memory (None), or is filled with NaN before
    the forward writes it (torch.empty promises nothing).  A pad row that is zero in fresh memory only shows up here."""
    r = _renderer(True)
    x, d, t, ws, wg, wc = _inputs(1400, 2400, screen=[])
    _hip_point_grads(r, x, d, t, ws, wg, wc, True)
    _dense(True, 65, True, poison=poison, r=r)


# ------------------------------------------------------------------------------------------------------------------------------
# B. colour-less tail, dense; sparse seeds at the launch sizes the oracle cannot be given
# ------------------------------------------------------------------------------------------------------------------------------
def _tail_dense(use_deform, tail, split=False):
    mc, M = 256, 256 + tail
    r = _renderer(use_deform)
    x, d, t, ws, wg, wc = _inputs(M, 3000 + M, use_deform)
    loss, pad = _hip_point_grads(r, x, d, t, ws, wg, wc, True, m_color=mc, split=split)
    ref, params = _oracle_point_grads(("tail", use_deform, M), use_deform, x, d, t, ws, wg, wc, mc)
    _check_point(r, params, loss, ref, pad, name=f"x3_tail_{int(use_deform)}_{M}" if split else None)


@pytest.mark.parametrize("use_deform", [True, False])
@pytest.mark.parametrize("tail", [64, 192])
def test_point_backward_tail_dense(use_deform, tail):
    """m_color = 256 < M = 256 + 64 / 256 + 192: the tail's launch arrangements of point_backward_chains (4 and 12 half-height
    deformation tiles; without a deformation network the tail's SDF tiles at the head of the colour launch), oracle on all rows."""
    _tail_dense(use_deform, tail)


def _sparse_rows(M, m_color, seed, main_every):
    """One row per 64-row tile at a random offset inside the tile (every ``main_every``-th tile of the coloured part, every tile of the
    tail) + the first and last row + both rows next to m_color."""
    rng = np.random.default_rng(seed)
    n_main = m_color if 0 < m_color < M else M
    K = {0, M - 1}
    for tile in range((M + 63) // 64):
        lo, hi = tile * 64, min(tile * 64 + 64, M)
        off = int(rng.integers(0, hi - lo))          # (drawn for every tile: the offsets do not depend on the thinning)
        if lo < n_main and tile % main_every:
            continue
        K.add(lo + off)
    if 0 < m_color < M:
        K |= {m_color - 1, m_color}
    return np.array(sorted(K))


SPARSE = {           # M, m_color, use_deform, every n-th tile of the coloured part
    "ragged_20031": (20031, 0, True, 1),
    "train_68608_deform": (65536 + 3072, 65536, True, 3),
    "train_68608_nodeform": (65536 + 3072, 65536, False, 3),
}


def _sparse_seeds(name, deterministic, split=False):
    M, m_color, use_deform, every = SPARSE[name]
    r = _renderer(use_deform)
    K = _sparse_rows(M, m_color, 7, every)
    x, d, t, ws, wg, wc = _inputs(M, 5000 + M, use_deform, screen=K)          # (rows without a seed add exact zeros whatever their masks)
    n_color = m_color if m_color else M
    stages = {int(k) % 64 // 16 for k in K}
    assert stages == {0, 1, 2, 3} and 250 <= len(K) <= 450, (stages, len(K))
    keep = torch.zeros(M, 1)
    keep[torch.from_numpy(K)] = 1.0
    ws, wg, wc = ws * keep, wg * keep, wc * keep          # exact zeros off K
    r.engine.deterministic = deterministic
    try:
        loss, pad = _hip_point_grads(r, x, d, t, ws, wg, wc, True, m_color=m_color, split=split)
    finally:
        r.engine.deterministic = False
    Kc = int((K < n_color).sum())          # K is sorted: its coloured rows come first
    Kt = torch.from_numpy(K)
    ref, params = _oracle_point_grads(("sparse", name), use_deform, x[Kt], d[Kt], t[Kt], ws[Kt], wg[Kt], wc[Kt], Kc)
    # gate: POINT_TOL unchanged -- rows with zero seeds add exact zeros to every fp32 sum, so the accumulation floor is that of |K| rows
    # (measured on MI355X, worst tensor / median: 8.3e-6 / 2.1e-6 at 20 031 rows, 5.6e-6 / 2.3e-6 at 68 608 rows with the deformation
    # network, 5.3e-6 / 2.3e-6 in deterministic mode, 2.4e-6 / 7.9e-7 without it; the dense M = 200 case measures up to 2.3e-5)
    _check_point(r, params, loss, ref, pad, name="x3_" * split + name + ("_det" if deterministic else ""))


@pytest.mark.parametrize("name,deterministic", [("ragged_20031", False), ("train_68608_deform", False), ("train_68608_nodeform", False),
                                                ("train_68608_deform", True)])
def test_point_backward_sparse_seeds(name, deterministic):
    """The parameter gradient is a sum over points of (adjoint seed x per-point term): with seeds that are exactly zero outside a row
    set K the full-size gradient equals the oracle's gradient on the |K| seeded points, while every tile, weight-gradient task and
    pad row of the big launch runs on real activations.  68 608 = the fused training launch of config 2 (bench.py's flagship)."""
    _sparse_seeds(name, deterministic)


# ------------------------------------------------------------------------------------------------------------------------------
# C. compositing away from S = 64
# ------------------------------------------------------------------------------------------------------------------------------
PROFILES = ("first_chunk", "last_chunk", "straddle", "nowhere", "immediately")
SAMPLE_DIST = 2.0 / 32


def _composite_case(N, S, seed, profile0=0):
    """Synthetic per-sample inputs (fp32-exact values in fp64 tensors).  Ray i has SDF profile (profile0 + i) % 5: the zero crossing --
    where the weights and the gradient mass sit -- in the first 64-lane chunk / in the last one / between s = 63 and 64 / nowhere
    (all-positive SDF) / before the first sample (alpha saturates at s = 0).  From N = 5 on: ray 2 has all z equal (near == far), ray 3
    two adjacent z swapped next to its crossing (negative section length: alpha ratio < 0, clipped, gradient exactly 0)."""
    rng = np.random.default_rng(seed)
    f32 = lambda a: torch.from_numpy(np.asarray(a, np.float32)).double()
    o = np.array([0.0, 0.0, -1.5]) + 0.05 * rng.normal(size=(N, 3))
    d = np.stack([0.25 * rng.normal(size=N), 0.25 * rng.normal(size=N), np.ones(N)], -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    rays = np.concatenate([o, d, np.zeros((N, 2)), rng.uniform(size=(N, 1))], -1)
    # depths 0.1 ... 3.0 along the axis: the section mid-points lie on both sides of the relax radius 1.2
    z = np.sort(rng.uniform(0.1, 3.0, size=(N, S)), axis=-1)
    last = (S - 1) // 64 * 64
    sdf = np.empty((N, S))
    cross = np.empty(N)
    for i in range(N):
        prof = PROFILES[(profile0 + i) % (3 if N >= 5 and i in (2, 3) else 5)]          # (rays 2 and 3 need a crossing)
        c = {"first_chunk": min(S, 64) * 0.4, "last_chunk": last + (S - last) * 0.3, "straddle": 63.5 if S > 64 else S * 0.5,
             "nowhere": -1.0, "immediately": -2.0}[prof]
        cross[i] = c
        if N >= 5 and i == 2:
            z[i] = z[i, S // 2]
        if prof == "nowhere":
            sdf[i] = 0.35 + 0.05 * rng.uniform(size=S)
        elif prof == "immediately":
            sdf[i] = -0.5 - 0.3 * (z[i] - z[i, 0])
        else:
            k = int(np.floor(c))
            zc = 0.5 * (z[i, k] + z[i, min(k + 1, S - 1)])
            sdf[i] = 0.3 * (zc - z[i]) + 0.01 * rng.normal(size=S)
            if N >= 5 and i == 2:
                sdf[i] = 0.05 * (c - np.arange(S))          # (all z equal: the profile runs over the sample index)
            if N >= 5 and i == 3:
                ks = min(k, S - 2)
                z[i, ks], z[i, ks + 1] = z[i, ks + 1], z[i, ks]
    # g_o: against the ray (true_cos near -1: the section's alpha is as large as it gets) with a random part, norms on both sides of 1
    g_o = -d[:, None, :] * rng.uniform(0.6, 1.4, size=(N, S, 1)) + 0.3 * rng.normal(size=(N, S, 3))
    flip = rng.uniform(size=(N, S)) < 0.1          # some samples face away (true_cos > 0: both relu branches of iter_cos)
    if N >= 5:
        flip[3] = False          # (the swapped pair of ray 3 must keep a negative true_cos: iter_cos = 0 would leave its ratio positive)
    g_o[flip] *= -1.0
    rgb = rng.uniform(size=(N, S, 3))
    return dict(rays=f32(rays), z=f32(z), sdf=f32(sdf).reshape(-1, 1), g_o=f32(g_o).reshape(-1, 3), rgb=f32(rgb).reshape(-1, 3), cross=cross)


def _alpha_ratio(c, var, ratio):
    """The un-clipped alpha ratio of the oracle's composite (endosurf_oracle.OracleRenderer.composite), for the input checks."""
    rays, z = c["rays"], c["z"]
    N, S = z.shape
    dists = torch.cat([z[:, 1:] - z[:, :-1], torch.full((N, 1), SAMPLE_DIST, dtype=z.dtype)], -1).reshape(-1, 1)
    tc = (rays[:, None, 3:6].expand(N, S, 3).reshape(-1, 3) * c["g_o"]).sum(-1, keepdim=True)
    ic = -(torch.relu(-tc * 0.5 + 0.5) * (1.0 - ratio) + torch.relu(-tc) * ratio)
    inv_s = float(np.exp(var * 10.0))
    pc, nc = torch.sigmoid((c["sdf"] - ic * dists * 0.5) * inv_s), torch.sigmoid((c["sdf"] + ic * dists * 0.5) * inv_s)
    mid = z + dists.reshape(N, S) * 0.5
    radius = (rays[:, None, :3] + O.d_over_z(rays[:, 3:6])[:, None] * mid[:, :, None]).norm(dim=-1)
    return ((pc - nc + 1e-6) / (pc + 1e-6)).reshape(N, S), radius


def _run_composite(eng, c, var_value, ratio, seed, n_aux=0, with_aux_grads=False):
    dt = torch.float64
    rays, z = c["rays"], c["z"]
    N, S = z.shape
    sdf, rgb, g_o = (c[k].clone().requires_grad_(True) for k in ("sdf", "rgb", "g_o"))
    var = torch.tensor(np.float32(var_value), dtype=dt, requires_grad=True)
    inv_s = torch.exp(var * 10.0).clamp(1e-6, 1e6)
    R = O.OracleRenderer(None, RENDER_CFG)
    ref = R.composite(rays[:, :3], rays[:, 3:6], z, SAMPLE_DIST, ratio, sdf, rgb, g_o, inv_s)
    f32 = lambda t: t.detach().to(torch.float32).cuda().contiguous()
    a = eng.composite_args(f32(rays), f32(z), f32(sdf).reshape(-1), f32(g_o), f32(rgb), f32(var).reshape(1), SAMPLE_DIST, ratio)
    out = eng.composite_forward(a)
    torch.cuda.synchronize()
    mx = lambda k, r_: float(np.max(np.abs(out[k].cpu().numpy().astype(np.float64) - r_.detach().numpy())))
    wmax_ref, idx_ref = ref["weights"].detach().max(-1, keepdim=True)
    # the tolerances of test_composite_forward_backward
    assert mx("color", ref["color_map"]) < 3e-6
    # depth: 5e-6 at the golden cases' depths (~1.3); these rays reach z = 3 over up to 256 terms, so the bound scales with the depth
    # (measured at S = 256: 5.1 / 5.9 / 6.0e-6 at depths up to 2.5; the oracle's own fp32 run is off its fp64 run by 5.1 / 5.9 / 6.0e-6 there)
    assert mx("depth", ref["depth_map"]) < 5e-6 * max(1.0, float(ref["depth_map"].detach().abs().max()))
    assert mx("weights", ref["weights"]) < 3e-6
    assert mx("cdf", ref["cdf"]) < 3e-6
    assert mx("weight_max", wmax_ref) < 3e-6
    eik = (out["eik_acc"][0] / (out["eik_acc"][1] + 1e-6)).item()
    assert abs(eik - float(ref["gradient_o_error"])) < 1e-5 * max(1.0, float(ref["gradient_o_error"]))
    # arg-max: the first index of the maximum of the kernel's own weights (torch.max's rule), and the oracle's index wherever the
    # oracle's maximum is not a near-tie (a runner-up within the forward tolerance may legitimately win in fp32)
    w_hip = out["weights"].cpu()
    assert torch.equal(out["wmax_idx"].cpu().long(), w_hip.max(-1)[1])
    second = ref["weights"].detach().scatter(1, idx_ref, -1.0).max(-1, keepdim=True)[0] if S > 1 else wmax_ref - 1.0
    clear = ((wmax_ref - second) > 1e-5).reshape(-1)
    assert torch.equal(out["wmax_idx"].cpu().long()[clear], idx_ref.reshape(-1)[clear])
    assert float(clear.double().mean()) >= 0.6, "too many near-ties of the two largest weights"

    rng = np.random.default_rng(seed)
    g = {k: torch.tensor(rng.normal(size=tuple(ref[k].shape)), dtype=dt) for k in ("color_map", "depth_map", "weights", "cdf", "gradients_o")}
    g_eik = torch.tensor(0.7, dtype=dt)
    g_wmax = torch.tensor(rng.normal(size=(N, 1)), dtype=dt) * clear.reshape(N, 1).to(dt)          # (near-tie: which sample gets it is ill-posed)
    scal = sum((ref[k] * g[k]).sum() for k in g) + ref["gradient_o_error"] * g_eik + (ref["weights"].max(-1, keepdim=True)[0] * g_wmax).sum()
    scal.backward()
    eik_den = (out["eik_acc"][1] + 1e-6).reshape(1).contiguous()
    aux = {}
    if n_aux and with_aux_grads:
        aux = dict(g_aux_sdf=f32(torch.tensor(rng.normal(size=n_aux))), g_aux_go=f32(torch.tensor(rng.normal(size=(n_aux, 3)))))
    bw = eng.composite_backward(a, f32(g["color_map"]), f32(g["depth_map"]).reshape(-1), f32(g_eik).reshape(1), eik_den,
                                g_weights=f32(g["weights"]), g_cdf=f32(g["cdf"]), g_wmax=f32(g_wmax).reshape(-1),
                                g_gradients_o=f32(g["gradients_o"]), n_aux=n_aux, **aux)
    torch.cuda.synchronize()
    P = N * S
    if n_aux:          # the auxiliary points' adjoint rows behind the N * S sample rows: the given rows, or zeros
        assert bw["d_sdf"].shape[0] == P + n_aux and bw["d_go"].shape[0] == P + n_aux
        assert torch.equal(bw["d_sdf"][P:], aux["g_aux_sdf"] if aux else torch.zeros(n_aux, device="cuda"))
        assert torch.equal(bw["d_go"][P:], aux["g_aux_go"] if aux else torch.zeros(n_aux, 3, device="cuda"))

    def rel(a_, b_):
        b_ = b_.detach().numpy().reshape(-1)
        return float(np.max(np.abs(a_.cpu().numpy().astype(np.float64).reshape(-1) - b_)) / (np.max(np.abs(b_)) + 1e-12))
    errs = dict(d_sdf=rel(bw["d_sdf"][:P], sdf.grad), d_go=rel(bw["d_go"][:P], g_o.grad), d_rgb=rel(bw["d_rgb"], rgb.grad))
    assert errs["d_sdf"] < 2e-4 and errs["d_go"] < 2e-4 and errs["d_rgb"] < 1e-5, errs
    dvar = bw["d_invs_acc"].item() * 10.0 * float(inv_s)
    assert abs(dvar - float(var.grad)) < 2e-4 * abs(float(var.grad)) + 1e-6, (dvar, float(var.grad))
    # per ray as well: a ray whose gradient is small next to the batch maximum must not hide behind it
    ds_hip, ds_ref = bw["d_sdf"][:P].cpu().double().reshape(N, S), sdf.grad.reshape(N, S)
    ray_err = (ds_hip - ds_ref).abs().max(-1)[0] / torch.clamp(ds_ref.abs().max(-1)[0], min=1e-2 * float(ds_ref.abs().max()))
    assert float(ray_err.max()) < 2e-3, (int(ray_err.argmax()), float(ray_err.max()))
    return ref, out, bw, sdf.grad.reshape(N, S)


VAR, RATIO = 0.36, 0.3          # inv_s = 36.6 (the "trained" weights' value); cos-anneal ratio strictly inside (0, 1): both branches of iter_cos


@pytest.mark.parametrize("N", [1, 5, 257])
@pytest.mark.parametrize("S", [32, 48, 64, 65, 96, 128, 192, 256])
def test_composite_sample_counts(S, N):
    """One to four 64-lane chunks per ray (the transmittance carry of the forward, the suffix sum of the backward and the arg-max run
    across them), half-filled and ragged last chunks, a partial last block of 4 rays."""
    from endosurf_amd.engine import Engine
    eng = Engine("cuda")
    # (a single ray: the crossing between s = 63 and 64 / at S / 2, before the first sample at S = 64, in the last chunk from S = 96 on)
    c = _composite_case(N, S, 100 * S + N, profile0=S // 16 if N > 1 else (4 if S == 64 else (2 if S <= 65 else 1)))
    ratio, radius = _alpha_ratio(c, VAR, RATIO)
    assert bool((radius < 1.2).any()) and bool((radius > 1.2).any()), "samples on both sides of the relax radius"
    if N >= 5:
        assert bool((ratio < 0).any()), "a negative section length must put some alpha ratios below 0"
        assert bool((c["z"][2] == c["z"][2, 0]).all())
    ref, out, bw, dsdf_ref = _run_composite(eng, c, VAR, RATIO, S + N)
    if N >= 5:
        # the clip passes no gradient: exactly 0 where the ratio is clearly outside [0, 1] (g_cdf still reaches prev_cdf there, through
        # d_sdf only: compare d_go's ray-direction part with the oracle's, which is 0 there up to the eikonal / g_gradients_o terms)
        outside = (ratio < -1e-3).reshape(-1)
        w = ref["weights"].detach().reshape(-1)
        assert bool((w[outside] == 0).all()) and bool((out["weights"].cpu().reshape(-1)[outside] == 0).all())
        # the mass of each profile really sits where the case says (else the chunk-crossing claims above are empty)
        wsum = ref["weights"].detach()
        for i in range(N):
            if i in (2, 3):
                continue
            prof = PROFILES[(S // 16 + i) % 5]
            if prof == "last_chunk" and S > 64 and S - (S - 1) // 64 * 64 >= 32:
                assert float(wsum[i, (S - 1) // 64 * 64:].sum()) > 0.3, (i, prof)
            if prof == "nowhere":
                assert float(wsum[i].sum()) < 0.25, (i, prof)
            if prof == "immediately":
                assert float(wsum[i, 0]) > 0.5, (i, prof)


@pytest.mark.parametrize("S", [32, 128])
def test_composite_deterministic_mode(S):
    """engine.deterministic: the eikonal sums and the inv_s adjoint go through per-ray partials and a fixed-order reduction."""
    from endosurf_amd.engine import Engine
    eng = Engine("cuda")
    eng.deterministic = True
    _run_composite(eng, _composite_case(37, S, 900 + S), VAR, RATIO, 5)


@pytest.mark.parametrize("with_aux_grads", [False, True])
def test_composite_aux_rows(with_aux_grads):
    from endosurf_amd.engine import Engine
    _run_composite(Engine("cuda"), _composite_case(6, 96, 77), VAR, RATIO, 6, n_aux=13, with_aux_grads=with_aux_grads)


@pytest.mark.parametrize("S", [65, 128, 256])
def test_composite_weight_max_across_chunks(S):
    """The weight maximum in a later chunk than a strong runner-up (and the other way round): value, index and the route of g_wmax.
    Exactly equal positive weights at two samples cannot be built (the later one carries the earlier one's 1 - alpha in its
    transmittance); exact ties are pinned on rows whose weights are ALL exactly 0 -- z running backwards with a negative sample_dist
    clips every alpha -- where the index must be the first of the row, as torch.max's."""
    from endosurf_amd.engine import Engine
    eng = Engine("cuda")
    N = 8
    rng = np.random.default_rng(S)
    f32 = lambda a: torch.from_numpy(np.asarray(a, np.float32)).double()
    c = _composite_case(N, S, 40 + S, profile0=3)          # ray geometry and rgb; SDF / g_o are replaced below
    z = np.linspace(0.6, 2.4, S)[None, :] + rng.uniform(-0.2, 0.2, size=(N, S)) * (1.8 / (S - 1))
    sdf = np.full((N, S), 0.3)
    d = c["rays"][:, 3:6].numpy()
    g_o = np.repeat(-d[:, None, :], S, axis=1)
    for i in range(N):
        # two dips of the SDF towards 0 (two weight peaks), one per chunk; the deeper dip alternates between the earlier and the later
        a_, b_ = int(rng.integers(4, 60)), (int(rng.integers(64, S - 1)) if S > 66 else 64)          # (not the last sample: its length is sample_dist)
        deep, shallow = (a_, b_) if i % 2 == 0 else (b_, a_)
        sdf[i, deep], sdf[i, shallow] = 0.0, 0.035
    c.update(z=f32(z), sdf=f32(sdf).reshape(-1, 1), g_o=f32(g_o).reshape(-1, 3))
    ref, out, bw, _ = _run_composite(eng, c, VAR, RATIO, 3)
    idx = ref["weights"].detach().max(-1)[1]
    assert bool((idx[0::2] < 64).all()) and bool((idx[1::2] >= 64).all()), idx          # the maximum really alternates between the chunks
    w = ref["weights"].detach()
    lo, hi = torch.minimum(w[:, :64].max(-1)[0], w[:, 64:].max(-1)[0]), w.max(-1)[0]
    assert bool((lo > 0.15 * hi).all()), (lo, hi)          # ... with a runner-up of comparable size in the other chunk
    # exact ties: every weight of every ray exactly 0
    zr = torch.flip(c["z"], dims=[1]).contiguous()
    dev = lambda t: t.to(torch.float32).cuda().contiguous()
    var = torch.tensor([VAR], device="cuda")
    sdf0 = torch.zeros_like(c["sdf"])          # on the level set: every section's cdf difference is far from the 1e-6 of the ratio
    a = eng.composite_args(dev(c["rays"]), dev(zr), dev(sdf0).reshape(-1), dev(c["g_o"]), dev(c["rgb"]), var, -SAMPLE_DIST, RATIO)
    out0 = eng.composite_forward(a)
    torch.cuda.synchronize()
    R = O.OracleRenderer(None, RENDER_CFG)
    ref0 = R.composite(c["rays"][:, :3], c["rays"][:, 3:6], zr, -SAMPLE_DIST, RATIO, sdf0, c["rgb"], c["g_o"], float(np.exp(np.float32(VAR) * 10.0)))
    assert float(ref0["weights"].abs().max()) == 0.0 and int(ref0["weights"].max(-1)[1].abs().max()) == 0
    assert float(out0["weights"].abs().max()) == 0.0 and float(out0["weight_max"].abs().max()) == 0.0
    assert int(out0["wmax_idx"].abs().max()) == 0


# ------------------------------------------------------------------------------------------------------------------------------
# D. render-level parameter gradients at the non-golden sample counts
# ------------------------------------------------------------------------------------------------------------------------------
def _scalar(ret, w, dt, dev):
    """The combination of test_gpu_backward._render_scalar with this module's fixed random weights."""
    cw, dw, gw, ww = (w[k].to(dtype=dt, device=dev) for k in ("cw", "dw", "gw", "ww"))
    return ((ret["color_map"] * cw).sum() + (ret["depth_map"] * dw).sum() + (ret["gradients_o"] * gw).sum()
            + (ret["weights"] * ww).sum() + 0.5 * ret["gradient_o_error"] + (ret["cdf"] * ww).sum() * 0.1
            + ret["s_val"].sum() * 0.01)


def _oracle_render_grads(use_deform, cfg, rays, z, it, w, dtype):
    net, params = _oracle_params(use_deform, dtype)
    R = O.OracleRenderer(net, cfg)
    ry, zz = rays.to(dtype), z.to(dtype)
    ret = R.render_core(ry[:, :3], ry[:, 3:6], ry[:, 8], zz, 2.0 / cfg["n_samples"], R.cos_anneal_ratio(it))
    ret["s_val"] = ret["s_val"].reshape(1, 1).expand(zz.shape[0], zz.shape[1]).mean(-1, keepdim=True)          # as render_rays returns it
    scal = _scalar(ret, w, dtype, "cpu")
    scal.backward()
    return float(scal), params


@pytest.mark.parametrize("name", ["config3_64+64", "coarse_32"])
def test_render_param_grads_sample_counts(name):
    """z is fixed (sampled once by the kernels, handed to both sides as z_vals): the budget is not set by inverse-CDF amplification.
    config3_64+64: 24 rays x 128 samples (two chunks per ray in compositing, S of BASELINE config 3).  coarse_32: 7 rays x 32 samples
    = 224 points (not a tile multiple), no deformation network, before important_begin_iter, cos-anneal ratio 1."""
    if name == "config3_64+64":
        use_deform, n_rays, it = True, 24, 1000
        cfg = dict(RENDER_CFG, n_samples=64, n_importance=64)
    else:
        use_deform, n_rays, it = False, 7, 1
        cfg = dict(RENDER_CFG, n_samples=32, n_importance=32, important_begin_iter=1000, anneal_end=0)
    r = renderer_for(SEED, "trained", use_deform, render_cfg=cfg)
    rays = torch.from_numpy(weightgen.make_rays(SEED + 1, n_rays))
    with torch.no_grad():
        z = r.sample_z(rays.cuda(), iter_step=it, perturb_overwrite=False)
    S = z.shape[1]
    assert S == (128 if use_deform else 32)
    rng = np.random.default_rng(11)
    w = {k: torch.from_numpy(rng.normal(size=s)) for k, s in (("cw", (n_rays, 3)), ("dw", (n_rays, 1)), ("gw", (n_rays, S, 3)), ("ww", (n_rays, S)))}
    ret = r.render_rays(rays.cuda(), iter_step=it, z_vals=z)
    scal = _scalar(ret, w, torch.float32, "cuda")
    scal.backward()
    torch.cuda.synchronize()
    v64, p64 = _oracle_render_grads(use_deform, cfg, rays, z.cpu(), it, w, torch.float64)
    v32, p32 = _oracle_render_grads(use_deform, cfg, rays, z.cpu(), it, w, torch.float32)
    assert abs(float(scal.detach()) - v64) < 3 * abs(v32 - v64) + 1e-4 * max(1.0, abs(v64)), (float(scal.detach()), v64, v32)
    rows = _grad_table(r, p64)
    bad = {}
    for k, (rel, nref, ngot) in rows.items():
        if nref < 1e-9:
            continue
        g64, g32 = p64[k].grad.reshape(-1), p32[k].grad.double().reshape(-1)
        ref_rel = float((g32 - g64).norm() / (g64.norm() + 1e-30))          # the oracle's own fp32-vs-fp64 error on this tensor
        budget = max(3 * ref_rel, FLOOR)
        if rel > budget:
            bad[k] = (rel, budget, ref_rel)
    assert not bad, bad
    assert sum(v[1] >= 1e-9 for v in rows.values()) >= 40


# ------------------------------------------------------------------------------------------------------------------------------
# E. up-sampling on tied and flat inputs
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_imp", [8, 16, 64])
@pytest.mark.parametrize("n", [32, 64, 80, 112])
def test_upsample_ties_and_flat_profiles(n, n_imp):
    """Row 0: all z equal (near == far: every new sample ties with every old one).  Row 1: constant SDF (flat weights).  Row 2: a
    zero-length section (two equal z) that takes nearly all the weight, so most new samples land exactly on an old pair.  Row 3: a
    plain crossing (control).  New depths against the oracle in fp64 at the budget of test_sampling_trace; the kernel's merge against
    the stable sort of (old, new) -- old sample first on ties."""
    from endosurf_amd import _lib
    r = _renderer(False)
    eng = r.engine
    rng = np.random.default_rng(n * 100 + n_imp)
    N, inv_s = 4, 64.0
    rays = weightgen.make_rays(SEED + 5, N, jitter=0.0)
    z = np.sort(rng.uniform(0.6, 2.4, size=(N, n)), axis=-1).astype(np.float32)
    sdf = (0.6 * (z[:, n // 2:n // 2 + 1] - z) + 0.01 * rng.normal(size=(N, n))).astype(np.float32)
    z[0] = z[0, n // 3]
    sdf[1] = 0.5
    k = 0          # (deep inside the surface every section's alpha is ~1: the FIRST section takes the weight, so that is the one of length 0)
    z[2, k + 1] = z[2, k]
    sdf[2] = -0.5
    o, d = torch.from_numpy(rays[:, :3]), torch.from_numpy(rays[:, 3:6])
    zt, st = torch.from_numpy(z), torch.from_numpy(sdf)
    R = O.OracleRenderer(None, RENDER_CFG)
    ref64 = R.up_sample(o.double(), d.double(), zt.double(), st.double(), n_imp, inv_s).numpy()
    ref32 = R.up_sample(o, d, zt, st, n_imp, inv_s).numpy().astype(np.float64)
    z_new = r.up_sample(o.cuda(), d.cuda(), zt.cuda(), st.cuda(), n_imp, inv_s)
    got = z_new.cpu().numpy().astype(np.float64)
    assert got.shape == ref64.shape
    qd = lambda a, b, q: float(np.quantile(np.abs(a - b), q))
    assert qd(got, ref64, 0.99) < 3 * qd(ref32, ref64, 0.99) + 2e-6, (qd(got, ref64, 0.99), qd(ref32, ref64, 0.99))
    assert np.max(np.abs(got - ref64)) < 3 * np.max(np.abs(ref32 - ref64)) + 1e-4
    assert np.all(got[0] == z[0, 0]), "all z equal: every new depth is that value"
    assert np.mean(got[2] == z[2, k]) > 0.5, "the zero-length section must receive most of the new samples"

    # merged depths: the renderer's cat_z_vals (last=True: no network query) against the oracle's on the same new depths -- exact
    zc, _ = r.cat_z_vals(o.cuda(), d.cuda(), None, zt.cuda(), z_new, st.cuda(), last=True)
    zc_ref, _ = R.cat_z_vals(o.double(), d.double(), None, zt.double(), z_new.cpu().double(), st.double(), last=True)
    assert torch.equal(zc.cpu().double(), zc_ref)
    # the kernel's own merge (es_upsample_step's z_out / src_idx, what the sampling chain consumes): sorted, and the STABLE order
    S = n + n_imp
    ry = torch.from_numpy(rays).cuda().contiguous()
    zn2, z_out, src = eng.empty(N, n_imp), eng.empty(N, S), eng.empty(N, S, dtype=torch.int32)
    zd, sd = zt.cuda().contiguous(), st.cuda().contiguous()
    _lib.check(eng.lib.es_upsample_step(_lib.ptr(ry), _lib.ptr(zd), n, _lib.ptr(sd), n, N, n, n_imp, float(inv_s), _lib.ptr(zn2), _lib.ptr(z_out),
                                        S, _lib.ptr(src), eng.st()), "es_upsample_step")
    torch.cuda.synchronize()
    assert torch.equal(zn2, z_new)
    cat = torch.cat([zt, zn2.cpu()], -1)
    z_sorted, order = torch.sort(cat, dim=-1, stable=True)          # stable: an old sample (lower index) stays ahead of an equal new one
    assert torch.equal(z_out.cpu(), z_sorted)
    assert bool((z_out[:, 1:] >= z_out[:, :-1]).all())
    assert torch.equal(src.cpu().long(), order)
    assert int((z_sorted[:, 1:] == z_sorted[:, :-1]).sum()) >= n, "the case must contain ties between old and new samples"
