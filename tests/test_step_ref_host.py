"""The fp64 references of tests/step_ref.py pinned WITHOUT a GPU:
  - train_loss / eod_loss / sn_loss / aux_points against the oracle's own code (O.train_loss, OracleRenderer.errorondepth and
    surface_neighbour_error run unbound on a stub renderer whose render, point evaluation and ray marching return prescribed tensors);
  - schedule against O.lr_factor, trainer.lr_factor, the renderer's get_cos_anneal_ratio and FlatAdam's bias corrections;
  - adam against torch.optim.Adam in fp64, where the distance between the kernel's Adam (beta2 = fl32(0.999)) and double-beta Adam is
    measured and bounded;
  - the numpy fp32 twins of the kernels (tests/step_twin.py, plain and with fused multiply-adds) below HALF of every gate of
    tests/step_cases.py on every input set of tests/test_gpu_step_kernels.py: the gates are satisfiable by the kernels' own arithmetic."""
import math
import types

import numpy as np
import pytest
import torch

import step_cases as C
import step_ref as R
import step_twin as T
from oracle import endosurf_oracle as O

D = torch.float64
W = C.LOSS_W


def _rel(a, b, tol=1e-12):
    a, b = torch.as_tensor(a, dtype=D), torch.as_tensor(b, dtype=D)
    assert a.shape == b.shape, (a.shape, b.shape)
    if a.numel():
        assert bool(((a - b).abs() <= tol * torch.maximum(b.abs(), torch.ones_like(b))).all()), float((a - b).abs().max())


# ---- the oracle's own loss code on a stub renderer ---------------------------------------------------------------------------------------
class _StubNet:
    def __init__(self, outs):
        self.outs, self.seen = list(outs), []

    def point_eval(self, pts, d, t, with_color=True):
        self.seen.append((pts.detach().clone(), t.detach().clone()))
        return self.outs.pop(0)


class _Stub:
    """What O.train_loss and the two OracleRenderer methods touch: render_rays, net.point_eval, ray_marching."""
    errorondepth = O.OracleRenderer.errorondepth
    surface_neighbour_error = O.OracleRenderer.surface_neighbour_error

    def __init__(self, ret, d_i, outs):
        self.ret, self.d_i, self.net = ret, d_i, _StubNet(outs)

    def render_rays(self, rays, iter_step=0, u_perturb=None):
        return self.ret

    def ray_marching(self, rays):
        return self.d_i


def _stub_case(N, seed=0):
    p = C.points_inputs(N, seed)
    rng = np.random.default_rng(77 + N)
    leaf = lambda *s: torch.from_numpy(rng.standard_normal(s)).requires_grad_(True)
    lv = dict(color_map=leaf(N, 3), depth_map=leaf(N, 1), eik=leaf(), sdf=leaf(N, 1), go=leaf(N, 3), g_s=leaf(N, 3), g_n=leaf(N, 3))
    batch = dict(rays=R.d64(p["rays"]), color=torch.from_numpy(rng.uniform(size=(N, 3))), depth=R.d64(p["depth_gt"]).reshape(N, 1),
                 mask=R.d64(p["mask"]).reshape(N, 1), color_mask=torch.from_numpy((rng.uniform(size=(N, 1)) < 0.6).astype(np.float64)))
    x, t, valid, inside = R.aux_points(p["rays"], p["depth_gt"], p["mask"], p["d_i"], p["u"], p["rad"])
    return p, lv, batch, x, t, valid, inside


@pytest.mark.parametrize("N", [1, 37, 300])
def test_train_loss_reference_is_the_oracles(N):
    p, lv, batch, x, t, valid, inside = _stub_case(N)
    outs = [dict(sdf=lv["sdf"], g_o=lv["go"]), dict(g_o=torch.cat([lv["g_s"][valid], lv["g_n"][valid]], 0))]
    stub = _Stub(dict(color_map=lv["color_map"], depth_map=lv["depth_map"], gradient_o_error=lv["eik"]), R.d64(p["d_i"]).reshape(N, 1), outs)
    w64 = {k: R.fl32(v) for k, v in W.items()}          # (the reference rounds the weights to fp32 like the C struct does)
    total, terms, _ = O.train_loss(stub, batch, 3, None, R.d64(p["u"]), weights=w64, surf_neig_rad=R.fl32(p["rad"]))
    total.backward()
    # the points the oracle evaluated are the reference's rows (and its validity mask the reference's)
    _rel(stub.net.seen[0][0], x[:N])
    _rel(stub.net.seen[0][1][:, 0], t[:N])
    if bool(valid.any()):
        _rel(stub.net.seen[1][0], torch.cat([x[N:2 * N][valid], x[2 * N:][valid]], 0))
    a_sdf = torch.cat([lv["sdf"].detach(), torch.zeros(2 * N, 1, dtype=D)], 0)
    a_go = torch.cat([lv["go"], lv["g_s"], lv["g_n"]], 0).detach()
    ref = R.train_loss(lv["color_map"], lv["depth_map"], lv["eik"], a_sdf, a_go, batch["rays"], x[:N], batch["color"], batch["depth"], batch["mask"],
                       batch["color_mask"], valid, W)
    _rel(total.detach(), ref["total"])
    for k in R.LOSS_KEYS:
        _rel(terms[k].detach(), ref["terms"][k])
    assert ref["n_valid"] == float(valid.sum())
    z = lambda v: torch.zeros_like(v) if v.grad is None else v.grad
    _rel(z(lv["color_map"]), ref["g_color"])
    _rel(z(lv["depth_map"]), ref["g_depth"])
    _rel(z(lv["eik"]), ref["g_eik"])
    _rel(z(lv["sdf"]), ref["g_aux_sdf"][:N])
    assert float(ref["g_aux_sdf"][N:].abs().max()) == 0.0
    _rel(torch.cat([z(lv["go"]), z(lv["g_s"]), z(lv["g_n"])], 0), ref["g_aux_go"])
    # the local normalisers the exact mode all-reduces
    m = batch["mask"]
    ins = inside[:, None]
    assert ref["den"] == [float(batch["color_mask"].sum()), float(ins.sum()), float((ins * m).sum()), float(valid.sum())]


@pytest.mark.parametrize("N", [1, 37, 300])
def test_eod_and_sn_references_are_the_oracles(N):
    p, lv, batch, x, t, valid, inside = _stub_case(N, seed=1)
    stub = _Stub(None, R.d64(p["d_i"]).reshape(N, 1), [dict(sdf=lv["sdf"], g_o=lv["go"]), dict(g_o=torch.cat([lv["g_s"][valid], lv["g_n"][valid]], 0))])
    a, b, ins = O.OracleRenderer.errorondepth(stub, batch["rays"], batch["depth"], batch["mask"])
    (0.7 * a - 1.3 * b).backward()
    ref = R.eod_loss(batch["rays"], x[:N], batch["mask"], lv["sdf"], lv["go"], 0.7, -1.3)
    _rel(a.detach(), ref["sdf_err"]); _rel(b.detach(), ref["ang_err"]); _rel(ins[:, 0], ref["inside"]); _rel(ins[:, 0], inside)
    _rel(lv["sdf"].grad[:, 0], ref["d_sdf"]); _rel(lv["go"].grad, ref["d_go"])
    sn, d_i, v = O.OracleRenderer.surface_neighbour_error(stub, batch["rays"], batch["mask"], R.fl32(p["rad"]), R.d64(p["u"]))
    assert torch.equal(v, valid)
    rs = R.sn_loss(torch.cat([lv["g_s"], lv["g_n"]], 0), valid, 1.9)
    _rel(sn.detach(), rs["loss"])
    if bool(valid.any()):
        (1.9 * sn).backward()
        _rel(torch.cat([lv["g_s"].grad, lv["g_n"].grad], 0), rs["d_g"])
    else:
        assert float(rs["d_g"].abs().max()) == 0.0 and float(rs["den"]) == 1.0


def test_exact_mode_reference_is_the_mean_over_parts():
    """den_global + world: the mean over two unequal parts of (terms, adjoints / world) is the loss of the concatenated batch."""
    a, b = C.loss_inputs(37, "mixed", seed=3), C.loss_inputs(100, "mixed", seed=4)
    ra, rb = C.loss_ref(a), C.loss_ref(b)
    den = [x + y for x, y in zip(ra["den"], rb["den"])]
    pa, pb = C.loss_ref(a, den_global=den, world=2.0), C.loss_ref(b, den_global=den, world=2.0)
    cat = C.concat_parts(a, b)
    rc = C.loss_ref(cat)
    assert rc["den"] == den
    for k in R.LOSS_KEYS:
        _rel((pa["terms"][k] + pb["terms"][k]) / 2, rc["terms"][k])
    for k in ("g_color", "g_depth"):
        _rel(torch.cat([pa[k], pb[k]], 0) / 2, rc[k])
    _rel(C.cat3(pa["g_aux_go"], pb["g_aux_go"]) / 2, rc["g_aux_go"])
    _rel(C.cat3(pa["g_aux_sdf"], pb["g_aux_sdf"]) / 2, rc["g_aux_sdf"])


# ---- schedule -------------------------------------------------------------------------------------------------------------------------------
def test_schedule_reference():
    from endosurf_amd.renderer import EndoSurfRenderer
    from endosurf_amd.trainer import FlatAdam, lr_factor
    b1, b2 = 0.9, 0.999
    for name, (s0, t0), steps, kw in C.schedule_cases():
        rec = []
        eng = types.SimpleNamespace(adam_step=lambda *a: rec.append(a))
        opt = types.SimpleNamespace(param_groups=[dict(lr=0.0, betas=(b1, b2), eps=1e-8)], step_count=int(t0), scalars_dev=None, eng=eng, _all=[],
                                    _var=types.SimpleNamespace(grad=None), _var_off=0, flat=torch.zeros(2), exp_avg=None, exp_avg_sq=None,
                                    model=types.SimpleNamespace(_epoch=0))
        for k in range(1, steps + 1):
            step, t = int(s0) + k, int(t0) + k
            s = R.schedule(float(step), float(t), kw["lr_init"], kw["n_iter"], kw["warm_up_end"], kw["lr_alpha"], b1, b2, 0.5, kw["anneal_end"])
            for f in (O.lr_factor, lr_factor):
                lr = kw["lr_init"] * f(step, kw["n_iter"], kw["warm_up_end"], kw["lr_alpha"])
                assert s[0] == pytest.approx(lr / (1.0 - b1 ** t), rel=4e-15, abs=0.0), (name, step)
            assert s[1] == math.sqrt(1.0 - b2 ** t) and s[2] == 0.5
            stub = types.SimpleNamespace(anneal_end=float(kw["anneal_end"]))
            assert s[3] == EndoSurfRenderer.get_cos_anneal_ratio(stub, step) == O.OracleRenderer.cos_anneal_ratio(stub, step)
            # FlatAdam's own expressions: what it hands to es_adam_step at this step count with this learning rate
            opt.param_groups[0]["lr"] = kw["lr_init"] * lr_factor(step, kw["n_iter"], kw["warm_up_end"], kw["lr_alpha"])
            FlatAdam.step(opt, grad=torch.zeros(2), variance_in_grad=True)
            assert opt.step_count == t and rec[-1][8] == pytest.approx(s[0], rel=4e-15, abs=0.0) and rec[-1][9] == s[1], (name, step)
    # the branches: warm-up strictly below warm_up_end, the cosine from the step equal to it
    assert R.schedule(3.0, 3.0, 1.0, 40, 4, 0.05, 0.0, 0.0, 1.0, 0)[0] == 0.75
    assert R.schedule(4.0, 4.0, 1.0, 40, 4, 0.05, 0.0, 0.0, 1.0, 0)[0] == 1.0
    assert R.schedule(40.0, 40.0, 1.0, 40, 4, 0.05, 0.0, 0.0, 1.0, 6)[0] == pytest.approx(0.05, rel=1e-15) and \
        R.schedule(3.0, 3.0, 1.0, 40, 4, 0.05, 0.0, 0.0, 1.0, 6)[3] == 0.5


# ---- Adam -----------------------------------------------------------------------------------------------------------------------------------
def _run_adam(n, betas_exact):
    """Seven steps on the inputs of the GPU test: step_ref.adam (fl32 betas) or torch.optim.Adam in fp64 with ``betas_exact`` doubles."""
    inp, hp = C.adam_inputs(n), C.ADAM_HP
    p0 = R.d64(inp["p"])
    ref = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=hp["lr"], betas=betas_exact, eps=R.fl32(hp["eps"]))
    p, m, v = p0.clone(), torch.zeros(n, dtype=D), torch.zeros(n, dtype=D)
    ups_t, ups_r = [], []
    for t in range(1, 8):
        g, ex, gs = inp["grads"][t - 1], inp["extras"][t - 1], inp["grad_scale"][t - 1]
        full = R.d64(g).clone()
        full[n // 2] += float(ex[0])
        before = ref.detach().clone()
        ref.grad = full * gs
        opt.step()
        ups_t.append(before - ref.detach())
        ss, bc = C.adam_scalars(t, dict(hp, beta1=betas_exact[0], beta2=betas_exact[1]))       # torch's bias corrections use ITS betas
        p, m, v, upd = R.adam(p, g, m, v, betas_exact[0], betas_exact[1], hp["eps"], ss, bc, gs, ex, n // 2)
        ups_r.append(upd)
    return ups_t, ups_r, (p, m, v), (ref.detach(), opt.state[ref]["exp_avg"], opt.state[ref]["exp_avg_sq"])


def test_adam_reference_and_beta_rounding(monkeypatch):
    """step_ref.adam is torch.optim.Adam when both are given the same betas, and the Adam the kernel implements (beta = fl32(beta),
    1 - beta from the rounded value) stays within |fl32(b2) - b2| / (1 - b2) = 1.287e-5 of double-beta Adam's update, relative to the
    update.  v is proportional to 1 - b2 and the update to v^-1/2, so half of that is the expectation.

    Measured here (n = 100003, seven steps, the GPU test's gradients): the median |d update| / |update| over the elements whose first
    moment does not cancel is 0.52 of the bound at every step (6.7e-6 of the update).  beta1's rounding (|fl32(0.9) - 0.9| = 2.4e-8)
    enters the first moment as E_t = b1 E_(t-1) + |d b1| (|m_(t-1)| + |g_t|), which is NOT relative to the update where m cancels; with
    that term added, step_size E_t / denom, the worst element sits at 0.51 of its allowance.  (Relative to the update alone the
    worst such element is 43 bounds away: a bound purely relative to the update holds for beta2's rounding only.)"""
    monkeypatch.setattr(R, "fl32", lambda x: float(x))          # same numbers on both sides: step_size / bc2_sqrt / betas unrounded
    n = 1000
    b1, b2 = R.fl32(0.9), R.fl32(0.999)
    ups_t, ups_r, (p, m, v), (pt, mt, vt) = _run_adam(n, (float(np.float32(0.9)), float(np.float32(0.999))))
    _rel(p, pt, 1e-13); _rel(m, mt, 1e-13); _rel(v, vt, 1e-13)
    monkeypatch.undo()
    b2r = float(np.float32(0.999))
    bound = abs(b2r - 0.999) / (1.0 - 0.999)
    assert 1.2e-5 < bound < 1.4e-5
    n = 100003
    ups_t, _, _, _ = _run_adam(n, (0.9, 0.999))                       # double betas
    p, m, v = R.d64(C.adam_inputs(n)["p"]), torch.zeros(n, dtype=D), torch.zeros(n, dtype=D)
    worst, typical, e1 = 0.0, [], torch.zeros(n, dtype=D)
    inp = C.adam_inputs(n)
    for t in range(1, 8):
        ss, bc = C.adam_scalars(t)
        # the kernel's Adam: fl32 betas; step_size and bc2_sqrt in double here, so that only the betas differ between the two sides
        g = R.d64(inp["grads"][t - 1]).clone()
        g[n // 2] += float(inp["extras"][t - 1][0])
        g = g * inp["grad_scale"][t - 1]
        b1r = float(np.float32(0.9))
        e1 = b1r * e1 + abs(b1r - 0.9) * (m.abs() + g.abs())          # beta1's rounding in m: E_t = b1 E_(t-1) + |d b1| (|m_(t-1)| + |g_t|)
        m = b1r * m + (1.0 - b1r) * g
        v = b2r * v + (1.0 - b2r) * g * g
        denom = v.sqrt() / bc + float(np.float32(1e-8))
        upd = ss * (m / denom)
        err = (upd - ups_t[t - 1]).abs()
        allowed = bound * ups_t[t - 1].abs() + ss * e1 / denom
        nz = allowed > 0
        assert bool((err[~nz] == 0).all())
        worst = max(worst, float((err[nz] / allowed[nz]).max()))
        big = ups_t[t - 1].abs() > 0.1 * C.ADAM_HP["lr"]                          # elements whose first moment does not cancel: beta2's rounding alone
        typical.append(float((err[big] / ups_t[t - 1].abs()[big]).median()) / bound)
    print(f"beta rounding: worst |d update| / allowed = {worst:.2f}; median |d update| / |update| = {min(typical):.2f} .. {max(typical):.2f} of "
          f"the bound {bound:.3e}")
    assert worst <= 1.0 and 0.4 <= min(typical) and max(typical) <= 0.6          # (a real, measurable distance: half the bound, not zero)


# ---- the fp32 twins stay below half of every gate ---------------------------------------------------------------------------------------------
OPS = [T.Ops(False), T.Ops(True)]
HALF = 0.5


def _ratio(got, ref, gate):
    """max |got - ref| / gate over all elements; 0 / 0 counts as 0, anything / 0 as inf."""
    err = (R.d64(np.asarray(got, np.float64)).reshape(-1) - torch.as_tensor(ref, dtype=D).reshape(-1)).abs()
    gate = torch.as_tensor(gate, dtype=D).reshape(-1).expand_as(err)
    r = torch.where(err == 0, torch.zeros_like(err), err / gate)
    return float(r.max()) if r.numel() else 0.0


@pytest.mark.parametrize("N", C.POINT_N + (4000,))
def test_twin_points_below_half_gate(N):
    inp = C.points_inputs(N)
    x, t, valid, inside = R.aux_points(inp["rays"], inp["depth_gt"], inp["mask"], inp["d_i"], inp["u"], inp["rad"])
    gate = C.gate_points(inp)
    for op in OPS:
        tx, tv, ti = T.aux_points(op, inp["rays"], inp["depth_gt"], inp["mask"], inp["d_i"], inp["u"], inp["rad"])
        assert _ratio(tx, x, gate) < HALF, (op.fused, _ratio(tx, x, gate))
        assert np.array_equal(tv, valid.numpy()) and np.array_equal(ti.astype(np.float64), inside.numpy())


@pytest.mark.parametrize("variant", ["mixed", "none_inside", "all_inside"])
@pytest.mark.parametrize("N", C.LOSS_N)
def test_twin_eod_below_half_gate(N, variant):
    inp = C.eod_inputs(N, variant)
    args = [inp[k] for k in ("rays", "pts", "mask", "sdf", "go")]
    for gs, ga in ((0.7, -1.3), (0.0, 2.0), (1.5, 0.0), (0.0, 0.0)):
        ref = R.eod_loss(*args, gs, ga)
        gate, gate_b = C.gate_eod(inp, ref), C.gate_eod_bwd(inp, ref, gs, ga)
        for op in OPS:
            f = T.eod_loss(op, *args)
            for k in ("sdf_err", "ang_err", "den"):
                assert _ratio(f[k], ref[k], gate[k]) < HALF, (k, op.fused)
            assert np.array_equal(f["inside"].astype(np.float64), ref["inside"].numpy())
            b = T.eod_loss_bwd(op, inp["rays"], f["inside"], inp["sdf"], inp["go"], f["den"], gs, ga)
            for k in ("d_sdf", "d_go"):
                assert _ratio(b[k], ref[k], gate_b[k]) < HALF, (k, op.fused, _ratio(b[k], ref[k], gate_b[k]))


@pytest.mark.parametrize("variant", ["mixed", "none_valid", "all_valid"])
@pytest.mark.parametrize("N", C.LOSS_N)
def test_twin_sn_below_half_gate(N, variant):
    inp = C.sn_inputs(N, variant)
    ref = R.sn_loss(inp["g"], inp["valid"], 1.7)
    den = float(ref["den"])
    gate = C.sn_term_gate(inp["g"], inp["valid"], N, den)
    gate_b = C.sn_bwd_gate(inp["g"], inp["valid"], N, 1.7 / den)
    for op in OPS:
        f = T.sn_loss(op, inp["g"], inp["valid"])
        assert float(f["den"]) == den and _ratio(f["loss"], ref["loss"], gate) < HALF
        b = T.sn_loss_bwd(op, inp["g"], inp["valid"], f["den"], 1.7)
        assert _ratio(b, ref["d_g"], gate_b) < HALF, (op.fused, _ratio(b, ref["d_g"], gate_b))


def _twin_loss_ratios(inp, ref, tw, N_depth=None, world=1.0):
    gate, gate_g = C.gate_loss_terms(inp, ref, N_depth, world), C.gate_loss_grads(inp, ref, world)
    out = {k: _ratio(tw["terms"][i], ref["terms"][k], gate[k]) for i, k in enumerate(("color", "depth", "sdf", "angle", "eikonal", "surf_neig"))}
    out["total"] = _ratio(tw["terms"][6], ref["total"], gate["total"])
    out.update({k: _ratio(tw[k], ref[k], gate_g[k]) for k in gate_g})
    return out


@pytest.mark.parametrize("variant", ["mixed", "masks_zero", "none_valid", "all_valid"])
@pytest.mark.parametrize("N", C.LOSS_N)
def test_twin_train_loss_below_half_gate(N, variant):
    inp = C.loss_inputs(N, variant)
    ref = C.loss_ref(inp)
    for op in OPS:
        tw = T.train_loss(op, inp, ref["w"])
        assert [float(x) for x in tw["den"]] == ref["den"] and float(tw["terms"][7]) == ref["n_valid"]
        r = _twin_loss_ratios(inp, ref, tw)
        assert max(r.values()) < HALF, (op.fused, r)


def test_twin_train_loss_exact_mode_below_half_gate():
    a, b = C.loss_inputs(1025, "mixed", seed=3), C.loss_inputs(300, "mixed", seed=4)
    cat = C.concat_parts(a, b)
    rc = C.loss_ref(cat)
    for op in OPS:
        da, db = T.train_loss(op, a, C.LOSS_W)["den"], T.train_loss(op, b, C.LOSS_W)["den"]
        den = (da + db).astype(np.float32)
        ta, tb = T.train_loss(op, a, rc["w"], den, 2.0), T.train_loss(op, b, rc["w"], den, 2.0)
        mean = dict(terms=(ta["terms"].astype(np.float64) + tb["terms"]) / 2)
        for k in ("g_color", "g_depth"):
            mean[k] = np.concatenate([ta[k], tb[k]], 0).astype(np.float64) / 2
        for k in ("g_aux_sdf", "g_aux_go"):
            mean[k] = C.cat3(ta[k], tb[k]).astype(np.float64) / 2
        r = _twin_loss_ratios(cat, rc, mean, N_depth=1025)
        assert max(r.values()) < HALF, (op.fused, r)


@pytest.mark.parametrize("n", C.ADAM_N)
def test_twin_adam_below_half_gate(n):
    inp, hp = C.adam_inputs(n), C.ADAM_HP
    for op in OPS:
        p, m, v = inp["p"].copy(), np.zeros(n, np.float32), np.zeros(n, np.float32)
        worst = [0.0, 0.0, 0.0]
        for t in range(1, 8):
            g, ex, gs = inp["grads"][t - 1], inp["extras"][t - 1], inp["grad_scale"][t - 1]
            ss, bc = C.adam_scalars(t)
            rp, rm, rv, upd = R.adam(p, g, m, v, hp["beta1"], hp["beta2"], hp["eps"], ss, bc, gs, ex, n // 2)
            g_eff = R.d64(g).clone()
            g_eff[n // 2] += float(ex[0])
            gates = C.gate_adam(rp, rm, rv, upd, g_eff * R.fl32(gs), hp["beta1"])
            p, m, v = T.adam(op, p, g, m, v, hp["beta1"], hp["beta2"], hp["eps"], ss, bc, gs, ex, n // 2)
            assert np.isfinite(p).all() and np.isfinite(v).all()
            for i, (got, ref, gate) in enumerate(zip((p, m, v), (rp, rm, rv), gates)):
                worst[i] = max(worst[i], _ratio(got, ref, gate))
        assert max(worst) <= HALF, (op.fused, worst)


def test_twin_schedule_and_finish_below_half_gate():
    for name, (s0, t0), steps, kw in C.schedule_cases():
        for k in range(1, steps + 1):
            s = R.schedule(s0 + k, t0 + k, kw["lr_init"], kw["n_iter"], kw["warm_up_end"], kw["lr_alpha"], 0.9, 0.999, 0.5, kw["anneal_end"])
            got = np.asarray(s, np.float32)
            assert _ratio(got, s, [2 * C.U * abs(x) for x in s]) <= HALF, (name, k)
    for acc in ((3.7, 1200.0), (0.0, 0.0), (1e-3, 1.0)):
        acc32 = np.asarray(acc, np.float32)
        eik, den = R.render_finish(acc32)
        d32 = acc32[1] + np.float32(1e-6)
        assert abs(float(d32) - den) <= 2 * C.U * den and abs(float(acc32[0] / d32) - float(acc32[0]) / float(d32)) <= C.U * abs(eik)
