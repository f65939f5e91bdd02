"""The small launches that hold a training step together, each ALONE through the C ABI against the fp64 references of
tests/step_ref.py (pinned to the oracle's own code by tests/test_step_ref_host.py):

  aux.hip    es_eod_points, es_sn_points, es_eod_loss (+ backward), es_sn_loss (+ backward), es_copy2
  rays.hip   es_train_aux_points          loss.hip   es_train_loss          step.hip   es_render_finish
  optim.hip  es_adam_step, es_adam_step_dev, es_train_schedule

Every output buffer has 64 guard elements behind it and is filled with a sentinel first; the guards and every element the kernel has no
business writing must still hold it.  No element is excluded from a comparison.  The gates are the derived ones of tests/step_cases.py
(inputs and derivations there; the numpy fp32 twins of the kernels stay below half of each on the same inputs).  Worst error / gate per
case is written to step_kernels.json in the log directory of test_gpu_backward.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import step_cases as SC
import step_ref as R
from test_gpu_backward import LOG

pytestmark = pytest.mark.gpu
SENT = -12345.6787109375
GUARD = 64
_REPORT = {}
F32 = torch.float32


def _note(case, **values):
    _REPORT.setdefault(case, {}).update(values)
    os.makedirs(LOG, exist_ok=True)
    with open(os.path.join(LOG, "step_kernels.json"), "w") as f:
        json.dump(_REPORT, f, indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def lib():
    from endosurf_amd import _lib
    return _lib.load()


def P(t, offset_bytes=0):
    if t is None:
        return None
    assert t.is_contiguous()
    return C.c_void_p(t.data_ptr() + offset_bytes)


def ST():
    from endosurf_amd import _lib
    return _lib.stream_ptr()


def dev(a):
    if a.dtype == np.bool_:
        a = a.astype(np.uint8)
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def out(n, dtype=F32):
    """n elements + the guard, all sentinel (0xA5 for bytes)."""
    if dtype == torch.uint8:
        return torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    return torch.full((n + GUARD,), SENT, dtype=dtype, device="cuda")


def untouched(buf, start=0):
    """buf[start:] still holds the sentinel bit for bit."""
    t = buf[start:]
    return bool((t == (0xA5 if buf.dtype == torch.uint8 else SENT)).all())


def ratio(got, ref, gate):
    """max |got - ref| / gate over ALL elements (0 / 0 = 0, x / 0 = inf); non-finite output counts as inf."""
    got = got.detach().cpu().to(torch.float64).reshape(-1)
    ref = torch.as_tensor(ref, dtype=torch.float64).reshape(-1)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if got.numel() == 0:
        return 0.0
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    err = (got - ref).abs()
    gate = torch.as_tensor(gate, dtype=torch.float64).reshape(-1).expand_as(err)
    return float(torch.where(err == 0, torch.zeros_like(err), err / gate).max())


def ok(status):
    assert status == 0, status


# ------------------------------------------------------------------------------------------------------------------------------------
# points: es_train_aux_points, es_eod_points (with and without ``inside``), es_sn_points against the same step_ref.aux_points
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SC.POINT_N)
def test_point_kernels(lib, N):
    inp = SC.points_inputs(N)
    x, t, valid, inside = R.aux_points(inp["rays"], inp["depth_gt"], inp["mask"], inp["d_i"], inp["u"], inp["rad"])
    gate = SC.gate_points(inp)
    rays, dg, mask, di, u = (dev(inp[k]) for k in ("rays", "depth_gt", "mask", "d_i", "u"))
    t32 = dev(inp["rays"][:, 8]).repeat(3)
    v8 = valid.to(torch.uint8).cuda()
    # the fused launch of the training step
    xf, tf, vf = out(9 * N), out(3 * N), out(N, torch.uint8)
    ok(lib.es_train_aux_points(P(rays), P(dg), P(mask), P(di), P(u), inp["rad"], N, P(xf), P(tf), P(vf), ST()))
    r_f = ratio(xf[:9 * N], x, gate)
    assert r_f <= 1.0, r_f
    assert torch.equal(tf[:3 * N], t32) and torch.equal(vf[:N], v8)
    assert untouched(xf, 9 * N) and untouched(tf, 3 * N) and untouched(vf, N)
    # errorondepth's points, with the inside mask and without
    xe, te, ie = out(3 * N), out(N), out(N)
    ok(lib.es_eod_points(P(rays), P(dg), P(mask), N, P(xe), P(te), P(ie), ST()))
    r_e = ratio(xe[:3 * N], x[:N], gate[:N])
    assert r_e <= 1.0, r_e
    assert torch.equal(te[:N], t32[:N]) and torch.equal(ie[:N].cpu().double(), inside)
    for r in inp["sphere_rows"][:3]:
        assert float(ie[r]) == 0.0          # exactly ON the sphere: not inside
    for r in inp["sphere_rows"][3:]:
        assert float(ie[r]) == 1.0          # one ulp inside
    assert untouched(xe, 3 * N) and untouched(te, N) and untouched(ie, N)
    xe2, te2 = out(3 * N), out(N)
    ok(lib.es_eod_points(P(rays), P(dg), None, N, P(xe2), P(te2), None, ST()))
    assert torch.equal(xe2, xe) and torch.equal(te2, te)
    # surface points and neighbours: rows [0, 2N) only
    xs, ts, vs = out(6 * N), out(2 * N), out(N, torch.uint8)
    ok(lib.es_sn_points(P(rays), P(mask), P(di), P(u), inp["rad"], N, P(xs), P(ts), P(vs), ST()))
    r_s = ratio(xs[:6 * N], x[N:], gate[N:])
    assert r_s <= 1.0, r_s
    assert torch.equal(ts[:2 * N], t32[:2 * N]) and torch.equal(vs[:N], v8)
    assert untouched(xs, 6 * N) and untouched(ts, 2 * N) and untouched(vs, N)
    _note(f"points_N{N}", train_aux_points=r_f, eod_points=r_e, sn_points=r_s, redraws=inp["redraws"],
          fused_rows_bit_identical_to_standalone=bool(torch.equal(xf[:3 * N], xe[:3 * N]) and torch.equal(xf[3 * N:9 * N], xs[:6 * N])))


# ------------------------------------------------------------------------------------------------------------------------------------
# es_eod_loss / es_eod_loss_backward
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["mixed", "none_inside", "all_inside"])
@pytest.mark.parametrize("N", SC.LOSS_N)
def test_eod_loss_kernels(lib, N, variant):
    inp = SC.eod_inputs(N, variant)
    args = [inp[k] for k in ("rays", "pts", "mask", "sdf", "go")]
    rays, pts, mask, sdf, go = (dev(a) for a in args)
    o, ins = out(3), out(N)
    ok(lib.es_eod_loss(P(rays), P(pts), P(mask), P(sdf), P(go), N, P(o), P(ins), ST()))
    ref = R.eod_loss(*args)
    gate = SC.gate_eod(inp, ref)
    rr = dict(sdf_err=ratio(o[0], ref["sdf_err"], gate["sdf_err"]), ang_err=ratio(o[1], ref["ang_err"], gate["ang_err"]),
              den=ratio(o[2], ref["den"], gate["den"]))
    assert max(rr.values()) <= 1.0, rr
    assert torch.equal(ins[:N].cpu().double(), ref["inside"]) and untouched(o, 3) and untouched(ins, N)
    if variant == "none_inside":
        assert float(o[0]) == 0.0 and float(o[2]) == float(np.float32(1e-6))
    for name, gs, ga in (("both", 0.7, -1.3), ("no_ang", 1.5, None), ("no_sdf", None, 2.0), ("neither", None, None)):
        g1 = None if gs is None else dev(np.asarray([gs], np.float32))
        g2 = None if ga is None else dev(np.asarray([ga], np.float32))
        d_sdf, d_go = out(N), out(3 * N)
        ok(lib.es_eod_loss_backward(P(rays), P(ins), P(sdf), P(go), P(o), P(g1), P(g2), N, P(d_sdf), P(d_go), ST()))
        rb = R.eod_loss(*args, R.fl32(gs or 0.0), R.fl32(ga or 0.0))
        gb = SC.gate_eod_bwd(inp, rb, R.fl32(gs or 0.0), R.fl32(ga or 0.0))
        rr[f"d_sdf_{name}"], rr[f"d_go_{name}"] = ratio(d_sdf[:N], rb["d_sdf"], gb["d_sdf"]), ratio(d_go[:3 * N], rb["d_go"], gb["d_go"])
        assert rr[f"d_sdf_{name}"] <= 1.0 and rr[f"d_go_{name}"] <= 1.0, (name, rr)
        assert untouched(d_sdf, N) and untouched(d_go, 3 * N)
        if gs is None or variant == "none_inside":
            assert float(d_sdf[:N].abs().max()) == 0.0
        if ga is None:
            assert float(d_go[:3 * N].abs().max()) == 0.0
        if variant != "none_inside" and N >= 4:
            assert float(d_sdf[1]) == 0.0 and float(d_go[6:9].abs().max()) == 0.0          # sgn(0) = 0; relu'(0) = 0 at cos exactly 0
            if gs is not None:
                assert float(d_sdf[3]) < 0.0          # inside * sdf negative
    _note(f"eod_loss_N{N}_{variant}", redraws=inp["redraws"], **rr)


# ------------------------------------------------------------------------------------------------------------------------------------
# es_sn_loss / es_sn_loss_backward
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["mixed", "none_valid", "all_valid"])
@pytest.mark.parametrize("N", SC.LOSS_N)
def test_sn_loss_kernels(lib, N, variant):
    inp = SC.sn_inputs(N, variant)
    g, v8 = dev(inp["g"]), dev(inp["valid"])
    o = out(2)
    ok(lib.es_sn_loss(P(g), P(v8), N, P(o), ST()))
    ref = R.sn_loss(inp["g"], inp["valid"], R.fl32(1.7))
    den = float(ref["den"])
    assert float(o[1]) == den and untouched(o, 2)
    rr = dict(loss=ratio(o[0], ref["loss"], SC.sn_term_gate(inp["g"], inp["valid"], N, den)))
    gl = dev(np.asarray([1.7], np.float32))
    d_g = out(6 * N)
    ok(lib.es_sn_loss_backward(P(g), P(v8), P(o), P(gl), N, P(d_g), ST()))
    rr["d_g"] = ratio(d_g[:6 * N], ref["d_g"], SC.sn_bwd_gate(inp["g"], inp["valid"], N, R.fl32(1.7) / den))
    assert max(rr.values()) <= 1.0, rr
    assert untouched(d_g, 6 * N)
    inv = (~torch.from_numpy(inp["valid"])).cuda()
    rows = d_g[:6 * N].view(2, N, 3)
    assert float(rows[:, inv].abs().sum()) == 0.0          # invalid rows: exactly 0 in both halves
    if variant == "none_valid":
        assert float(o[0]) == 0.0 and den == 1.0 and float(d_g[:6 * N].abs().max()) == 0.0
    _note(f"sn_loss_N{N}_{variant}", **rr)


# ------------------------------------------------------------------------------------------------------------------------------------
# es_train_loss
# ------------------------------------------------------------------------------------------------------------------------------------
_G = (("g_color", 3), ("g_depth", 1), ("g_aux_sdf", 3), ("g_aux_go", 9))


def _loss_launch(lib, d, N, w, den_out=None, den_global=None, world=0.0):
    """One es_train_loss on device inputs ``d`` -> (status, sentinel-backed outputs)."""
    from endosurf_amd import _lib
    o = dict(terms=out(8), total_out=out(1), g_eik=out(1))
    o.update({k: out(m * max(N, 0)) for k, m in _G})
    a = _lib.es_loss_args()
    for k in SC.LOSS_ARGS:
        setattr(a, k, P(d.get(k)))
    a.N = N
    a.w_color, a.w_depth, a.w_sdf, a.w_angle, a.w_eik, a.w_sn = (float(w[k]) for k in R.LOSS_KEYS)
    for k, t in o.items():          # (an empty batch's per-ray outputs may be null)
        setattr(a, k, None if (N == 0 and k in dict(_G)) else P(t))
    a.den_out, a.den_global, a.world = P(den_out), P(den_global), float(world)
    return lib.es_train_loss(C.byref(a), ST()), o


def _loss_ratios(inp, ref, terms, grads, N_depth=None, world=1.0):
    gate, gate_g = SC.gate_loss_terms(inp, ref, N_depth, world), SC.gate_loss_grads(inp, ref, world)
    rr = {k: ratio(terms[i], ref["terms"][k], gate[k]) for i, k in enumerate(R.LOSS_KEYS)}
    rr["total"] = ratio(terms[6], ref["total"], gate["total"])
    rr.update({k: ratio(grads[k], ref[k], gate_g[k]) for k in gate_g})
    return rr


@pytest.mark.parametrize("variant", ["mixed", "masks_zero", "none_valid", "all_valid"])
@pytest.mark.parametrize("N", SC.LOSS_N)
def test_train_loss_kernel(lib, N, variant):
    inp = SC.loss_inputs(N, variant)
    ref = SC.loss_ref(inp)
    d = {k: dev(inp[k]) for k in SC.LOSS_ARGS}
    st, o = _loss_launch(lib, d, N, ref["w"])
    ok(st)
    terms = o["terms"][:8].cpu()
    rr = _loss_ratios(inp, ref, terms, {k: o[k][:m * N] for k, m in _G})
    assert max(rr.values()) <= 1.0, rr
    assert bool(torch.isfinite(terms).all())
    assert float(terms[7]) == ref["n_valid"] and float(o["g_eik"][0]) == ref["w"]["eikonal"] and float(terms[4]) == float(inp["eik"][0])
    assert o["total_out"][:1].view(torch.int32).item() == o["terms"][6:7].view(torch.int32).item()          # bit for bit
    assert float(o["g_aux_sdf"][N:3 * N].abs().max()) == 0.0
    for k, t in o.items():
        n = dict(_G).get(k, 0) * N or dict(terms=8, total_out=1, g_eik=1)[k]
        assert untouched(t, n), k
    inv = (~torch.from_numpy(inp["valid_sn"])).cuda()
    assert float(o["g_aux_go"][3 * N:9 * N].view(2, N, 3)[:, inv].abs().sum()) == 0.0
    if variant == "masks_zero":          # denominators 1e-10 (1e-6 for the unmasked angle term): the masked adjoints are exactly 0, nothing non-finite
        assert float(terms[0]) == 0.0 and float(terms[1]) == 0.0 and float(terms[2]) == 0.0
        for k in ("g_color", "g_depth", "g_aux_sdf"):
            assert float(o[k][:dict(_G)[k] * N].abs().max()) == 0.0, k
        assert bool(torch.isfinite(o["g_aux_go"][:9 * N]).all())
    if variant == "none_valid":
        assert float(terms[5]) == 0.0 and float(o["g_aux_go"][3 * N:9 * N].abs().max()) == 0.0
    if variant == "mixed":
        gc = o["g_color"][:3 * N].view(N, 3)
        assert float(gc[::4, 1].abs().max()) == 0.0 and float(o["g_depth"][:N][::5].abs().max()) == 0.0          # sgn(0) = 0
        if N >= 4:
            assert float(o["g_aux_sdf"][1]) == 0.0 and float(o["g_aux_go"][6:9].abs().max()) == 0.0
    _note(f"train_loss_N{N}_{variant}", redraws=inp["redraws"], **rr)


def test_train_loss_exact_mode_in_one_process(lib):
    """den_out on each of two unequal parts, the normalisers summed, den_global + world = 2 on each part: the mean over the parts of
    (terms, adjoints / world) is step_ref.train_loss of the concatenated batch."""
    a, b = SC.loss_inputs(1025, "mixed", seed=3), SC.loss_inputs(300, "mixed", seed=4)
    cat = SC.concat_parts(a, b)
    ref = SC.loss_ref(cat)
    dens, devs = [], []
    for part in (a, b):
        N = part["rays"].shape[0]
        d = {k: dev(part[k]) for k in SC.LOSS_ARGS}
        den = out(4)
        st, o = _loss_launch(lib, d, N, ref["w"], den_out=den)
        ok(st)
        assert untouched(den, 4) and all(untouched(t) for t in o.values())          # its four floats and nothing else
        dens.append(den[:4].clone()); devs.append(d)
    den_g = (dens[0] + dens[1]).contiguous()
    assert [float(x) for x in den_g] == ref["den"]
    res = []
    for part, d in zip((a, b), devs):
        N = part["rays"].shape[0]
        st, o = _loss_launch(lib, d, N, ref["w"], den_global=den_g, world=2.0)
        ok(st)
        res.append({k: (o[k][:dict(_G).get(k, 0) * N or 8].cpu().double()) for k in ("terms", "g_color", "g_depth", "g_aux_sdf", "g_aux_go")})
    ra, rb = res
    shp = dict(g_color=3, g_depth=1, g_aux_sdf=1, g_aux_go=3)
    terms = (ra["terms"] + rb["terms"]) / 2
    grads = {k: torch.cat([ra[k].view(-1, shp[k]), rb[k].view(-1, shp[k])], 0) / 2 for k in ("g_color", "g_depth")}
    grads.update({k: SC.cat3(ra[k].view(-1, shp[k]), rb[k].view(-1, shp[k])) / 2 for k in ("g_aux_sdf", "g_aux_go")})
    rr = _loss_ratios(cat, ref, terms, grads, N_depth=1025)
    assert max(rr.values()) <= 1.0, rr
    _note("train_loss_exact_mode_1025+300", **rr)


def test_train_loss_empty_batch(lib):
    """N == 0 launches: five terms 0, terms[4] = eik, terms[6] = total_out = w_eik * eik, terms[7] = 0, g_eik = w_eik, den_out four zeros;
    N < 0 is refused with the buffers untouched."""
    w = {k: R.fl32(v) for k, v in SC.LOSS_W.items()}
    eik = np.asarray([0.0371], np.float32)
    d = dict(eik=dev(eik))
    st, o = _loss_launch(lib, d, 0, w)
    ok(st)
    t = o["terms"][:8].cpu()
    assert [float(t[i]) for i in (0, 1, 2, 3, 5, 7)] == [0.0] * 6 and float(t[4]) == float(eik[0])
    assert float(t[6]) == float(np.float32(w["eikonal"]) * eik[0]) == float(o["total_out"][0]) and float(o["g_eik"][0]) == w["eikonal"]
    assert untouched(o["terms"], 8) and untouched(o["total_out"], 1) and untouched(o["g_eik"], 1)
    den = out(4)
    st, o = _loss_launch(lib, d, 0, w, den_out=den)
    ok(st)
    assert den[:4].tolist() == [0.0] * 4 and untouched(den, 4) and all(untouched(x) for x in o.values())
    st, o = _loss_launch(lib, d, -1, w)
    assert st != 0 and all(untouched(x) for x in o.values())


# ------------------------------------------------------------------------------------------------------------------------------------
# es_render_finish, es_copy2
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("acc", [(3.7, 1200.0), (0.25, 0.0)])
@pytest.mark.parametrize("n_aux", SC.FINISH_N)
def test_render_finish(lib, n_aux, acc):
    rng = np.random.default_rng(n_aux)
    acc32 = np.asarray(acc, np.float32)
    src_s, src_g = rng.standard_normal(n_aux + 7).astype(np.float32), rng.standard_normal(3 * n_aux + 7).astype(np.float32)
    ds, dg_ = (dev(src_s), dev(src_g)) if n_aux else (None, None)
    eik, den2, a_sdf, a_go = out(1), out(2), out(n_aux), out(3 * n_aux)
    acc_d = dev(acc32)
    ok(lib.es_render_finish(P(acc_d), P(ds), P(dg_), n_aux, P(eik), P(den2), P(a_sdf) if n_aux else None, P(a_go) if n_aux else None, ST()))
    den32 = acc32[1] + np.float32(1e-6)
    assert float(den2[0]) == float(den32) == float(den2[1])
    want = float(acc32[0]) / float(den32)
    assert abs(float(eik[0]) - want) <= float(np.spacing(np.float32(want)))          # 1 ulp
    assert abs(float(eik[0]) - R.render_finish(acc32)[0]) <= 4 * SC.U * abs(R.render_finish(acc32)[0])
    if n_aux:
        assert torch.equal(a_sdf[:n_aux], ds[:n_aux]) and torch.equal(a_go[:3 * n_aux], dg_[:3 * n_aux])
    assert untouched(eik, 1) and untouched(den2, 2) and untouched(a_sdf, n_aux) and untouched(a_go, 3 * n_aux)


@pytest.mark.parametrize("na,nb", SC.COPY2)
def test_copy2(lib, na, nb):
    rng = np.random.default_rng(na + nb)
    sa, sb = dev(rng.standard_normal(na + 5).astype(np.float32)), dev(rng.standard_normal(nb + 5).astype(np.float32))
    da, db = out(na), out(nb)
    ok(lib.es_copy2(P(da) if na else None, P(sa) if na else None, na, P(db) if nb else None, P(sb) if nb else None, nb, ST()))
    assert torch.equal(da[:na], sa[:na]) and torch.equal(db[:nb], sb[:nb]) and untouched(da, na) and untouched(db, nb)


# ------------------------------------------------------------------------------------------------------------------------------------
# es_train_schedule: one launch per step, the state carried on the device
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SC.schedule_cases(), ids=lambda c: c[0])
def test_train_schedule(lib, case):
    name, (s0, t0), steps, kw = case
    b1, b2, gs = 0.9, 0.999, 0.5
    state = out(2, torch.float64)
    state[:2] = torch.tensor([s0, t0], dtype=torch.float64)
    scal = out(4 * steps)
    for k in range(steps):
        ok(lib.es_train_schedule(P(state), kw["lr_init"], float(kw["n_iter"]), float(kw["warm_up_end"]), kw["lr_alpha"], b1, b2, gs, float(kw["anneal_end"]),
                                 P(scal, 16 * k), ST()))
    got = scal[:4 * steps].cpu().view(steps, 4)
    worst = 0.0
    for k in range(steps):
        s = R.schedule(s0 + k + 1, t0 + k + 1, kw["lr_init"], kw["n_iter"], kw["warm_up_end"], kw["lr_alpha"], b1, b2, gs, kw["anneal_end"])
        r = ratio(got[k], s, [2 * SC.U * abs(x) for x in s])          # gate E
        assert r <= 1.0, (name, k + 1, got[k].tolist(), s)
        worst = max(worst, r)
    assert state[:2].tolist() == [s0 + steps, t0 + steps] and untouched(state, 2) and untouched(scal, 4 * steps)
    _note(f"schedule_{name}", worst=worst)


def test_train_schedule_refuses_bad_arguments(lib):
    state = out(2, torch.float64)
    state[:2] = 0.0
    scal = out(4)
    for n_iter, warm in ((4.0, 4.0), (3.0, 4.0), (40.0, -1.0)):
        assert lib.es_train_schedule(P(state), 1e-3, n_iter, warm, 0.05, 0.9, 0.999, 1.0, 0.0, P(scal), ST()) != 0
    assert untouched(scal) and state[:2].tolist() == [0.0, 0.0] and untouched(state, 2)


# ------------------------------------------------------------------------------------------------------------------------------------
# es_adam_step / es_adam_step_dev
# ------------------------------------------------------------------------------------------------------------------------------------
_ADAM_CASES = [(1, None), (1, 0), (255, None), (255, 0), (255, 254), (255, 77), (256, None), (256, 255), (257, 256), (257, 77),
               (100003, None), (100003, 0), (100003, 100002), (100003, 77), (100003, 65537)]


@pytest.mark.parametrize("n,extra_index", _ADAM_CASES)
def test_adam_kernels(lib, n, extra_index):
    inp, hp = SC.adam_inputs(n), SC.ADAM_HP
    bufs = [[out(n) for _ in range(3)] for _ in range(2)]          # (p, m, v) of es_adam_step and of es_adam_step_dev
    for p, m, v in bufs:
        p[:n] = dev(inp["p"]); m[:n] = 0.0; v[:n] = 0.0
    worst = [0.0, 0.0, 0.0]
    for t in range(1, 8):
        g_np, ex_np, gs = inp["grads"][t - 1], inp["extras"][t - 1], inp["grad_scale"][t - 1]
        g, ex = dev(g_np), (None if extra_index is None else dev(ex_np))
        ss, bc = SC.adam_scalars(t)
        p, m, v = bufs[0]
        rp, rm, rv, upd = R.adam(p[:n], g, m[:n], v[:n], hp["beta1"], hp["beta2"], hp["eps"], ss, bc, gs, None if extra_index is None else ex_np,
                                 extra_index or 0)
        g_eff = R.d64(g_np).clone()
        if extra_index is not None:
            g_eff[extra_index] += float(ex_np[0])
        gates = SC.gate_adam(rp, rm, rv, upd, g_eff * R.fl32(gs), hp["beta1"])
        ok(lib.es_adam_step(P(p), P(g), P(m), P(v), n, hp["beta1"], hp["beta2"], hp["eps"], ss, bc, gs, P(ex), extra_index or 0, ST()))
        scal = dev(np.asarray([ss, bc, gs], np.float32))
        p2, m2, v2 = bufs[1]
        ok(lib.es_adam_step_dev(P(p2), P(g), P(m2), P(v2), n, hp["beta1"], hp["beta2"], hp["eps"], P(scal), P(ex), extra_index or 0, ST()))
        for i, (got, ref, gate) in enumerate(zip((p, m, v), (rp, rm, rv), gates)):
            r = ratio(got[:n], ref, gate)          # gate D, per step: both sides started from the kernel's fp32 state
            assert r <= 1.0, (t, "pmv"[i], r)
            worst[i] = max(worst[i], r)
        for x, y in zip(bufs[0], bufs[1]):
            assert torch.equal(x, y)          # the same kernel fed through ``scal``: bit-identical, guards included
        assert all(untouched(x, n) for x in bufs[0])
    _note(f"adam_n{n}_extra{extra_index}", p=worst[0], m=worst[1], v=worst[2])


def test_adam_refuses_extra_index_out_of_range(lib):
    n = 300
    hp = SC.ADAM_HP
    p, g, m, v = (dev(np.random.default_rng(i).standard_normal(n).astype(np.float32)) for i in range(4))
    v = v.abs()
    keep = [x.clone() for x in (p, m, v)]
    ex, scal = dev(np.asarray([1.0], np.float32)), dev(np.asarray([1e-3, 1.0, 1.0], np.float32))
    for idx in (n, -1, n + 1000):
        assert lib.es_adam_step(P(p), P(g), P(m), P(v), n, hp["beta1"], hp["beta2"], hp["eps"], 1e-3, 1.0, 1.0, P(ex), idx, ST()) != 0
        assert lib.es_adam_step_dev(P(p), P(g), P(m), P(v), n, hp["beta1"], hp["beta2"], hp["eps"], P(scal), P(ex), idx, ST()) != 0
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip((p, m, v), keep))
