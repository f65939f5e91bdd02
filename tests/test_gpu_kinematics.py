"""GPU: tissue velocity and strain rate.  Kernel level through the C ABI -- es_deform_derivatives (csrc/deform_jet.hip)
bit for bit against es_deform_jacobian and against the fp64 reference of ``kinematics_ref`` on rows screened away from the ReLU kinks,
es_kinematics_rows (csrc/kinematics.hip) against the fp64 numpy twin ``kinematics.kinematics_rows`` -- then Engine and renderer.
Every test prints the figures it asserts on."""
import ctypes as C

import numpy as np
import pytest
import torch

import weightgen
from gpu_util import renderer_for
from kinematics_ref import derivatives, derivs_fn
from shapes_util import FORWARD_GATE
from test_gpu_strain import CASES, Dev, _patch, close, deform_margin, screened
from test_kinematics_host import hand_rows
from track_util import assert_contraction, deform_fn, draw, oracle_net

from endosurf_amd import kinematics, tracking

pytestmark = pytest.mark.gpu

M = 200
HALF_MAX_POINTS = 3072          # 4-point (32-row) tiles up to here, 8-point (64-row) tiles above (csrc/deform_jet.hip)
MARGIN = 4.0                    # x the worst-row error of the oracle's own fp32 run: the yardstick of 7i's end-to-end test
RTOL, ATOL = 2.4e-7, 1e-13      # two fp32 ulps: the kernel's fp64 error is far below half an ulp, only the final rounding can differ
OUTS = ("jac", "d_t", "dd", "xc")
ROW_KEYS = ("velocity", "speed", "L", "rate", "principal_rates", "divergence", "vorticity", "area_rate", "surface_rates", "valid")
BARE_KEYS = tuple(k for k in ROW_KEYS if k not in ("area_rate", "surface_rates"))


def derivs_dev(dev, x, t, want=OUTS):
    """es_deform_derivatives at fp32 host points: dict(jac [M,3,3], d_t [M,3], dd [M,3,3], xc [M,3]) of the outputs in ``want`` as host
    tensors; ``t`` [M] or [1] (read as t_scalar).  Unwritten entries would stay NaN."""
    _lib, n = dev._lib, x.shape[0]
    ptr = _lib.ptr
    shapes = {"jac": (n, 3, 3), "d_t": (n, 3), "dd": (n, 3, 3), "xc": (n, 3)}
    out = {k: torch.full(shapes[k], float("nan"), device="cuda") for k in want}
    p = _lib.es_points()
    xd, td = x.cuda().contiguous(), t.reshape(-1).cuda().contiguous()
    assert td.numel() in (1, n)
    p.x, p.t, p.mode, p.n_per_ray, p.ldz, p.M = ptr(xd), ptr(td), 0, 1, 1, n
    p.t_scalar = 1 if td.numel() == 1 and n != 1 else 0
    _lib.check(dev.lib.es_deform_derivatives(C.byref(p), ptr(dev.packed), ptr(dev.weff), ptr(out.get("jac")), ptr(out.get("d_t")),
                                             ptr(out.get("dd")), ptr(out.get("xc")), _lib.stream_ptr()), "es_deform_derivatives")
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def rows_dev(jac, d_t, dd, normals):
    """es_kinematics_rows on fp32 host rows: ``kinematics.kinematics_rows``' dict as host tensors (NaN / True where the kernel did not
    write)."""
    from endosurf_amd import _lib
    lib, ptr = _lib.load(), _lib.ptr
    n = jac.shape[0]
    dev = lambda a: None if a is None else a.float().cuda().contiguous()
    j, dt, h, nn = dev(jac), dev(d_t), dev(dd), dev(normals)
    shapes = {"velocity": (n, 3), "speed": (n,), "L": (n, 3, 3), "rate": (n, 3, 3), "principal_rates": (n, 3), "divergence": (n,),
              "vorticity": (n, 3)}
    if normals is not None:
        shapes.update(area_rate=(n,), surface_rates=(n, 2))
    out = {k: torch.full(s, float("nan"), device="cuda") for k, s in shapes.items()}
    out["valid"] = torch.ones(n, dtype=torch.bool, device="cuda")
    _lib.check(lib.es_kinematics_rows(ptr(j), ptr(dt), ptr(h), ptr(nn), n, ptr(out["velocity"]), ptr(out["speed"]), ptr(out["L"]), ptr(out["rate"]),
                                      ptr(out["principal_rates"]), ptr(out["divergence"]), ptr(out["vorticity"]), ptr(out.get("area_rate")),
                                      ptr(out.get("surface_rates")), ptr(out["valid"]), _lib.stream_ptr()), "es_kinematics_rows")
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def worst_row(a, b):
    """The largest entry of |a - b| over the rows, in fp64."""
    return float((a.double() - b.double()).abs().max())


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"{c[1]}{c[0]}")
def case(request):
    """One state: device weights, the fp64 and fp32 oracles, 200 screened rows, the reference derivatives on them in fp64 and in the
    oracle's own fp32 run, and the device's (computed once, shared, never written to)."""
    seed, mode = request.param
    state = weightgen.make_state(seed, mode, True)
    dev, net64, net32 = Dev(state), oracle_net(state, torch.float64), oracle_net(state, torch.float32)
    x, t = screened(net64, M, seed)
    ref64, ref32 = derivatives(net64, x.double(), t.double()), derivatives(net32, x, t)
    yard = {k: worst_row(ref32[k], ref64[k]) for k in ("jac", "d_t", "dd")}
    return dict(seed=seed, mode=mode, dev=dev, net64=net64, x=x, t=t, ref64=ref64, yard=yard, got=derivs_dev(dev, x, t), name=f"{mode}{seed}")


def test_jacobian_and_value_are_the_jacobian_kernels_bits(case):
    """jac_out and xc_out ``torch.equal`` to es_deform_jacobian's, at the sizes around the tile edges and on both tile heights."""
    dev, x, t = case["dev"], case["x"], case["t"]
    for m in (1, 3, 4, 5, 7, 8, 9, 17, 200):
        J, xc = dev.jacobian(x[:m], t[:m])
        got = derivs_dev(dev, x[:m], t[:m])
        assert bool(torch.isfinite(J).all()) and torch.equal(got["jac"], J) and torch.equal(got["xc"], xc), m
    for n in (HALF_MAX_POINTS, HALF_MAX_POINTS + 1, HALF_MAX_POINTS + 9):
        idx = torch.arange(n) % M
        J, xc = dev.jacobian(x[idx], t[idx])
        got = derivs_dev(dev, x[idx], t[idx], want=("jac", "xc"))
        assert torch.equal(got["jac"], J) and torch.equal(got["xc"], xc), n


def test_time_and_second_derivatives_against_the_fp64_reference(case):
    """dt_out and dd_out within 4 x the worst-row error of the oracle's own fp32 run against its fp64 run on the same rows, at the sizes
    around the edges of the 4- and 8-point tiles; J within FORWARD_GATE["v"] as in 7i.  The measured figures are in DESIGN.md 7l."""
    dev, x, t, ref, yard = case["dev"], case["x"], case["t"], case["ref64"], case["yard"]
    for m in (1, 3, 4, 5, 7, 8, 9, 17, 200):
        got = derivs_dev(dev, x[:m], t[:m])
        err = {k: worst_row(got[k], ref[k][:m]) for k in ("jac", "d_t", "dd")}
        print(f"[{case['name']}] M {m:4d}: " + "  ".join(f"{k} {err[k]:.3e} (fp32 oracle {yard[k]:.3e}, gate {MARGIN * yard[k]:.3e})" for k in err))
        assert all(torch.equal(got[k], case["got"][k][:m]) for k in OUTS), m
        assert err["d_t"] <= MARGIN * yard["d_t"] and err["dd"] <= MARGIN * yard["dd"], (m, err, yard)
        assert err["jac"] <= FORWARD_GATE["v"]
    assert float(case["got"]["dd"].abs().max()) > 0.1 and float(case["got"]["d_t"].abs().max()) > 1e-3


def test_rows_do_not_depend_on_their_place_or_neighbours(case):
    """The same rows again, permuted, in a smaller batch and alone: the same bits.  So are the two tile heights: the 200 rows repeated
    to the threshold (the last batch of the 4-point tiles) and to threshold + 1 and + 9 rows (8-point tiles, the last tile one row
    long) come out as in the 200-row batch, so the oracle parity shown on one height holds on the other."""
    dev, x, t, full = case["dev"], case["x"], case["t"], case["got"]
    perm = torch.from_numpy(np.random.default_rng(3).permutation(M).copy())
    again, shuffled = derivs_dev(dev, x, t), derivs_dev(dev, x[perm], t[perm])
    first, alone = derivs_dev(dev, x[:21], t[:21]), derivs_dev(dev, x[117:118], t[117:118])
    for k in OUTS:
        a = full[k]
        assert bool(torch.isfinite(a).all()), k
        assert torch.equal(a, again[k]) and torch.equal(a[perm], shuffled[k]) and torch.equal(a[:21], first[k]) and torch.equal(a[117:118], alone[k]), k
    for n in (HALF_MAX_POINTS, HALF_MAX_POINTS + 1, HALF_MAX_POINTS + 9):
        idx = torch.arange(n) % M
        got = derivs_dev(dev, x[idx], t[idx])
        for k in OUTS:
            assert torch.equal(full[k][idx], got[k]), (k, n)


def test_each_output_alone_and_a_shared_time(case):
    dev, x, t, full = case["dev"], case["x"], case["t"], case["got"]
    for k in OUTS:
        only = derivs_dev(dev, x, t, want=(k,))
        assert set(only) == {k} and torch.equal(only[k], full[k]), k
    shared = derivs_dev(dev, x, t[:1])                                  # read as t_scalar
    per_row = derivs_dev(dev, x, t[:1].expand(M).contiguous())
    for k in OUTS:
        assert torch.equal(shared[k], per_row[k]), k
        assert torch.equal(shared[k][:1], full[k][:1]) and not torch.equal(shared[k][1:], full[k][1:]), k          # (the time is read)


def test_second_and_time_derivatives_against_the_point_adjoint(case):
    """The reverse sweep of the point forward (es_point_vjp) for a random covector g: ES_WS_CURV[k] = -sum_i g_i dd[i][k] and ES_WS_TBAR =
    sum_i g_i d_t[i] -- another kernel, another summation order.  Within FORWARD_GATE["v"] (3e-6) scaled by |g| max|dd| (|g| max|d_t|)."""
    from endosurf_amd import _lib, engine
    dev, full = case["dev"], case["got"]
    eng = engine.Engine(torch.device("cuda", torch.cuda.current_device()))
    g = torch.from_numpy(np.random.default_rng(70 + case["seed"]).normal(size=(M, 3))).float()
    ctx = eng.point_forward(eng.points(x=case["x"].cuda(), t=case["t"].cuda()), dev.weff, dev.packed, _lib.PF_DEFORM, fp32_only=True)
    ctx.view("gc").copy_(g.cuda())
    eng.point_vjp(ctx, dev.weff, dev.packed)
    curv, tbar = ctx.view("curv").cpu().double(), ctx.view("tbar").cpu().double().reshape(M)
    gn = g.double().norm(dim=-1)
    mine_c = torch.einsum("mi,mik->mk", g.double(), full["dd"].double())
    mine_t = (g.double() * full["d_t"].double()).sum(-1)
    s_c, s_t = float(full["dd"].abs().max()), float(full["d_t"].abs().max())
    e_c = float(((mine_c + curv).abs().amax(-1) / (gn * s_c)).max())
    e_t = float(((mine_t - tbar).abs() / (gn * s_t)).max())
    print(f"\n[{case['name']}] sum g dd against -ES_WS_CURV {e_c:.3e}, sum g d_t against ES_WS_TBAR {e_t:.3e} (gate {FORWARD_GATE['v']:.0e}, "
          f"relative to |g| max|dd| = |g| {s_c:.3f} and |g| max|d_t| = |g| {s_t:.3f})")
    assert e_c <= FORWARD_GATE["v"] and e_t <= FORWARD_GATE["v"]


@pytest.fixture(scope="module")
def row_inputs():
    """The device's own derivatives of the seed-11 weights at 257 points of ``track_util.draw``, copied to the host, and normals of any
    length."""
    dev = Dev(weightgen.make_state(11, "trained", True))
    x, t, _ = draw(11, 257)
    d = derivs_dev(dev, x, t)
    n = torch.from_numpy(np.random.default_rng(9).normal(size=(257, 3)) * 3.0).float()
    return d["jac"], d["d_t"], d["dd"], n


@pytest.mark.parametrize("m", [0, 1, 63, 64, 65, 257])
def test_kinematics_rows_against_the_numpy_twin(row_inputs, m):
    jac, d_t, dd, n = (a[:m] for a in row_inputs)
    got, want = rows_dev(jac, d_t, dd, n), kinematics.kinematics_rows(jac, d_t, dd, n)
    assert set(got) == set(want) == set(ROW_KEYS)
    for k in ROW_KEYS:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype and close(got[k], want[k]), (k, m)
    assert bool(want["valid"].all())
    if m:
        worst = max(float(((got[k].double() - want[k].double()).abs() / want[k].double().abs().clamp_min(1e-30)).max())
                    for k in ("speed", "velocity"))
        print(f"\nM {m}: largest relative difference of v to the twin {worst:.3e} (two ulps: {RTOL:.1e}); speed up to "
              f"{float(want['speed'].max()):.3f}, |L| up to {float(want['L'].abs().max()):.3f}")
    again = rows_dev(jac, d_t, dd, n)
    assert all(torch.equal(got[k], again[k]) for k in ROW_KEYS)          # bit-identical from call to call
    # without normals: the same rows and (here) valid, and no surface outputs
    bare = rows_dev(jac, d_t, dd, None)
    assert set(bare) == set(BARE_KEYS) and all(torch.equal(bare[k], got[k]) for k in bare)


def test_kinematics_rows_on_hand_made_rows(row_inputs):
    jac, d_t, dd, n, valid = (a.float() if a.dtype == torch.float64 else a for a in hand_rows())
    # behind 64 ordinary rows, so that the block holds both kinds
    jac, d_t, dd, n = (torch.cat([a[:64], b]) for a, b in zip(row_inputs, (jac, d_t, dd, n)))
    valid = torch.cat([torch.ones(64, dtype=torch.bool), valid])
    got, want = rows_dev(jac, d_t, dd, n), kinematics.kinematics_rows(jac, d_t, dd, n)
    assert torch.equal(got["valid"], valid) and torch.equal(want["valid"], valid)
    for k in ROW_KEYS:
        assert bool(torch.isfinite(got[k].double()).all()), k
        assert close(got[k], want[k]), k
        assert not bool(got[k][~valid].double().abs().sum()), k          # zeros in every output of a row that is not valid
    assert float(got["speed"][64]) > 0 and not bool(got["velocity"][-1].abs().sum()) and not bool(got["L"][-1].abs().sum())
    # without normals the two rows with a bad normal are valid again
    bare = rows_dev(jac, d_t, dd, None)
    assert torch.equal(bare["valid"][64:], torch.tensor([True, False, False, False, False, False, False, True, True, True]))


@pytest.fixture(scope="module")
def R():
    return renderer_for(11, "trained", True)


def test_point_kinematics_end_to_end_on_the_oracles_tracks(R):
    """500 rows tracked in fp64 on the host, the positions rounded to fp32 and handed with their times to ``renderer.point_kinematics``
    and to the fp64 twin over the fp64 reference at the same fp32 points.  On the rows that keep 1e-5 from every kink of the
    deformation network (at least 300 of them; a row nearer may take the other branch in fp32, which says nothing about the kernels)
    every output agrees within 4 x the worst-row error of the oracle's own fp32 run on the same rows."""
    state = weightgen.make_state(11, "trained", True)
    net64, net32 = oracle_net(state, torch.float64), oracle_net(state, torch.float32)
    x, t_from, t_to = draw(11, 500)
    assert_contraction(net64, x, t_from, t_to)
    ref = tracking.warp_points(deform_fn(net64), x.double(), t_from.double(), t_to.double(), max_iters=300, tol=1e-13)
    assert bool(ref["converged"].all())
    y = ref["points"].float()
    n = torch.from_numpy(np.random.default_rng(2).normal(size=(500, 3))).float()
    want = kinematics.point_kinematics(derivs_fn(net64), y.double(), t_to.double(), n.double())
    o32 = kinematics.point_kinematics(derivs_fn(net32), y, t_to, n)
    got = R.point_kinematics(y, t_to, n)
    assert all(got[k].is_cuda for k in ROW_KEYS) and got["L"].shape == (500, 3, 3) and got["principal_rates"].shape == (500, 3)
    keep = deform_margin(net64, y.double(), t_to.double()) >= 1e-5
    print(f"\nkept {int(keep.sum())} of 500 rows")
    assert int(keep.sum()) >= 300
    assert bool(want["valid"].all()) and bool(got["valid"].all())
    for k in ROW_KEYS[:-1]:
        yard = float((o32[k].double() - want[k])[keep].abs().max())
        err = float((got[k].cpu().double() - want[k])[keep].abs().max())
        print(f"{k}: device {err:.3e}, fp32 oracle {yard:.3e} (bound {MARGIN * yard:.3e})")
        assert err <= MARGIN * yard, (k, err, yard)
    # the C ABI's bits through the renderer's weights and call
    d = R.deform_derivatives(y, t_to)
    assert set(d) == {"jac", "d_t", "dd"} and torch.equal(d["jac"], R.deform_jacobian(y, t_to))
    bare = R.point_kinematics(y.numpy(), t_to.tolist())
    assert set(bare) == set(BARE_KEYS) and all(torch.equal(bare[k], got[k]) for k in bare)


def test_mesh_kinematics_is_the_composition_of_its_two_launches(R):
    verts, tris = _patch()
    times = [0.3, 0.31, 0.9]
    track = R.track_mesh(verts.cuda(), tris.cuda(), t=0.3, times=times)
    assert bool(track["converged"].all())
    out = R.mesh_kinematics(track, times)
    shapes = {"velocity": (3, 289, 3), "speed": (3, 289), "L": (3, 289, 3, 3), "rate": (3, 289, 3, 3), "principal_rates": (3, 289, 3),
              "divergence": (3, 289), "vorticity": (3, 289, 3), "area_rate": (3, 289), "surface_rates": (3, 289, 2), "valid": (3, 289)}
    assert {k: tuple(v.shape) for k, v in out.items()} == shapes and all(v.is_cuda for v in out.values())
    assert bool(out["valid"].all())
    # the composition, spelled out: one derivative launch with a time per row, the normals of each frame, one launch of the algebra
    eng = R.engine
    weff, packed = R._weights()
    tt = torch.tensor(times, device="cuda").repeat_interleave(289)
    d = eng.deform_derivatives(eng.points(x=track["vertices"].reshape(-1, 3).contiguous(), t=tt), weff.detach(), packed)
    normals = torch.stack([eng.vertex_normals(track["vertices"][f].contiguous(), tris.cuda()) for f in range(3)])
    rows = eng.kinematics_rows(d["jac"], d["d_t"], d["dd"], normals.reshape(-1, 3))
    for k in ROW_KEYS:
        assert torch.equal(out[k].reshape(rows[k].shape), rows[k]), k
    print(f"\nspeed {float(out['speed'].min()):.4f} .. {float(out['speed'].max()):.4f}, area rate {float(out['area_rate'].min()):.4f} .. "
          f"{float(out['area_rate'].max()):.4f}, divergence {float(out['divergence'].min()):.4f} .. {float(out['divergence'].max()):.4f}")
    assert float(out["speed"].max()) > 1e-3          # (the tissue does move)
    # against the twin over the same derivatives: the default normals are the twin's, bit for bit (meshing.vertex_normals)
    host = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in track.items()}
    twin = kinematics.mesh_kinematics(lambda p, t: {k: v.cpu() for k, v in R.deform_derivatives(p, t).items()}, host, torch.tensor(times))
    assert all(close(out[k].cpu(), twin[k]) for k in ROW_KEYS)
    # host tensors, numpy arrays and lists give the device tensors' result
    as_np = {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in host.items()}
    as_list = {k: (v.tolist() if torch.is_tensor(v) else v) for k, v in host.items()}
    for tr, tm in ((host, torch.tensor(times)), (as_np, np.asarray(times, np.float32)), (as_list, times)):
        o = R.mesh_kinematics(tr, tm)
        assert all(torch.equal(o[k], out[k]) for k in ROW_KEYS)
    given = R.mesh_kinematics(track, times, normals=normals.cpu().numpy())
    assert all(torch.equal(given[k], out[k]) for k in ROW_KEYS)
    one = R.point_kinematics(track["vertices"][2], 0.9, normals[2])
    assert all(torch.equal(one[k], out[k][2]) for k in ROW_KEYS)


def test_without_a_deformation_network(monkeypatch):
    r = renderer_for(11, "trained", False)

    def refuse(*a, **k):
        raise AssertionError("the derivative kernel was launched")
    monkeypatch.setattr(r.engine, "deform_derivatives", refuse)
    verts, tris = _patch(5)
    d = r.deform_derivatives(verts, 0.4)
    assert d["jac"].is_cuda and torch.equal(d["jac"], torch.eye(3, device="cuda")[None].expand(25, 3, 3))
    assert d["d_t"].shape == (25, 3) and d["dd"].shape == (25, 3, 3) and not bool(d["d_t"].abs().sum()) and not bool(d["dd"].abs().sum())
    track = r.track_mesh(verts, tris, t=0.3, times=[0.3, 0.9])
    out = r.mesh_kinematics(track, [0.3, 0.9])
    assert bool(out["valid"].all()) and out["L"].shape == (2, 25, 3, 3)
    for k in ROW_KEYS[:-1]:
        assert not bool(out[k].abs().sum()), k
    pk = r.point_kinematics(verts, 0.4)
    assert bool(pk["valid"].all()) and not bool(pk["velocity"].abs().sum()) and not bool(pk["L"].abs().sum())


def test_engine_methods(case):
    from endosurf_amd import engine
    eng = engine.Engine(torch.device("cuda", torch.cuda.current_device()))
    dev, xd, td, full = case["dev"], case["x"].cuda(), case["t"].cuda(), case["got"]
    d = eng.deform_derivatives(eng.points(x=xd, t=td), dev.weff, dev.packed, want_xc=True)
    only = eng.deform_derivatives(eng.points(x=xd, t=td), dev.weff, dev.packed)
    assert set(d) == set(OUTS) and set(only) == {"jac", "d_t", "dd"}
    assert all(torch.equal(d[k].cpu(), full[k]) for k in OUTS) and all(torch.equal(only[k], d[k]) for k in only)
    rows = eng.kinematics_rows(d["jac"], d["d_t"], d["dd"])
    assert set(rows) == set(BARE_KEYS) and rows["valid"].dtype == torch.bool and rows["L"].shape == (M, 3, 3)
    assert all(close(rows[k].cpu(), v) for k, v in kinematics.kinematics_rows(full["jac"], full["d_t"], full["dd"]).items())
    J, dt, dd = d["jac"], d["d_t"], d["dd"]
    for bad in (lambda: eng.kinematics_rows(J.cpu(), dt, dd), lambda: eng.kinematics_rows(J, dt[:5], dd), lambda: eng.kinematics_rows(J, dt, dd[:, 0]),
                lambda: eng.kinematics_rows(J, dt, dd, xd[:5]), lambda: eng.kinematics_rows(J.reshape(M, 9), dt, dd)):
        with pytest.raises(ValueError):
            bad()


def test_refusals():
    """Status 1 with a message before anything is launched (the addresses are host numpy's and never dereferenced); M = 0 is status 0."""
    from endosurf_amd import _lib
    lib = _lib.load()
    buf = np.zeros(64, np.float32)
    b = buf.ctypes.data

    def pts(M=4, mode=0):
        p = _lib.es_points()
        p.M, p.mode, p.t_scalar, p.n_per_ray, p.ldz = M, mode, 1, 1, 1
        p.x, p.t, p.rays, p.z = b, b, b, b
        return p
    der = lambda p, packed=b, weff=b, j=b, dt=b, dd=b, xc=b: lib.es_deform_derivatives(C.byref(p), packed, weff, j, dt, dd, xc, None)
    assert der(pts(mode=1)) == 1 and b"mode 0" in lib.es_last_error()
    assert der(pts(mode=2)) == 1 and b"mode 0" in lib.es_last_error()
    assert der(pts(M=-1)) == 1 and b"negative" in lib.es_last_error()
    assert der(pts(), packed=None) == 1 and b"null buffer" in lib.es_last_error()
    assert der(pts(), weff=None) == 1 and b"null buffer" in lib.es_last_error()
    assert der(pts(), j=None, dt=None, dd=None, xc=None) == 1 and b"every output" in lib.es_last_error()
    nox = pts()
    nox.x = None
    assert der(nox) == 1 and b"x and t" in lib.es_last_error()
    assert lib.es_deform_derivatives(None, b, b, b, b, b, b, None) == 1 and b"null" in lib.es_last_error()
    assert lib.es_deform_derivatives(C.byref(_lib.es_points()), None, None, None, None, None, None, None) == 0
    outs = ("v", "sp", "L", "rate", "pr", "div", "vort", "area", "surf", "valid")

    def rows(jac=b, d_t=b, dd=b, n=b, M=4, **null):
        return lib.es_kinematics_rows(jac, d_t, dd, n, M, *(None if null.get(k, 1) is None else b for k in outs), None)
    assert rows(jac=None) == 1 and b"null buffer" in lib.es_last_error()
    assert rows(d_t=None) == 1 and b"null buffer" in lib.es_last_error()
    assert rows(dd=None) == 1 and b"null buffer" in lib.es_last_error()
    assert rows(**{k: None for k in outs}) == 1 and b"every output" in lib.es_last_error()
    assert rows(n=None, surf=None) == 1 and b"normals" in lib.es_last_error()          # area_rate without normals
    assert rows(n=None, area=None) == 1 and b"normals" in lib.es_last_error()          # surface_rates without normals
    assert rows(M=-1) == 1 and b"negative" in lib.es_last_error()
    assert rows(jac=None, d_t=None, dd=None, n=None, M=0, **{k: None for k in outs}) == 0
