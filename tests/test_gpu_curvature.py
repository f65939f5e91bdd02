"""GPU: surface curvature.  Kernel level through the C ABI -- es_sdf_hessian (csrc/sdf_hess.hip) against autograd through
the fp64 oracle and against es_query_sdf_tiles bit for bit, es_curvature_rows (csrc/curvature.hip) against the fp64 numpy twin
``curvature.compose_hessian`` / ``curvature_rows`` -- then Engine and renderer.  Every test prints the figures it asserts on; the
oracle comparisons go to curvature_shapes.json in the log directory of test_gpu_backward.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import weightgen
from curvature_ref import hessian_canonical, hessian_observed
from gpu_util import renderer_for
from point_adjoint_ref import cast_net, reordered, row_error, through_go_only
from shapes_util import FORWARD_GATE
from test_gpu_backward import LOG
from test_gpu_strain import CASES, Dev, screened
from track_util import draw, oracle_net

from endosurf_amd import curvature

pytestmark = pytest.mark.gpu

M = 200
HALF_MAX_POINTS = 1024          # the 32-row tile (2 points) up to here, the 64-row tile (6 points) above (csrc/sdf_hess.hip)
MARGIN = 4.0                    # one more draw of fp32 rounding in another summation order (test_gpu_point_adjoint_shapes.py)
RTOL, ATOL = 2.4e-7, 1e-13      # two fp32 ulps: the kernel's fp64 error is far below half an ulp, only the final rounding can differ
ROW_KEYS = ("gradient", "hessian", "mean", "gauss", "principal", "valid")
_REPORT = {}


def _note(case, **values):
    _REPORT.setdefault(case, {}).update(values)
    os.makedirs(LOG, exist_ok=True)
    with open(os.path.join(LOG, "curvature_shapes.json"), "w") as f:
        json.dump(_REPORT, f, indent=1, sort_keys=True)


def _points(_lib, xd, mode=0):
    p = _lib.es_points()
    p.x, p.mode, p.n_per_ray, p.ldz, p.M = _lib.ptr(xd), mode, 1, 1, xd.shape[0]
    return p


def hessian_dev(dev, xc, tile_rows=0, want=(True, True, True)):
    """es_sdf_hessian at fp32 host points: (sdf [M], gradient [M,3], hessian [M,3,3]) as host tensors, None where not asked for.
    Unwritten entries would stay NaN."""
    _lib, n = dev._lib, xc.shape[0]
    xd = xc.cuda().contiguous()
    bufs = [torch.full(s, float("nan"), device="cuda") if w else None for s, w in zip(((n,), (n, 3), (n, 3, 3)), want)]
    _lib.check(dev.lib.es_sdf_hessian(C.byref(_points(_lib, xd)), _lib.ptr(dev.packed), _lib.ptr(dev.weff), tile_rows, *(_lib.ptr(b) for b in bufs),
                                      _lib.stream_ptr()), "es_sdf_hessian")
    torch.cuda.synchronize()
    return tuple(None if b is None else b.cpu() for b in bufs)


def query_dev(dev, xc, tile_points):
    """es_query_sdf_tiles without deformation at the same points."""
    _lib, n = dev._lib, xc.shape[0]
    xd, td = xc.cuda().contiguous(), torch.zeros(n, device="cuda")
    p = _points(_lib, xd)
    p.t = _lib.ptr(td)
    out = torch.full((n,), float("nan"), device="cuda")
    _lib.check(dev.lib.es_query_sdf_tiles(C.byref(p), _lib.ptr(dev.packed), _lib.ptr(dev.weff), _lib.ptr(out), 0, tile_points, _lib.stream_ptr()),
               "es_query_sdf_tiles")
    torch.cuda.synchronize()
    return out.cpu()


def rows_dev(grad_c, hess_c, jac=None, dd=None):
    """es_curvature_rows on fp32 host rows: dict of host tensors (NaN / True where the kernel did not write)."""
    from endosurf_amd import _lib
    lib, ptr = _lib.load(), _lib.ptr
    n = grad_c.shape[0]
    dev = lambda a: None if a is None else a.float().cuda().contiguous()
    g, H, J, d = dev(grad_c), dev(hess_c), dev(jac), dev(dd)
    out = {k: torch.full(s, float("nan"), device="cuda") for k, s in dict(gradient=(n, 3), hessian=(n, 3, 3), mean=(n,), gauss=(n,), principal=(n, 2)).items()}
    out["valid"] = torch.ones(n, dtype=torch.bool, device="cuda")
    _lib.check(lib.es_curvature_rows(ptr(g), ptr(H), ptr(J), ptr(d), n, ptr(out["gradient"]), ptr(out["hessian"]), ptr(out["mean"]), ptr(out["gauss"]),
                                     ptr(out["principal"]), ptr(out["valid"]), _lib.stream_ptr()), "es_curvature_rows")
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def rows_twin(grad_c, hess_c, jac=None, dd=None):
    """The twin on the same fp32 values, in fp64 throughout."""
    f = lambda a: None if a is None else a.double()
    go, Ho = curvature.compose_hessian(f(grad_c), f(hess_c), f(jac), f(dd))
    return {"gradient": go, "hessian": Ho, **curvature.curvature_rows(go, Ho)}


def close(got, want):
    if got.dtype == torch.bool:
        return torch.equal(got, want)
    g, w = got.double(), want.double()
    same = (g - w).abs() <= ATOL + RTOL * w.abs()
    return bool((same | (torch.isnan(g) & torch.isnan(w)) | (torch.isinf(w) & (g == w))).all())


def yardstick(fn, net64, ref64):
    """The worse of the fp32 oracle's and its reordered twin's worst row_error against ``ref64``: ``fn(net, dtype)`` -> tensor."""
    return max(float(row_error(fn(net, torch.float32).double().numpy(), ref64).max()) for net in (net64, reordered(net64, 1)))


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"{c[1]}{c[0]}")
def case(request):
    """One state: device weights, the fp64 oracle, 200 screened rows, the canonical points x + D rounded to fp32, the fp64 references
    there and the device's own results (computed once, shared, never written to)."""
    seed, mode = request.param
    state = weightgen.make_state(seed, mode, True)
    dev, net64 = Dev(state), oracle_net(state, torch.float64)
    x, t = screened(net64, M, seed)
    with torch.no_grad():
        xc = (x.double() + net64.deform(x.double(), t.double(), with_jac=False)[0]).float()
    sdf64, g64, H64 = hessian_canonical(net64, xc)
    sdf, g, H = hessian_dev(dev, xc)
    return dict(seed=seed, mode=mode, name=f"{mode}{seed}", dev=dev, net64=net64, x=x, t=t, xc=xc, sdf64=sdf64, g64=g64, H64=H64, sdf=sdf, g=g, H=H)


def test_sdf_hessian_against_the_fp64_oracle(case):
    """The value is es_query_sdf_tiles' without deformation bit for bit (32- and 64-point tiles); the gradient within FORWARD_GATE["gc"]
    of the fp64 oracle; the Hessian's row_error at most 4 x the worse of the fp32 oracle's and its reordered twin's own on the same
    rows; the Hessian exactly symmetric."""
    dev, xc, net64 = case["dev"], case["xc"], case["net64"]
    for tile in (32, 64):
        assert torch.equal(case["sdf"], query_dev(dev, xc, tile)), tile
    e_g = float((case["g"].double() - case["g64"]).abs().max())
    H64 = case["H64"].numpy()
    err = float(row_error(case["H"].double().numpy(), H64).max())
    yard = yardstick(lambda net, dtype: hessian_canonical(net, xc, dtype)[2], net64, H64)
    print(f"\n[{case['name']}] gradient {e_g:.3e} (gate {FORWARD_GATE['gc']:.1e})  Hessian row error {err:.3e}, fp32 oracle {yard:.3e} "
          f"(bound {MARGIN * yard:.3e}), max |H| {np.abs(H64).max():.1f}")
    _note(f"canonical_{case['name']}", gradient=e_g, hessian=[err, yard], max_abs_hessian=float(np.abs(H64).max()))
    assert bool(torch.isfinite(case["H"]).all())
    assert e_g <= FORWARD_GATE["gc"]
    assert err <= MARGIN * yard, (err, yard)
    assert torch.equal(case["H"], case["H"].transpose(1, 2))
    # either output alone is the same as in the triple
    assert torch.equal(hessian_dev(dev, xc, want=(False, False, True))[2], case["H"])
    assert torch.equal(hessian_dev(dev, xc, want=(False, True, False))[1], case["g"])
    assert torch.equal(hessian_dev(dev, xc, want=(True, False, False))[0], case["sdf"])


def test_rows_do_not_depend_on_their_place_or_neighbours(case):
    """The same bits on prefixes around the edges of the 2- and 6-point tiles, on the first batch that selects the 64-row tile (the 200
    rows repeated to 1 025) and on that batch + 5, permuted, alone, and on both tile heights asked for by name."""
    dev, xc, full = case["dev"], case["xc"], (case["sdf"], case["g"], case["H"])
    for tile_rows in (0, 64):
        for m in (1, 2, 3, 5, 6, 7, 12, 13):
            for a, b in zip(full, hessian_dev(dev, xc[:m], tile_rows)):
                assert torch.equal(a[:m], b), (tile_rows, m)
    for n in (HALF_MAX_POINTS, HALF_MAX_POINTS + 1, HALF_MAX_POINTS + 6):
        idx = torch.arange(n) % M
        for a, b in zip(full, hessian_dev(dev, xc[idx])):
            assert torch.equal(a[idx], b), n
    perm = torch.from_numpy(np.random.default_rng(3).permutation(M).copy())
    for a, again, shuffled, alone, t32, t64 in zip(full, hessian_dev(dev, xc), hessian_dev(dev, xc[perm]), hessian_dev(dev, xc[117:118]),
                                                   hessian_dev(dev, xc, 32), hessian_dev(dev, xc, 64)):
        assert torch.equal(a, again) and torch.equal(a[perm], shuffled) and torch.equal(a[117:118], alone)
        assert torch.equal(a, t32) and torch.equal(a, t64)


def test_an_empty_batch_launches_nothing_and_refusals():
    """M = 0: status 0 and nothing written (the buffers keep their NaN).  Status 1 with a message before anything is launched (the
    addresses are host numpy's and never dereferenced): a mode other than 0, a null input, no output, tile_rows."""
    from endosurf_amd import _lib
    lib = _lib.load()
    bufs = [torch.full((8,), float("nan"), device="cuda") for _ in range(3)]
    p = _lib.es_points()
    p.x = _lib.ptr(bufs[0])
    assert lib.es_sdf_hessian(C.byref(p), None, None, 0, *(_lib.ptr(b) for b in bufs), None) == 0
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(b).all()) for b in bufs)
    assert lib.es_sdf_hessian(C.byref(_lib.es_points()), None, None, 0, None, None, None, None) == 0
    b = np.zeros(64, np.float32).ctypes.data

    def pts(mode=0, x=b):
        q = _lib.es_points()
        q.M, q.mode, q.n_per_ray, q.ldz, q.x, q.rays, q.z = 4, mode, 1, 1, x, b, b
        return q
    hess = lambda q, packed=b, weff=b, tile=0, s=b, g=b, h=b: lib.es_sdf_hessian(C.byref(q), packed, weff, tile, s, g, h, None)
    assert hess(pts(mode=1)) == 1 and b"mode 0" in lib.es_last_error()
    assert hess(pts(mode=2)) == 1 and b"mode 0" in lib.es_last_error()
    assert hess(pts(x=None)) == 1 and b"null buffer" in lib.es_last_error()
    assert hess(pts(), packed=None) == 1 and b"null buffer" in lib.es_last_error()
    assert hess(pts(), weff=None) == 1 and b"null buffer" in lib.es_last_error()
    assert hess(pts(), s=None, g=None, h=None) == 1 and b"every output" in lib.es_last_error()
    assert hess(pts(), tile=16) == 1 and b"tile_rows" in lib.es_last_error()
    rows = lambda g=b, H=b, J=b, d=b, n=4, go=b, Ho=b, m=b, ga=b, pr=b, v=b: lib.es_curvature_rows(g, H, J, d, n, go, Ho, m, ga, pr, v, None)
    assert rows(g=None) == 1 and b"null buffer" in lib.es_last_error()
    assert rows(H=None) == 1 and b"null buffer" in lib.es_last_error()
    assert rows(go=None, Ho=None, m=None, ga=None, pr=None, v=None) == 1 and b"every output" in lib.es_last_error()
    assert rows(n=-1) == 1 and b"negative" in lib.es_last_error()
    assert rows(g=None, H=None, J=None, d=None, n=0, go=None, Ho=None, m=None, ga=None, pr=None, v=None) == 0


@pytest.fixture(scope="module")
def R():
    return renderer_for(11, "trained", True)


@pytest.fixture(scope="module")
def own_rows(R):
    """The device's own rows on the seed-11 weights at 257 points of ``track_util.draw``: g_c, H_c at x + D, J and the forward's
    ES_WS_CURV, copied to the host."""
    from endosurf_amd import _lib
    x, t, _ = draw(11, 257)
    eng = R.engine
    with torch.no_grad():
        weff, packed = R._weights()
        weff = weff.detach()
        jac, xc = eng.deform_jacobian(eng.points(x=x.cuda(), t=t.cuda()), weff, packed, want_xc=True)
        _, g, H = eng.sdf_hessian(xc, weff, packed)
        dd = eng.point_forward(eng.points(x=x.cuda(), t=t.cuda()), weff, packed, _lib.PF_DEFORM, fp32_only=True).view("curv").clone()
    torch.cuda.synchronize()
    return g.cpu(), H.cpu(), jac.cpu(), dd.cpu()


@pytest.mark.parametrize("m", [0, 1, 63, 64, 65, 257])
def test_curvature_rows_against_the_numpy_twin(own_rows, m):
    g, H, J, dd = (a[:m] for a in own_rows)
    got, want = rows_dev(g, H, J, dd), rows_twin(g, H, J, dd)
    assert set(got) == set(want) == set(ROW_KEYS)
    for k in ROW_KEYS:
        assert got[k].shape == want[k].shape and close(got[k], want[k]), (k, m)
    assert bool(want["valid"].all())
    if m:
        worst = max(float(((got[k].double() - want[k]).abs() / want[k].abs().clamp_min(1e-30)).max()) for k in ("mean", "gauss", "principal", "hessian"))
        print(f"\nM {m}: largest relative difference to the twin {worst:.3e} (two ulps: {RTOL:.1e}); principal curvatures "
              f"{float(want['principal'].min()):.2f} .. {float(want['principal'].max()):.2f}")
    again = rows_dev(g, H, J, dd)
    assert all(torch.equal(got[k], again[k]) for k in ROW_KEYS)          # bit-identical from call to call
    # jac null is the identity, dd null is zero; then gradient and Hessian pass through unchanged
    eye = torch.eye(3)[None].expand(m, 3, 3).contiguous()
    bare, given = rows_dev(g, H), rows_dev(g, H, eye, torch.zeros(m, 3))
    assert all(torch.equal(bare[k], given[k]) for k in ROW_KEYS)
    assert torch.equal(bare["gradient"], g) and torch.equal(bare["hessian"], H)
    assert all(close(bare[k], v) for k, v in rows_twin(g, H).items())


def hand_rows():
    """(grad_c, hess_c, jac, dd, valid) fp32: a sphere as a distance and as |x|^2 - R^2, a cylinder, a paraboloid at the origin, the
    sphere under a rotation and under a scaling J, a zero gradient, a NaN on each input."""
    eye = np.eye(3)
    p = np.array([0.3, -0.5, 0.8]); R = float(np.linalg.norm(p)); n = p / R
    sphere = (n, (eye - np.outer(n, n)) / R)
    c = np.array([0.6, 0.8, 0.0])
    q, _ = np.linalg.qr(np.random.default_rng(6).normal(size=(3, 3)))
    nan3, nan33 = np.array([0.0, np.nan, 0.0]), eye.copy()
    nan33[1, 2] = np.nan
    zero = np.zeros(3)
    rows = [(*sphere, eye, zero, True), (2 * p, 2 * eye, eye, zero, True),
            (c, (eye - np.outer(c, c) - np.diag([0.0, 0.0, 1.0])) / 0.5, eye, zero, True),
            (np.array([0.0, 0.0, 1.0]), -np.diag([1.5, 0.5, 0.0]), eye, zero, True),
            (*sphere, q, zero, True), (*sphere, 2.0 * eye, zero, True), (*sphere, eye, np.array([0.1, -0.2, 0.3]), True),
            (zero, sphere[1], eye, zero, False), (nan3, sphere[1], eye, zero, False), (n, nan33, eye, zero, False),
            (n, sphere[1], nan33, zero, False), (n, sphere[1], eye, nan3, False)]
    g, H, J, d, v = zip(*rows)
    f = lambda a: torch.from_numpy(np.asarray(a, np.float64)).float()
    return f(g), f(H), f(J), f(d), torch.tensor(v), R


def test_curvature_rows_on_hand_made_rows(own_rows):
    g, H, J, d, valid, R = hand_rows()
    # behind 64 ordinary rows, so that the block holds both kinds
    g, H, J, d = (torch.cat([a[:64], b]) for a, b in zip(own_rows, (g, H, J, d)))
    valid = torch.cat([torch.ones(64, dtype=torch.bool), valid])
    got, want = rows_dev(g, H, J, d), rows_twin(g, H, J, d)
    assert torch.equal(got["valid"], valid) and torch.equal(want["valid"], valid)
    for k in ROW_KEYS:
        assert close(got[k], want[k]), k
    for k in ("mean", "gauss", "principal"):
        assert bool(torch.isfinite(got[k]).all()) and not bool(got[k][~valid].abs().sum()), k          # zeros in a row that is not valid
    h = {k: v[64:] for k, v in got.items()}
    tol = 4e-7          # the fp32 entries of n and H carry half an ulp each
    for row, k in ((0, 1 / R), (1, 1 / R), (4, 1 / R), (5, 2 / R)):          # the sphere, squared, rotated, scaled by 2 (radius R / 2)
        assert float((h["principal"][row] - k).abs().max()) <= tol * k and abs(float(h["mean"][row]) - k) <= tol * k, row
        assert abs(float(h["gauss"][row]) - k * k) <= 2 * tol * k * k, row
    assert abs(float(h["principal"][2][0]) - 2.0) <= 2 * tol and abs(float(h["principal"][2][1])) <= 2 * tol          # the cylinder, R = 0.5
    assert h["principal"][3].tolist() == [-0.5, -1.5] and float(h["mean"][3]) == -1.0 and float(h["gauss"][3]) == 0.75          # the paraboloid
    assert torch.equal(h["hessian"][6], H[64 + 6] - torch.diag(d[64 + 6]))          # - diag(dd)


def test_observed_space_against_the_fp64_oracle(case):
    """``renderer.sdf_hessian(x, t)`` against autograd through ``sdf_observed`` in fp64 on the screened rows, which keep RELU_MARGIN from
    every kink: value and gradient within FORWARD_GATE, the Hessian's row_error at most 4 x the worse of the fp32 oracle's and its
    reordered twin's own."""
    r = renderer_for(case["seed"], case["mode"], True)
    x, t, net64 = case["x"], case["t"], case["net64"]
    sdf64, g64, H64 = hessian_observed(net64, x, t)
    out = r.sdf_hessian(x, t)
    assert all(v.is_cuda for v in out.values()) and {k: tuple(v.shape) for k, v in out.items()} == {"sdf": (M, 1), "gradient": (M, 3), "hessian": (M, 3, 3)}
    e_s, e_g = float((out["sdf"].cpu().double() - sdf64).abs().max()), float((out["gradient"].cpu().double() - g64).abs().max())
    err = float(row_error(out["hessian"].cpu().double().numpy(), H64.numpy()).max())
    yard = yardstick(lambda net, dtype: hessian_observed(net, x, t, dtype)[2], net64, H64.numpy())
    print(f"\n[{case['name']}] observed: sdf {e_s:.3e}  gradient {e_g:.3e}  Hessian row error {err:.3e}, fp32 oracle {yard:.3e} "
          f"(bound {MARGIN * yard:.3e}), max |H_o| {float(H64.abs().max()):.1f}")
    _note(f"observed_{case['name']}", sdf=e_s, gradient=e_g, hessian=[err, yard], max_abs_hessian=float(H64.abs().max()))
    assert e_s <= FORWARD_GATE["sdf"] and e_g <= FORWARD_GATE["go"]
    assert err <= MARGIN * yard, (err, yard)
    # the canonical space is the kernel alone: the C ABI's bits
    can = r.sdf_hessian(case["xc"], space="canonical")
    assert torch.equal(can["sdf"].cpu()[:, 0], case["sdf"]) and torch.equal(can["gradient"].cpu(), case["g"]) and torch.equal(can["hessian"].cpu(), case["H"])
    # a shared time is read as one value
    shared = r.sdf_hessian(x[:9], float(t[0]))
    assert torch.equal(shared["hessian"][:1], out["hessian"][:1]) and not torch.equal(shared["hessian"][1:], out["hessian"][1:9])


def test_hessian_vector_products_against_the_point_adjoint(case):
    """On 64 rows and three directions w: H_o w from ``renderer.sdf_hessian`` against ``Engine.point_input_adjoint`` behind a saving
    forward and a full backward with d_go = w.  Both are held to the fp64 oracle's grad_x <g_o, w> under 4 x their own fp32 yardstick
    (the Hessian's for one route, the Hessian-vector product's for the other), and to each other under the sum of the two gates."""
    from endosurf_amd import _lib
    r = renderer_for(case["seed"], case["mode"], True)
    eng, net64 = r.engine, case["net64"]
    x, t = case["x"][:64], case["t"][:64]
    with torch.no_grad():
        weff, packed = r._weights()
    weff = weff.detach()
    H = r.sdf_hessian(x, t)["hessian"].cpu().double()
    for k in range(3):
        w = torch.from_numpy(np.random.default_rng(70 + k).normal(size=(64, 3)).astype(np.float32))
        ref64 = through_go_only(net64, x, t, w).numpy()
        ours = torch.einsum("mjk,mk->mj", H, w.double()).numpy()
        ctx = eng.point_forward(eng.points(x=x.cuda(), t=t.cuda()), weff, packed, _lib.PF_DEFORM | _lib.PF_SAVE, fp32_only=True)
        eng.point_backward(ctx, weff, packed, None, w.cuda())
        theirs = eng.point_input_adjoint(ctx, weff, packed, None, w.cuda()).cpu().double().numpy()
        gate_a = MARGIN * yardstick(lambda net, dtype: torch.einsum("mjk,mk->mj", hessian_observed(net, x, t, dtype)[2], w.to(dtype)), net64, ref64)
        gate_b = MARGIN * yardstick(lambda net, dtype: through_go_only(net, x, t, w, dtype=dtype), net64, ref64)
        e_a, e_b = float(row_error(ours, ref64).max()), float(row_error(theirs, ref64).max())
        apart = float(row_error(ref64 + (ours - theirs), ref64).max())
        print(f"\n[{case['name']}] direction {k}: one launch {e_a:.3e} (gate {gate_a:.3e}), point adjoint {e_b:.3e} (gate {gate_b:.3e}), "
              f"apart {apart:.3e}")
        _note(f"hvp_{case['name']}_{k}", hessian_route=[e_a, gate_a], adjoint_route=[e_b, gate_b], apart=apart)
        assert e_a <= gate_a and e_b <= gate_b and apart <= gate_a + gate_b


def test_surface_and_mesh_curvature_are_the_composition(R):
    """``surface_curvature`` is ``sdf_hessian`` followed by one ``es_curvature_rows`` launch; ``mesh_curvature`` on a tracked 24^3-lattice
    mesh is that composition on all F * V rows, bit for bit; rows of unconverged track entries are not valid and zero."""
    mesh = R.extract_observation_mesh(0.3, [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0], 24)
    times = [0.3, 0.31, 0.9]
    track = R.track_mesh(mesh, t=0.3, times=times)
    F, V = 3, int(mesh["vertices"].shape[0])
    conv = track["converged"].clone()
    conv[1, 5] = False
    conv[2, V - 1] = False
    track = {**track, "converged": conv}
    out = R.mesh_curvature(track, times=times)
    assert {k: tuple(v.shape) for k, v in out.items()} == {"mean": (F, V), "gauss": (F, V), "principal": (F, V, 2), "valid": (F, V)}
    assert all(v.is_cuda for v in out.values())
    tt = torch.tensor(times, device="cuda").repeat_interleave(V)
    rows = R.surface_curvature(track["vertices"].reshape(-1, 3), tt)
    h = R.sdf_hessian(track["vertices"].reshape(-1, 3), tt)
    alg = R.engine.curvature_rows(h["gradient"], h["hessian"])
    assert all(torch.equal(rows[k], h[k]) for k in h) and all(torch.equal(rows[k], alg[k]) for k in ("mean", "gauss", "principal", "valid"))
    valid = rows["valid"].reshape(F, V) & conv
    assert torch.equal(out["valid"], valid) and not bool(out["valid"][1, 5]) and not bool(out["valid"][2, V - 1])
    for k in ("mean", "gauss", "principal"):
        want = rows[k].reshape(out[k].shape)
        assert torch.equal(out[k], torch.where(valid.reshape(F, V, *([1] * (want.dim() - 2))), want, torch.zeros_like(want))), k
    assert float(out["mean"][1, 5]) == 0.0 and out["principal"][2, V - 1].tolist() == [0.0, 0.0]
    print(f"\n{V} vertices: mean curvature at t = 0.3 {float(out['mean'][0].min()):.2f} .. {float(out['mean'][0].max()):.2f}, "
          f"valid {int(out['valid'].sum())} of {F * V}")
    assert int(out["valid"].sum()) >= 0.9 * F * V
    # against the twin on the same gradient and Hessian
    twin = curvature.curvature_rows(h["gradient"].cpu().double(), h["hessian"].cpu().double())
    assert all(close(alg[k].cpu(), twin[k]) for k in ("mean", "gauss", "principal", "valid"))
    # a mesh at one time; host tensors, numpy arrays and lists give the device tensors' result
    one, at = R.mesh_curvature(mesh, t=0.3), R.surface_curvature(mesh["vertices"], 0.3)
    assert set(one) == {"mean", "gauss", "principal", "valid"} and one["mean"].shape == (V,) and all(torch.equal(one[k], at[k]) for k in one)
    host = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in track.items()}
    as_np = {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in host.items()}
    for tr, tm in ((host, torch.tensor(times)), (as_np, np.asarray(times, np.float32))):
        o = R.mesh_curvature(tr, times=tm)
        assert all(torch.equal(o[k], out[k]) for k in out)
    with pytest.raises(TypeError):
        R.mesh_curvature(track)
    with pytest.raises(ValueError):
        R.sdf_hessian(mesh["vertices"], 0.3, space="world")


def test_without_a_deformation_network(monkeypatch):
    """J = I and CURV = 0: the observed call is the canonical call bit for bit, and neither the Jacobian kernel, the point forward nor
    the composing launch runs."""
    r = renderer_for(11, "trained", False)

    def refuse(*a, **k):
        raise AssertionError("a launch of the deformation route")
    for name in ("deform_jacobian", "point_forward"):
        monkeypatch.setattr(r.engine, name, refuse)
    x, t, _ = draw(11, 77)
    obs, can = r.sdf_hessian(x, t), r.sdf_hessian(x, space="canonical")
    assert all(torch.equal(obs[k], can[k]) for k in can) and bool(torch.isfinite(obs["hessian"]).all())
    sc = r.surface_curvature(x, t)
    assert set(sc) == {"sdf", "gradient", "hessian", "mean", "gauss", "principal", "valid"} and torch.equal(sc["hessian"], can["hessian"])
    empty = r.surface_curvature(x[:0], 0.1)
    assert empty["hessian"].shape == (0, 3, 3) and empty["mean"].shape == (0,) and empty["valid"].shape == (0,)


def test_engine_methods(case):
    from endosurf_amd import engine
    eng = engine.Engine(torch.device("cuda", torch.cuda.current_device()))
    dev, xd = case["dev"], case["xc"].cuda()
    sdf, g, H = eng.sdf_hessian(xd, dev.weff, dev.packed)
    assert torch.equal(sdf.cpu(), case["sdf"]) and torch.equal(g.cpu(), case["g"]) and torch.equal(H.cpu(), case["H"])
    assert torch.equal(eng.sdf_hessian(xd, dev.weff, dev.packed, tile_rows=64)[2], H)
    rows = eng.curvature_rows(g, H)
    assert set(rows) == set(ROW_KEYS) and rows["valid"].dtype == torch.bool and rows["principal"].shape == (M, 2)
    assert all(close(rows[k].cpu(), v) for k, v in rows_twin(case["g"], case["H"]).items())
    assert set(eng.curvature_rows(g, H, curvature=False)) == {"gradient", "hessian"}
    for bad in (lambda: eng.sdf_hessian(xd.cpu(), dev.weff, dev.packed), lambda: eng.sdf_hessian(xd.reshape(-1), dev.weff, dev.packed),
                lambda: eng.sdf_hessian(xd, dev.weff, dev.packed, tile_rows=16), lambda: eng.curvature_rows(g.cpu(), H),
                lambda: eng.curvature_rows(g, H[:5]), lambda: eng.curvature_rows(g, H, H[:5]), lambda: eng.curvature_rows(g, H, None, g[:5])):
        with pytest.raises(ValueError):
            bad()
