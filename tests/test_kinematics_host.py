"""CPU: ``endosurf_amd.kinematics``, the fp64 twin of the kinematics kernels -- on an affine map with a closed form, and
over the fp64 oracle's derivatives (``kinematics_ref``) against finite differences of what the project already has: ``tracking``'s
warp, the oracle's closed-form Jacobian and ``strain``'s area ratio.  Every test prints the figures it asserts on."""
import numpy as np
import pytest
import torch

import weightgen
from kinematics_ref import derivatives, derivs_fn, jacobian_fn
from track_util import deform_fn, draw, oracle_net

from endosurf_amd import kinematics, strain, tracking

CASES = [(11, "trained"), (23, "trained"), (21, "init")]
M = 200
H = 1e-6              # the step of every central difference here
MAX_KINK_ROWS = 8     # rows whose stencil may cross a ReLU kink of the deformation network


def test_affine_map_has_the_closed_form():
    """D(y, t) = t A y with |A|_2 = 0.4: J = I + t A, D_t = A y, dd = 0, d_xt = A, so v = -J^-1 A y and L = -J^-1 A."""
    rng = np.random.default_rng(5)
    A = rng.normal(size=(3, 3))
    A *= 0.4 / np.linalg.norm(A, 2)
    m = 64
    y, t = rng.uniform(-0.8, 0.8, size=(m, 3)), rng.uniform(0.05, 0.95, size=m)
    n = rng.normal(size=(m, 3))
    J = np.eye(3)[None] + t[:, None, None] * A[None]
    Jinv = np.linalg.inv(J)
    v_want, L_want = -np.einsum("mij,jk,mk->mi", Jinv, A, y), -np.einsum("mij,jk->mik", Jinv, A)
    tt = torch.from_numpy
    args = (tt(J), tt(y @ A.T), torch.zeros(m, 3, 3, dtype=torch.float64), tt(n))
    Am = tt(np.broadcast_to(A, (m, 3, 3)).copy())
    for dd in (args[2], torch.zeros(m, 3, 3, 3, dtype=torch.float64)):          # the diagonal and the full form
        out = kinematics.kinematics_rows(args[0], args[1], dd, args[3], d_xt=Am)
        e_v, e_L = float((out["velocity"].numpy() - v_want).__abs__().max()), float((out["L"].numpy() - L_want).__abs__().max())
        e_p = float((out["principal_rates"].sum(-1) - out["divergence"]).abs().max())
        e_s = float((out["surface_rates"].sum(-1) - out["area_rate"]).abs().max())
        print(f"\naffine: v {e_v:.2e}  L {e_L:.2e}  sum principal - divergence {e_p:.2e}  sum surface - area {e_s:.2e}  (gate 1e-13)")
        assert max(e_v, e_L, e_p, e_s) <= 1e-13
        assert bool(out["valid"].all()) and out["velocity"].dtype == torch.float64
        assert torch.equal(out["rate"], 0.5 * (out["L"] + out["L"].transpose(1, 2)))
        assert float((out["speed"] - out["velocity"].norm(dim=-1)).abs().max()) <= 1e-15
        W = out["L"] - out["L"].transpose(1, 2)
        assert torch.equal(out["vorticity"], torch.stack([W[:, 2, 1], W[:, 0, 2], W[:, 1, 0]], -1))
        assert bool((out["principal_rates"][:, :-1] >= out["principal_rates"][:, 1:]).all())
        assert bool((out["surface_rates"][:, 0] >= out["surface_rates"][:, 1]).all())
    # the full second derivative of a quadratic map D_i = 0.5 y^T Q_i y (independent of t: v = 0 unless D_t is handed in) equals the
    # diagonal form when Q_i is diagonal
    q = rng.normal(size=(m, 3, 3)) * 0.1
    full = np.zeros((m, 3, 3, 3))
    for k in range(3):
        full[:, :, k, k] = q[:, :, k]
    a = kinematics.kinematics_rows(args[0], args[1], tt(q), args[3])
    b = kinematics.kinematics_rows(args[0], args[1], tt(full), args[3])
    assert all(torch.equal(a[k], b[k]) for k in a) and float(a["L"].abs().max()) > 0
    # without normals: the same rows, no surface outputs; fp32 inputs come back as fp32
    bare = kinematics.kinematics_rows(args[0], args[1], tt(q))
    assert set(a) - set(bare) == {"area_rate", "surface_rates"} and all(torch.equal(bare[k], a[k]) for k in bare)
    assert kinematics.kinematics_rows(args[0].float(), args[1].float(), tt(q).float())["L"].dtype == torch.float32


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"{c[1]}{c[0]}")
def case(request):
    """One state: the fp64 oracle, 200 points of ``track_util.draw`` with times mapped to 0.05 + 0.9 t, the reference derivatives there
    and the twin's rows over them (computed once, shared, never written to)."""
    seed, mode = request.param
    net = oracle_net(weightgen.make_state(seed, mode, True), torch.float64)
    x, t, _ = draw(seed, M)
    x, t = x.double(), 0.05 + 0.9 * t.double()
    ref = derivatives(net, x, t, full=True)
    n = torch.from_numpy(np.random.default_rng(40 + seed).normal(size=(M, 3)))
    rows = kinematics.kinematics_rows(ref["jac"], ref["d_t"], ref["dd"], n)
    return dict(name=f"{mode}{seed}", net=net, x=x, t=t, ref=ref, n=n, rows=rows)


def _warp(net, x, t_from, t_to):
    out = tracking.warp_points(deform_fn(net), x, t_from, t_to, max_iters=300, tol=1e-13)
    assert bool(out["converged"].all())
    return out["points"]


def test_the_mixed_second_derivatives_of_the_network_vanish(case):
    ref = case["ref"]
    off = ref["hess"].clone()
    for k in range(3):
        off[:, :, k, k] = 0.0
    print(f"\n[{case['name']}] max |D_i,jk| j != k {float(off.abs().max())}, max |D_i,kt| {float(ref['d_xt'].abs().max())}, "
          f"max |D_i,kk| {float(ref['dd'].abs().max()):.3f}")
    assert float(off.abs().max()) == 0.0 and float(ref["d_xt"].abs().max()) == 0.0
    assert float(ref["dd"].abs().max()) > 0.1
    # the reference's Jacobian is the oracle's closed form
    assert float((ref["jac"] - jacobian_fn(case["net"])(case["x"], case["t"])).abs().max()) <= 1e-13
    assert bool(case["rows"]["valid"].all())


def test_velocity_is_the_time_derivative_of_the_track(case):
    """v against the central difference (h = 1e-6) of ``tracking.warp_points`` from t to t +- h: within 1e-6 on all but at most 8 rows
    (a row whose stencil crosses a ReLU kink differs by the jump of D_t there)."""
    net, x, t = case["net"], case["x"], case["t"]
    fd = (_warp(net, x, t, t + H) - _warp(net, x, t, t - H)) / (2 * H)
    err = (case["rows"]["velocity"] - fd).abs().amax(-1)
    bad = int((err > 1e-6).sum())
    print(f"\n[{case['name']}] v against the difference of the warp: 90th percentile {float(err.quantile(0.9)):.2e}, rows above 1e-6: {bad} "
          f"(at most {MAX_KINK_ROWS}); speed up to {float(case['rows']['speed'].max()):.3f}")
    assert bad <= MAX_KINK_ROWS


def test_velocity_gradient_is_the_derivative_of_the_velocity(case):
    """L against the central difference (h = 1e-6) of v over x: within 1e-5 on all but at most 8 rows."""
    net, x, t = case["net"], case["x"], case["t"]
    fn = derivs_fn(net)
    fd = torch.zeros(M, 3, 3, dtype=torch.float64)
    for k in range(3):
        e = torch.zeros(3, dtype=torch.float64)
        e[k] = H
        vp, vm = (kinematics.point_kinematics(fn, x + s * e, t)["velocity"] for s in (1.0, -1.0))
        fd[:, :, k] = (vp - vm) / (2 * H)
    err = (case["rows"]["L"] - fd).abs().amax((-1, -2))
    bad = int((err > 1e-5).sum())
    print(f"\n[{case['name']}] L against the difference of v: 90th percentile {float(err.quantile(0.9)):.2e}, rows above 1e-5: {bad} "
          f"(at most {MAX_KINK_ROWS}); |L| up to {float(case['rows']['L'].abs().max()):.3f}")
    assert bad <= MAX_KINK_ROWS


def test_divergence_and_area_rate_are_the_rates_of_the_strain(case):
    """Along the track of each point, F(t') = J(y(t'), t')^-1 J(x, t): tr L is d/dt' ln det F at t' = t, and with the normal n at (x, t)
    area_rate is d/dt' ln |cof(F) n| there (at t' = t the current normal is n itself).  Both by central differences (h = 1e-6) of
    ``strain.track_strain`` over the oracle's closed-form Jacobian, within 1e-6 on all but at most 8 rows."""
    net, x, t, n = case["net"], case["x"], case["t"], case["n"]
    ends = [strain.track_strain(jacobian_fn(net), x, t, _warp(net, x, t, t + s * H), t + s * H, n) for s in (1.0, -1.0)]
    for key, mine in (("det", "divergence"), ("area", "area_rate")):
        fd = (ends[0][key].log() - ends[1][key].log()) / (2 * H)
        err = (case["rows"][mine] - fd).abs()
        bad = int((err > 1e-6).sum())
        print(f"\n[{case['name']}] {mine} against the difference of ln {key}: median {float(err.median()):.2e}, rows above 1e-6: {bad} "
              f"(at most {MAX_KINK_ROWS}); up to {float(case['rows'][mine].abs().max()):.3f}")
        assert bad <= MAX_KINK_ROWS
    r = case["rows"]
    assert float((r["principal_rates"].sum(-1) - r["divergence"]).abs().max()) <= 1e-13
    assert float((r["surface_rates"].sum(-1) - r["area_rate"]).abs().max()) <= 1e-13


def hand_rows():
    """(jac, d_t, dd, normals, valid) fp64: an ordinary row, a negative determinant, a NaN and an inf in each input, a zero normal, a
    NaN normal."""
    eye, nan, inf = np.eye(3), float("nan"), float("inf")
    J = eye + 0.1 * np.random.default_rng(8).normal(size=(3, 3))
    dt, dd, n = np.array([0.1, -0.2, 0.05]), 0.3 * np.random.default_rng(9).normal(size=(3, 3)), np.array([0.3, -0.5, 0.8])

    def put(a, idx, val):
        a = a.copy()
        a[idx] = val
        return a
    rows = [(J, dt, dd, n, True), (np.diag([-1.0, 1.0, 1.0]), dt, dd, n, False), (put(J, (1, 2), nan), dt, dd, n, False),
            (J, put(dt, 1, nan), dd, n, False), (J, dt, put(dd, (2, 0), nan), n, False), (J, put(dt, 0, inf), dd, n, False),
            (J, dt, put(dd, (0, 1), -inf), n, False), (J, dt, dd, np.zeros(3), False), (J, dt, dd, put(n, 1, nan), False),
            (eye, np.zeros(3), dd, n, True)]
    a, b, c, d, v = zip(*rows)
    f = lambda z: torch.from_numpy(np.asarray(z, np.float64))
    return f(a), f(b), f(c), f(d), torch.tensor(v)


def test_validity_on_hand_made_rows():
    jac, d_t, dd, n, valid = hand_rows()
    out = kinematics.kinematics_rows(jac, d_t, dd, n)
    assert torch.equal(out["valid"], valid)
    for k, v in out.items():
        assert bool(torch.isfinite(v.double()).all()), k
        if k != "valid":
            assert not bool(v[~valid].abs().sum()), k          # zeros in every output of a row that is not valid
    assert float(out["speed"][0]) > 0 and float(out["L"][0].abs().max()) > 0
    assert not bool(out["velocity"][-1].abs().sum()) and not bool(out["L"][-1].abs().sum())          # at rest: v = 0, L = 0, valid
    # without normals the two rows with a bad normal are valid again; a NaN in d_xt is a NaN in an input
    bare = kinematics.kinematics_rows(jac, d_t, dd)
    assert torch.equal(bare["valid"], torch.tensor([True, False, False, False, False, False, False, True, True, True]))
    xt = torch.zeros(10, 3, 3, dtype=torch.float64)
    xt[0, 1, 1] = float("nan")
    assert not bool(kinematics.kinematics_rows(jac, d_t, dd, d_xt=xt)["valid"][0])
    for bad in (lambda: kinematics.kinematics_rows(jac, d_t[:5], dd), lambda: kinematics.kinematics_rows(jac, d_t, dd, n[:3])):
        with pytest.raises(ValueError):
            bad()
    empty = kinematics.kinematics_rows(jac[:0], d_t[:0], dd[:0], n[:0])
    assert empty["L"].shape == (0, 3, 3) and empty["surface_rates"].shape == (0, 2) and empty["principal_rates"].shape == (0, 3)


def test_mesh_kinematics_shapes_and_unconverged_rows():
    """A three-frame track of a 5 x 5 patch under the affine map: [F,V,...] maps, the default normals of each frame's vertices, rows of
    unconverged entries zero and not valid, and one call of ``derivs_fn`` with a time per row."""
    A = torch.tensor([[0.1, 0.2, 0.0], [-0.1, 0.05, 0.1], [0.0, 0.1, -0.2]], dtype=torch.float64)
    calls = []

    def fn(x, t):
        calls.append((tuple(x.shape), tuple(t.shape)))
        m = x.shape[0]
        return {"jac": torch.eye(3, dtype=torch.float64)[None] + t[:, None, None] * A[None], "d_t": x @ A.t(),
                "dd": torch.zeros(m, 3, 3, dtype=torch.float64), "d_xt": A[None].expand(m, 3, 3)}
    i, j = np.meshgrid(np.arange(5), np.arange(5), indexing="ij")
    v0 = torch.from_numpy(np.stack([0.1 * i.reshape(-1), 0.1 * j.reshape(-1), 0.02 * (i * j).reshape(-1)], -1).astype(np.float64))
    q = (i[:-1, :-1] * 5 + j[:-1, :-1]).reshape(-1)
    tris = torch.from_numpy(np.concatenate([np.stack([q, q + 5, q + 6], 1), np.stack([q, q + 6, q + 1], 1)]).astype(np.int32))
    times = torch.tensor([0.2, 0.5, 0.8], dtype=torch.float64)
    canon = v0 + 0.2 * v0 @ A.t()
    verts = torch.stack([torch.linalg.solve(torch.eye(3, dtype=torch.float64) + tt * A, canon.t()).t() for tt in times])
    conv = torch.ones(3, 25, dtype=torch.bool)
    conv[1, 7] = conv[2, 0] = False
    track = {"vertices": verts, "triangles": tris, "converged": conv, "canonical": canon}
    out = kinematics.mesh_kinematics(fn, track, times)
    assert calls == [((75, 3), (75,))]
    shapes = {"velocity": (3, 25, 3), "speed": (3, 25), "L": (3, 25, 3, 3), "rate": (3, 25, 3, 3), "principal_rates": (3, 25, 3),
              "divergence": (3, 25), "vorticity": (3, 25, 3), "area_rate": (3, 25), "surface_rates": (3, 25, 2), "valid": (3, 25)}
    assert {k: tuple(v.shape) for k, v in out.items()} == shapes
    assert torch.equal(out["valid"], conv)
    for k, v in out.items():
        if k != "valid":
            assert not bool(v[~conv].abs().sum()), k
    # the rows are the per-point rows at each frame's own time, with that frame's normals
    from endosurf_amd.meshing import vertex_normals
    n1 = torch.from_numpy(vertex_normals(verts[1].numpy(), tris.numpy()))
    one = kinematics.point_kinematics(fn, verts[1], 0.5, n1)
    keep = conv[1]
    assert all(torch.equal(out[k][1][keep], one[k][keep]) for k in one)
    want = -torch.linalg.solve(torch.eye(3, dtype=torch.float64) + 0.5 * A, A)
    assert float((out["L"][1][keep] - want[None]).abs().max()) <= 1e-13
    given = kinematics.mesh_kinematics(fn, track, times, normals=torch.stack([n1, n1, n1]))
    assert torch.equal(given["area_rate"][1], out["area_rate"][1])
    seen = []
    kinematics.mesh_kinematics(fn, track, times, rows_fn=lambda *a: (seen.append(len(a)), kinematics.kinematics_rows(*a))[1])
    assert seen == [4]
    with pytest.raises(ValueError):
        kinematics.mesh_kinematics(fn, track, times[:2])
