"""CPU: ``endosurf_amd.curvature`` -- ``curvature_rows`` on closed forms, its ordering, identities and validity rule, and
``compose_hessian`` against autograd through the fp64 oracle's observed-space SDF.  Every test prints the figures it asserts on."""
import numpy as np
import pytest
import torch

import weightgen
from curvature_ref import hessian_canonical, hessian_observed
from point_adjoint_ref import sweep
from shapes_util import inputs
from track_util import oracle_net

from endosurf_amd import curvature

CASES = [(11, "trained"), (23, "trained"), (21, "init")]
M = 200


def points_on_sphere(n, R, seed):
    p = np.random.default_rng(seed).normal(size=(n, 3))
    return torch.from_numpy(R * p / np.linalg.norm(p, axis=-1, keepdims=True))


def sphere_distance(x, R):
    """g, H of |x| - R."""
    r = x.norm(dim=-1)
    n = x / r[:, None]
    return n, (torch.eye(3, dtype=x.dtype)[None] - n[:, :, None] * n[:, None, :]) / r[:, None, None]


def worst(got, want):
    return float((got.double() - torch.as_tensor(want, dtype=torch.float64)).abs().max())


@pytest.mark.parametrize("R", [0.25, 1.0, 3.5])
def test_sphere_both_ways(R):
    """|x| - R and |x|^2 - R^2 (the same surface, |g| = 2R): both principal curvatures +1/R seen from outside, to 1e-12."""
    x = points_on_sphere(64, R, 1)
    g, H = sphere_distance(x, R)
    for name, (gg, HH) in {"distance": (g, H), "squared": (2.0 * x, 2.0 * torch.eye(3, dtype=torch.float64).expand(64, 3, 3))}.items():
        out = curvature.curvature_rows(gg, HH)
        e = max(worst(out["principal"], 1.0 / R), worst(out["mean"], 1.0 / R), worst(out["gauss"], 1.0 / R ** 2))
        print(f"sphere R {R} ({name}): {e:.3e}")
        assert bool(out["valid"].all()) and e <= 1e-12


def test_cylinder():
    """sqrt(x^2 + y^2) - R: principal curvatures (1/R, 0)."""
    R = 0.6
    rng = np.random.default_rng(2)
    phi, z = rng.uniform(0, 2 * np.pi, 64), rng.uniform(-1, 1, 64)
    n = torch.from_numpy(np.stack([np.cos(phi), np.sin(phi), 0 * z], -1))
    ez = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64)
    H = (torch.eye(3, dtype=torch.float64)[None] - n[:, :, None] * n[:, None, :] - ez[None, :, None] * ez[None, None, :]) / R
    out = curvature.curvature_rows(n, H)
    e = max(worst(out["principal"][:, 0], 1.0 / R), worst(out["principal"][:, 1], 0.0), worst(out["mean"], 0.5 / R), worst(out["gauss"], 0.0))
    print(f"cylinder: {e:.3e}")
    assert bool(out["valid"].all()) and e <= 1e-12


@pytest.mark.parametrize("alpha,beta", [(1.5, 0.5), (2.0, -1.0), (-0.5, -3.0), (0.7, 0.7)])
def test_paraboloid_at_the_origin(alpha, beta):
    """f = z - (alpha x^2 + beta y^2) / 2 at the origin: g = e_z, H = -diag(alpha, beta, 0), so with n towards increasing f the principal
    curvatures are (-alpha, -beta), in descending order: the graph z = (alpha x^2 + beta y^2) / 2 bends TOWARDS n where alpha > 0, and a
    surface that bends away from its normal (the sphere seen from outside) is the positive one."""
    g = torch.tensor([[0.0, 0.0, 1.0]], dtype=torch.float64)
    H = -torch.diag(torch.tensor([alpha, beta, 0.0], dtype=torch.float64))[None]
    out = curvature.curvature_rows(g, H)
    want = sorted([-alpha, -beta], reverse=True)
    e = max(worst(out["principal"][0], want), worst(out["mean"], -(alpha + beta) / 2), worst(out["gauss"], alpha * beta))
    print(f"paraboloid ({alpha}, {beta}): {e:.3e}")
    assert e <= 1e-12


def test_order_and_identities():
    """Random symmetric Hessians and gradients: principal is descending, kappa_1 kappa_2 = gauss and (kappa_1 + kappa_2) / 2 = mean; the
    result does not depend on the length of the gradient's scaling of the pair (g, H) together; dtype and shape of the inputs kept."""
    rng = np.random.default_rng(5)
    A = rng.normal(size=(300, 3, 3))
    H = torch.from_numpy(A + A.transpose(0, 2, 1))
    g = torch.from_numpy(rng.normal(size=(300, 3)))
    out = curvature.curvature_rows(g, H)
    k1, k2 = out["principal"][:, 0], out["principal"][:, 1]
    assert bool(out["valid"].all()) and bool((k1 >= k2).all())
    scale = float(out["principal"].abs().max())
    e_g, e_m = worst(k1 * k2, out["gauss"]) / scale ** 2, worst(0.5 * (k1 + k2), out["mean"]) / scale
    print(f"identities: gauss {e_g:.3e}  mean {e_m:.3e}")
    assert e_g <= 1e-12 and e_m <= 1e-12
    again = curvature.curvature_rows(3.0 * g, 3.0 * H)
    assert worst(again["principal"], out["principal"]) / scale <= 1e-12
    f32 = curvature.curvature_rows(g.float(), H.float())
    assert f32["mean"].dtype == torch.float32 and f32["principal"].shape == (300, 2) and f32["valid"].dtype == torch.bool
    empty = curvature.curvature_rows(g[:0], H[:0])
    assert empty["mean"].shape == (0,) and empty["principal"].shape == (0, 2) and empty["valid"].shape == (0,)


def test_rows_that_are_not_valid_are_zero():
    """A zero, NaN or infinite gradient and a NaN or infinite entry of the Hessian: not valid, zeros; their neighbours untouched."""
    x = points_on_sphere(7, 1.0, 3)
    g, H = sphere_distance(x, 1.0)
    g, H = g.clone(), H.clone()
    g[1] = 0.0
    g[2, 1] = float("nan")
    g[3, 0] = float("inf")
    H[4, 1, 2] = float("nan")
    H[5, 0, 0] = float("inf")
    out = curvature.curvature_rows(g, H)
    assert out["valid"].tolist() == [True, False, False, False, False, False, True]
    bad = ~out["valid"]
    for k in ("mean", "gauss", "principal"):
        assert bool((out[k][bad] == 0).all()) and bool(torch.isfinite(out[k]).all())
    assert worst(out["principal"][out["valid"]], 1.0) <= 1e-12


def test_compose_hessian_identity_and_shapes():
    rng = np.random.default_rng(8)
    g, H = torch.from_numpy(rng.normal(size=(5, 3))), torch.from_numpy(rng.normal(size=(5, 3, 3)))
    go, Ho = curvature.compose_hessian(g, H)
    assert torch.equal(go, g) and torch.equal(Ho, H)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    J = torch.from_numpy(q)[None].expand(5, 3, 3)
    dd = torch.from_numpy(rng.normal(size=(5, 3)))
    go, Ho = curvature.compose_hessian(g, H, J, dd)
    want = J.transpose(1, 2) @ H @ J - torch.diag_embed(dd)
    assert worst(go, torch.einsum("mik,mi->mk", J, g)) <= 1e-14 and worst(Ho, want) <= 1e-14
    with pytest.raises(ValueError):
        curvature.compose_hessian(g, H[:4])


@pytest.mark.parametrize("seed,mode", CASES, ids=lambda v: str(v))
def test_compose_hessian_against_the_observed_autograd_hessian(seed, mode):
    """H_o = J^T H_c J - diag(CURV(g_c)) and g_o = J^T g_c, from the fp64 oracle's pieces on the 200 screened rows of
    ``shapes_util.inputs``, against autograd through ``sdf_observed``: within 1e-12 (measured 3e-14; the entries reach 19 to 35 on the
    trained states)."""
    net = oracle_net(weightgen.make_state(seed, mode, True), torch.float64)
    x, _, t, _, _, _ = inputs(M, seed)
    x, t = x.double(), t.double()
    with torch.no_grad():
        d, J = net.deform(x, t)
    _, gc, Hc = hessian_canonical(net, x + d)
    _, dd, _ = sweep(net, x, t, gc)
    go, Ho = curvature.compose_hessian(gc, Hc, J, dd)
    _, go_ref, Ho_ref = hessian_observed(net, x, t)
    e_g, e_h = worst(go, go_ref), worst(Ho, Ho_ref)
    print(f"[{mode}{seed}] compose against autograd: gradient {e_g:.3e}  Hessian {e_h:.3e}  (max |H_o| {float(Ho_ref.abs().max()):.1f})")
    assert e_g <= 1e-12 and e_h <= 1e-12


def test_surface_and_mesh_curvature_compose():
    """``surface_curvature`` and ``mesh_curvature`` over an analytic field (a sphere that grows with time): [V] maps for a mesh at one
    time, [F,V] maps for a track, unconverged rows not valid and zero, ``rows_fn`` used when given."""
    def hessian_fn(p, t):          # |x| - (1 + t)
        g, H = sphere_distance(p, 1.0)
        return (p.norm(dim=-1) - (1.0 + t))[:, None], g, H
    V, F = 12, 3
    unit = points_on_sphere(V, 1.0, 4)
    times = torch.tensor([0.0, 0.5, 1.0], dtype=torch.float64)
    sc = curvature.surface_curvature(hessian_fn, 2.0 * unit, 1.0)
    assert set(sc) == {"sdf", "gradient", "hessian", "mean", "gauss", "principal", "valid"}
    assert worst(sc["mean"], 0.5) <= 1e-12 and worst(sc["sdf"], 0.0) <= 1e-12
    mesh = curvature.mesh_curvature(hessian_fn, {"vertices": 2.0 * unit, "triangles": None}, 1.0)
    assert mesh["mean"].shape == (V,) and torch.equal(mesh["mean"], sc["mean"]) and torch.equal(mesh["principal"], sc["principal"])
    conv = torch.ones(F, V, dtype=torch.bool)
    conv[1, 5] = False
    track = {"vertices": (1.0 + times)[:, None, None] * unit[None], "converged": conv, "triangles": None}
    out = curvature.mesh_curvature(hessian_fn, track, times)
    assert out["mean"].shape == (F, V) and out["principal"].shape == (F, V, 2) and torch.equal(out["valid"], conv)
    want = (1.0 / (1.0 + times))[:, None].expand(F, V).clone()
    want[1, 5] = 0.0
    assert worst(out["mean"], want) <= 1e-12 and float(out["gauss"][1, 5]) == 0.0 and out["principal"][1, 5].tolist() == [0.0, 0.0]
    calls = []
    def rows_fn(g, H):
        calls.append(g.shape[0])
        return curvature.curvature_rows(g, H)
    curvature.mesh_curvature(hessian_fn, track, times, rows_fn=rows_fn)
    assert calls == [F * V]
    with pytest.raises(ValueError):
        curvature.mesh_curvature(hessian_fn, track, times[:2])
