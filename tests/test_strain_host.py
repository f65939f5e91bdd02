"""CPU: tissue strain along surface tracks on the host (endosurf_amd/strain.py): an affine deformation, where everything is exact;
finite differences of the tracked map of the fp64 oracle; the per-row algebra against numpy's SVD; the rows that are not valid."""
import numpy as np
import pytest
import torch

import weightgen
from oracle import endosurf_oracle as O

from endosurf_amd import strain, tracking

EYE = np.eye(3)


def _affine():
    """D(y, t) = t A y with |A|_2 = 0.4: J = I + t A wherever, a contraction for every t in [0, 1]."""
    A = np.random.default_rng(5).normal(size=(3, 3))
    A = torch.from_numpy(A * (0.4 / np.linalg.norm(A, 2)))
    deform_fn = lambda y, t: t[:, None] * (y @ A.T)
    jacobian_fn = lambda y, t: torch.eye(3, dtype=y.dtype)[None] + t[:, None, None] * A[None]
    return A, deform_fn, jacobian_fn


def _patch(n, origin, eu, ev):
    """An n x n vertex patch origin + i eu + j ev, two triangles per cell."""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    v = np.asarray(origin)[None] + i.reshape(-1, 1) * np.asarray(eu)[None] + j.reshape(-1, 1) * np.asarray(ev)[None]
    q = (i[:-1, :-1] * n + j[:-1, :-1]).reshape(-1)
    tris = np.concatenate([np.stack([q, q + n, q + n + 1], 1), np.stack([q, q + n + 1, q + 1], 1)])
    return torch.from_numpy(v), torch.from_numpy(tris.astype(np.int64))


def test_affine_map_gives_the_closed_form():
    A, deform_fn, jacobian_fn = _affine()
    rng = np.random.default_rng(6)
    x = torch.from_numpy(rng.uniform(-0.8, 0.8, size=(50, 3)))
    t_a, t_b = torch.from_numpy(rng.uniform(size=50)), torch.from_numpy(rng.uniform(size=50))
    w = tracking.warp_points(deform_fn, x, t_a, t_b, max_iters=300, tol=1e-14)
    assert bool(w["converged"].all())
    out = strain.track_strain(jacobian_fn, x, t_a, w["points"], t_b)
    want = np.stack([np.linalg.inv(EYE + tb * A.numpy()) @ (EYE + ta * A.numpy()) for ta, tb in zip(t_a.tolist(), t_b.tolist())])
    assert bool(out["valid"].all()) and out["F"].dtype == torch.float64
    assert float(np.abs(out["F"].numpy() - want).max()) <= 1e-13
    assert float(np.abs(out["det"].numpy() - np.linalg.det(want)).max()) <= 1e-13
    # relative to the canonical shape: F = J(y_b, t_b)^-1, whatever t_from says
    can = strain.track_strain(jacobian_fn, None, None, w["points"], t_b)
    want = np.stack([np.linalg.inv(EYE + tb * A.numpy()) for tb in t_b.tolist()])
    assert float(np.abs(can["F"].numpy() - want).max()) <= 1e-13 and "area" not in can


@pytest.mark.parametrize("tilted", [True, False], ids=["tilted_given_normals", "axis_plane_default_normals"])
def test_affine_map_triangle_areas_equal_the_area_ratio(tilted):
    """A flat mesh under an affine map: every triangle's area changes by exactly |cof(F) n|, n the plane's normal.  The tilted plane
    gets its normal in fp64; the plane z = const takes the default normals, ``meshing.vertex_normals``, which are exact there (fp32
    normals of a tilted plane are 6e-8 off the direction, and the area ratio with them)."""
    A, deform_fn, jacobian_fn = _affine()
    if tilted:
        eu, ev = np.array([0.1, 0.02, -0.03]), np.array([-0.01, 0.09, 0.04])
        n = np.cross(eu, ev)
        verts, tris = _patch(5, [-0.2, -0.25, 0.1], eu, ev)
        normals = torch.from_numpy(np.broadcast_to(3.0 * n, (25, 3)).copy())          # (any positive length)
    else:
        verts, tris = _patch(5, [-0.2, -0.25, 0.1], [0.1, 0.0, 0.0], [0.0, 0.09, 0.0])
        normals = None
    times = torch.tensor([0.3, 0.6, 0.9], dtype=torch.float64)
    track = tracking.track_mesh(deform_fn, verts, tris, 0.3, times, max_iters=300, tol=1e-14)
    assert bool(track["converged"].all())
    out = strain.mesh_strain(jacobian_fn, track, times, reference=0, normals=normals)
    ratio = strain.triangle_area_ratio(track["vertices"][0], track["vertices"], tris)
    assert tuple(ratio.shape) == (3, 32) and bool(out["valid"].all())
    err = float((out["area"][:, tris] - ratio[:, :, None]).abs().max())
    print(f"\n[affine {'tilted' if tilted else 'axis'}] |area - triangle ratio| {err:.3e}; ratios {ratio[:, 0].tolist()}")
    assert err <= 1e-10
    assert float((ratio[0] - 1).abs().max()) <= 1e-12 and float((ratio[2] - 1).abs().min()) > 1e-3
    # the product of the surface stretches is the area ratio
    assert float((out["surface_stretch"].prod(-1) - out["area"]).abs().max()) <= 1e-12


@pytest.mark.parametrize("seed", [11, 21])
def test_finite_differences_of_the_tracked_map(seed):
    """F = J(y_b, t_b)^-1 J(x, t_a) against the central difference of ``tracking.warp_points`` on the fp64 oracle, h = 1e-7.  The map
    is piecewise linear, so the difference is exact except where a stencil crosses a ReLU kink: at least 99 % of the rows agree within
    1e-7.  (The oracle alone leaves out 5 and 6 of the 2 000 rows; the others agree to 1.6e-9 at the 99th percentile.)"""
    state = weightgen.make_state(seed, "trained", True)
    net = O.OracleNet({k: torch.tensor(v, dtype=torch.float64) for k, v in state.items()}, True)

    def deform_fn(y, t):
        with torch.no_grad():
            return net.deform(y, t, with_jac=False)[0]

    def jacobian_fn(y, t):
        with torch.no_grad():
            return net.deform(y, t)[1]
    rng = np.random.default_rng(7)
    M, h = 2000, 1e-7
    x = torch.from_numpy(rng.uniform(-0.8, 0.8, size=(M, 3)))
    t_a = torch.from_numpy(rng.uniform(size=M))
    t_b = torch.from_numpy(rng.uniform(size=M))
    offs = torch.cat([torch.zeros(1, 3, dtype=torch.float64), h * torch.eye(3, dtype=torch.float64), -h * torch.eye(3, dtype=torch.float64)])
    pts = (x[None] + offs[:, None]).reshape(7 * M, 3)          # the points, then +h e_0..2, then -h e_0..2
    w = tracking.warp_points(deform_fn, pts, t_a.repeat(7), t_b.repeat(7), max_iters=300, tol=1e-13)
    assert bool(w["converged"].all())
    y = w["points"].reshape(7, M, 3)
    fd = torch.stack([(y[1 + j] - y[4 + j]) / (2 * h) for j in range(3)], dim=-1)          # column j = d Phi / d x_j
    out = strain.track_strain(jacobian_fn, x, t_a, y[0], t_b)
    assert bool(out["valid"].all())
    err = (out["F"] - fd).abs().reshape(M, 9).max(-1)[0]
    good = err <= 1e-7
    print(f"\n[trained{seed}] rows off by more than 1e-7: {int((~good).sum())} of {M}; the others: 99th percentile "
          f"{float(torch.quantile(err[good], 0.99)):.3e}, max {float(err[good].max()):.3e}")
    assert int(good.sum()) >= 0.99 * M


def _random_F(M, seed, scale=0.3):
    G = np.random.default_rng(seed).normal(size=(M, 3, 3))
    return EYE[None] + scale * G / np.linalg.norm(G, 2, axis=(1, 2))[:, None, None]


def _plane_basis(n):
    """An orthonormal basis [3,2] of the plane normal to n, by QR (another construction than the module's)."""
    q, _ = np.linalg.qr(np.concatenate([n.reshape(3, 1) / np.linalg.norm(n), EYE], 1))
    return q[:, 1:3]


def test_stretches_against_numpy_svd():
    M = 300
    Ja, Jb = _random_F(M, 1), _random_F(M, 2)
    n = np.random.default_rng(3).normal(size=(M, 3))
    out = strain.strain_rows(torch.from_numpy(Ja), torch.from_numpy(Jb), torch.from_numpy(n))
    F = np.linalg.inv(Jb) @ Ja
    assert bool(out["valid"].all())
    assert float(np.abs(out["F"].numpy() - F).max()) <= 1e-13
    assert float(np.abs(out["stretch"].numpy() - np.linalg.svd(F, compute_uv=False)).max()) <= 1e-13
    surf = np.stack([np.linalg.svd(F[i] @ _plane_basis(n[i]), compute_uv=False) for i in range(M)])
    assert float(np.abs(out["surface_stretch"].numpy() - surf).max()) <= 1e-13
    nn = n / np.linalg.norm(n, axis=1, keepdims=True)
    area = np.linalg.det(F) * np.linalg.norm(np.einsum("mji,mj->mi", np.linalg.inv(F), nn), axis=1)          # det F |F^-T n|
    assert float(np.abs(out["area"].numpy() - area).max()) <= 1e-12
    # the invariants: the product of the stretches is the volume ratio, of the surface stretches the area ratio
    assert float((out["stretch"].prod(-1) - out["det"]).abs().max()) <= 1e-12
    assert float((out["surface_stretch"].prod(-1) - out["area"]).abs().max()) <= 1e-12
    # descending
    assert bool((out["stretch"][:, :-1] >= out["stretch"][:, 1:]).all()) and bool((out["surface_stretch"][:, 0] >= out["surface_stretch"][:, 1]).all())
    # fp32 inputs come back as fp32, computed in fp64 from the fp32 values
    o32 = strain.strain_rows(torch.from_numpy(Ja).float(), torch.from_numpy(Jb).float(), torch.from_numpy(n).float())
    o64 = strain.strain_rows(torch.from_numpy(Ja).float().double(), torch.from_numpy(Jb).float().double(), torch.from_numpy(n).float().double())
    assert all(o32[k].dtype == (torch.bool if k == "valid" else torch.float32) for k in o32)
    assert all(torch.equal(o32[k], o64[k].to(o32[k].dtype)) for k in o32)


def test_identity_rotation_and_coincident_stretches():
    eye = torch.eye(3, dtype=torch.float64)[None]
    out = strain.strain_rows(None, eye, torch.tensor([[0.0, 0.0, 2.0]], dtype=torch.float64))
    assert torch.equal(out["stretch"], torch.ones(1, 3, dtype=torch.float64)) and torch.equal(out["F"], eye)
    assert torch.equal(out["surface_stretch"], torch.ones(1, 2, dtype=torch.float64))
    assert float(out["det"]) == 1.0 and float(out["area"]) == 1.0
    # the coincident-eigenvalue case, F = I + 1e-9 G: to 1e-14 of the SVD
    G = np.random.default_rng(4).normal(size=(64, 3, 3))
    F = EYE[None] + 1e-9 * G
    n = np.random.default_rng(5).normal(size=(64, 3))
    out = strain.strain_rows(torch.from_numpy(F), eye.expand(64, 3, 3), torch.from_numpy(n))
    assert float(np.abs(out["stretch"].numpy() - np.linalg.svd(F, compute_uv=False)).max()) <= 1e-14
    surf = np.stack([np.linalg.svd(F[i] @ _plane_basis(n[i]), compute_uv=False) for i in range(64)])
    assert float(np.abs(out["surface_stretch"].numpy() - surf).max()) <= 1e-14
    assert float((out["stretch"] - 1).abs().max()) > 1e-10          # (and they are not all 1)
    # a pure rotation: stretches of 1, area and volume kept
    q, _ = np.linalg.qr(np.random.default_rng(6).normal(size=(3, 3)))
    q = q * np.sign(np.linalg.det(q))
    out = strain.strain_rows(torch.from_numpy(q)[None], eye, torch.tensor([[0.3, -0.5, 0.8]], dtype=torch.float64))
    assert bool(out["valid"].all())
    assert float((out["stretch"] - 1).abs().max()) <= 1e-15 and float((out["surface_stretch"] - 1).abs().max()) <= 1e-15
    assert abs(float(out["det"]) - 1) <= 1e-15 and abs(float(out["area"]) - 1) <= 1e-15


def test_a_diagonal_stretch():
    F = torch.diag(torch.tensor([2.0, 1.0, 0.5], dtype=torch.float64))[None]
    z = strain.strain_rows(F, torch.eye(3, dtype=torch.float64)[None], torch.tensor([[0.0, 0.0, 1.0]], dtype=torch.float64))
    assert z["stretch"].tolist() == [[2.0, 1.0, 0.5]] and float(z["det"]) == 1.0
    assert float(z["area"]) == 2.0 and z["surface_stretch"].tolist() == [[2.0, 1.0]]
    x = strain.strain_rows(F, torch.eye(3, dtype=torch.float64)[None], torch.tensor([[1.0, 0.0, 0.0]], dtype=torch.float64))
    assert float(x["area"]) == 0.5 and x["surface_stretch"].tolist() == [[1.0, 0.5]]
    # the same F as a quotient: jac_to = F^-1
    q = strain.strain_rows(None, torch.diag(torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64))[None], torch.tensor([[0.0, 0.0, 5.0]], dtype=torch.float64))
    assert q["stretch"].tolist() == [[2.0, 1.0, 0.5]] and float(q["area"]) == 2.0


def test_rows_that_are_not_valid():
    good = _random_F(6, 8)
    flip = good.copy()
    flip[:, 0] *= -1.0          # a negative determinant
    nan = good.copy()
    nan[:, 1, 2] = np.nan
    n = np.random.default_rng(9).normal(size=(6, 3))
    g, f, a, nn = (torch.from_numpy(v) for v in (good, flip, nan, n))

    def all_zero(out, rows):
        for k, v in out.items():
            assert bool(torch.isfinite(v.double()).all()), k
            assert not bool(v[rows].double().abs().sum()), k          # zeros, and valid False
    for ja, jb in ((f, g), (g, f), (a, g), (g, a), (None, f), (None, a)):
        for normals in (None, nn):
            out = strain.strain_rows(ja, jb, normals)
            all_zero(out, slice(None))
    # one bad row leaves its neighbours alone
    mixed = g.clone()
    mixed[2] = f[2]
    mixed[4] = a[4]
    zn = nn.clone()
    zn[1] = 0.0
    zn[3, 0] = float("nan")
    zn[5, 1] = float("inf")
    out, ref = strain.strain_rows(g, mixed, zn), strain.strain_rows(g, g, nn)
    assert out["valid"].tolist() == [True, False, False, False, False, False]
    all_zero(out, slice(1, None))
    assert all(torch.equal(out[k][:1], ref[k][:1]) for k in out)
    # without normals, a row's normal cannot make it invalid
    assert strain.strain_rows(g, mixed)["valid"].tolist() == [True, True, False, True, False, True]
    # no rows at all
    empty = strain.strain_rows(None, torch.zeros(0, 3, 3), torch.zeros(0, 3))
    assert {k: tuple(v.shape) for k, v in empty.items()} == {"F": (0, 3, 3), "det": (0,), "stretch": (0, 3), "area": (0,),
                                                             "surface_stretch": (0, 2), "valid": (0,)}


def test_mesh_strain_shapes_references_and_convergence():
    A, deform_fn, jacobian_fn = _affine()
    verts, tris = _patch(4, [-0.2, -0.25, 0.1], [0.1, 0.02, -0.03], [-0.01, 0.09, 0.04])
    times = torch.tensor([0.2, 0.5, 0.8, 1.0], dtype=torch.float64)
    track = tracking.track_mesh(deform_fn, verts, tris, 0.5, times, max_iters=300, tol=1e-14)
    out = strain.mesh_strain(jacobian_fn, track, times, reference=1)
    want = {"F": (4, 16, 3, 3), "det": (4, 16), "stretch": (4, 16, 3), "area": (4, 16), "surface_stretch": (4, 16, 2), "valid": (4, 16)}
    assert {k: tuple(v.shape) for k, v in out.items()} == want and bool(out["valid"].all())
    # the reference frame against itself: nothing moves (J is evaluated once, so J^-1 J cancels to rounding)
    assert float((out["F"][1] - torch.eye(3, dtype=torch.float64)).abs().max()) <= 1e-15
    assert float((out["stretch"][1] - 1).abs().max()) <= 1e-15 and float((out["area"][1] - 1).abs().max()) <= 1e-6
    # frame f against frame 1 is the closed form
    for f, t in enumerate(times.tolist()):
        F = np.linalg.inv(EYE + t * A.numpy()) @ (EYE + 0.5 * A.numpy())
        assert float(np.abs(out["F"][f].numpy() - F[None]).max()) <= 1e-13
    # the canonical reference: F = J(y_f, t_f)^-1 at the canonical vertices' normals
    can = strain.mesh_strain(jacobian_fn, track, times, reference="canonical")
    assert {k: tuple(v.shape) for k, v in can.items()} == want
    for f, t in enumerate(times.tolist()):
        assert float(np.abs(can["F"][f].numpy() - np.linalg.inv(EYE + t * A.numpy())[None]).max()) <= 1e-13
    # ``valid`` includes the track's ``converged``, of the frame and of the reference frame; rows that are not valid are zero
    conv = track["converged"].clone()
    conv[2, 5] = False          # one vertex of frame 2
    conv[1, 7] = False          # one vertex of the reference frame: that vertex in every frame
    out2 = strain.mesh_strain(jacobian_fn, dict(track, converged=conv), times, reference=1)
    expect = torch.ones(4, 16, dtype=torch.bool)
    expect[2, 5] = False
    expect[:, 7] = False
    assert torch.equal(out2["valid"], expect)
    for k in ("F", "det", "stretch", "area", "surface_stretch"):
        assert not bool(out2[k][~expect].abs().sum()) and torch.equal(out2[k][expect], out[k][expect])
    can2 = strain.mesh_strain(jacobian_fn, dict(track, converged=conv), times, reference="canonical")
    assert torch.equal(can2["valid"], conv)
    with pytest.raises(ValueError):
        strain.mesh_strain(jacobian_fn, track, times, reference=4)
    with pytest.raises(ValueError):
        strain.mesh_strain(jacobian_fn, track, times[:3])
