"""CPU: endosurf_amd.geodesic, the specification and fp64 twin of csrc/geodesic.hip -- exact cases, independence of the order of the
updates, accuracy against the great-circle distance and against Dijkstra on the edge graph, point sources and targets, tracks."""
import math

import numpy as np
import pytest

from endosurf_amd import geodesic as G
from geodesic_util import (INF, NAN, bumpy, check_exact, dijkstra, exact_cases, gauss_seidel, great_circle, grid_mesh, rigid_track,
                           sphere_mesh, twin_sphere, ulps)


def solve(v, f, src):
    out = G.mesh_geodesic(v, f, src)
    assert out["sweeps"] <= max(len(v), 1)
    return out["distance"], out["sweeps"]


@pytest.mark.parametrize("name", list(exact_cases()))
def test_exact_cases(name):
    check_exact(name, solve)


def test_corner_update_on_a_right_triangle():
    """A plane wave along e1 of a right corner with legs 1/4: t = ua + 1/4 exactly; a front too steep for the triangle falls back to
    the edges; an infinite neighbour contributes nothing."""
    c, a, b = (np.array(p, np.float64) for p in ([0, 0, 0], [0.25, 0, 0], [0, 0.25, 0]))
    assert G.corner_update(c, a, b, np.float64(0.5), np.float64(0.75)) == 0.75          # |grad| = 1 needs (t - .5)^2 + (t - .75)^2 = 1/16
    assert abs(G.corner_update(c, a, b, np.float64(0.5), np.float64(0.5)) - (0.5 + 0.25 / math.sqrt(2.0))) < 1e-15
    assert G.corner_update(c, a, b, np.float64(0.0), np.float64(1.0)) == 0.25            # no real root: the edge from a
    assert G.corner_update(c, a, b, np.float64(INF), np.float64(1.0)) == 1.25
    assert G.corner_update(c, a, b, np.float64(INF), np.float64(INF)) == INF
    # a sliver (collinear corners): the edges only
    assert G.corner_update(c, a, 2 * a, np.float64(1.0), np.float64(0.0)) == 0.5


@pytest.mark.parametrize("n,method", [(17, "tetrahedra"), (17, "cubes"), (33, "tetrahedra"), (33, "cubes")])
def test_order_of_the_updates_does_not_matter(n, method):
    """The same updates applied one at a time in random order reach a fixed point that is the Jacobi twin's up to fp64 rounding
    (printed; half an fp32 ulp there is 3e-8), so after rounding to fp32 only a rounding-boundary flip can
    differ: at most 1 ulp."""
    v, f, top = sphere_mesh(n, method)
    ref = twin_sphere(n, method)["distance"][0]
    start = np.full((1, len(v)), np.inf)
    start[0, top] = 0.0
    ref64 = G._Frame(v, f).solve(start)[0][0]          # the twin's field before it is rounded
    assert np.array_equal(ref64.astype(np.float32), ref)
    worst, flips = 0.0, 0
    for seed in range(3):
        u = gauss_seidel(v, f, top, seed)
        worst = max(worst, float(np.abs(u - ref64).max()))
        d = ulps(u.astype(np.float32), ref)
        flips += int((d > 0).sum())
        assert d.max() <= 1
    print(f"GEODESIC_MEASURED order {method} {n}^3: V={len(v)} max |u - twin| in fp64 {worst:.3e}, {flips} fp32 entries differ over 3 orders")


def _errors(n, method):
    v, f, top = sphere_mesh(n, method)
    exact = great_circle(v, top)
    far = exact > 0.05
    out = twin_sphere(n, method)
    assert out["sweeps"] <= len(v)
    twin = np.abs(out["distance"][0].astype(np.float64) - exact)[far] / exact[far]
    graph = np.abs(dijkstra(v, f, top) - exact)[far] / exact[far]
    print(f"GEODESIC_MEASURED sphere {method} {n}^3: V={len(v)} T={len(f)} sweeps={out['sweeps']} twin mean {twin.mean():.4%} max {twin.max():.2%}; "
          f"edge graph mean {graph.mean():.4%} max {graph.max():.2%}")
    return twin.mean(), graph.mean()


@pytest.mark.parametrize("method", ["tetrahedra", "cubes"])
def test_accuracy_on_the_sphere(method):
    """Against the analytic great-circle distance where it exceeds 0.05: the mean relative error is below the edge graph's at every
    resolution and does not grow from 17^3 to 65^3."""
    err = {n: _errors(n, method) for n in (17, 33, 65)}
    for n, (twin, graph) in err.items():
        assert twin < graph, (method, n)
    assert err[65][0] <= err[17][0], method


@pytest.mark.parametrize("n", [9, 17, 33])
def test_accuracy_on_the_planar_grid(n):
    v, f = grid_mesh(n, h=1.0 / (n - 1))
    exact = np.linalg.norm(v.astype(np.float64), axis=1)
    out = G.mesh_geodesic(v, f, np.array([0]))
    assert out["sweeps"] <= len(v)
    twin = np.abs(out["distance"][0][1:] - exact[1:]) / exact[1:]
    graph = np.abs(dijkstra(v, f, 0)[1:] - exact[1:]) / exact[1:]
    print(f"GEODESIC_MEASURED plane n={n}: twin max {twin.max():.4%}, edge graph max {graph.max():.4%}, sweeps {out['sweeps']}")
    assert twin.max() < graph.max()


def test_source_point_on_a_vertex_is_the_vertex_field():
    v, f, top = sphere_mesh(17)
    by_id = G.mesh_geodesic(v, f, np.array([top, 5]))
    by_point = G.mesh_geodesic(v, f, v[[top, 5]])
    assert by_point["distance"].shape == by_id["distance"].shape and ulps(by_point["distance"], by_id["distance"]).max() <= 1
    # off the mesh: no valid triangle, a non-finite point
    none = G.mesh_geodesic(v, np.array([[0, 0, 1]]), v[[top]])
    assert np.isinf(none["distance"]).all()
    nan = G.mesh_geodesic(v, f, np.array([[NAN, 0, 0], [0, 0, 1]], np.float32), targets=v[[3]])
    assert np.isinf(nan["distance"][0]).all() and np.isfinite(nan["distance"][1]).all()
    assert np.isinf(nan["target_distance"][0]).all() and np.isfinite(nan["target_distance"][1]).all()


def test_source_and_target_in_one_triangle_give_their_straight_distance():
    v, f = grid_mesh(5)
    p, q = np.array([[0.3125, 0.0625, 0.0]], np.float32), np.array([[0.4375, 0.125, 0.0], [0.875, 0.625, 0.0]], np.float32)
    out = G.mesh_geodesic(v, f, p, targets=q)
    assert out["target_distance"].shape == (1, 2) and out["distance"].shape == (1, 25)
    assert ulps(out["target_distance"][0, 0], np.float32(math.hypot(0.125, 0.0625))) <= 1
    straight = math.hypot(0.875 - 0.3125, 0.625 - 0.0625)          # the other target: the plane's distance, over-estimated by a few %
    assert straight <= out["target_distance"][0, 1] <= 1.05 * straight
    # the read-out at a vertex is the field there; a target on no triangle is unreachable
    at_vertices = G.mesh_geodesic(v, f, p, targets=v[[7, 24]])
    assert ulps(at_vertices["target_distance"][0], out["distance"][0, [7, 24]]).max() <= 1
    v2 = np.concatenate([v, v[:3] + [0, 0, 4.0]]).astype(np.float32)
    f2 = np.concatenate([f, [[25, 26, 27]]])
    apart = G.mesh_geodesic(v2, f2, p, targets=np.array([[0.0625, 0.0625, 4.0], [NAN, 0, 0]], np.float32))
    assert np.isinf(apart["target_distance"]).all()


def test_track_geodesic_on_rigid_and_scaled_copies():
    v, f = bumpy(9, 7)
    a = (0.75 * v[[1, 10, 30]] + 0.25 * v[[8, 17, 37]]).astype(np.float32)          # on edges and in triangles of frame 0
    b = ((v[[40, 52, 20]].astype(np.float64) + v[[47, 60, 28]] + v[[48, 59, 27]]) / 3.0).astype(np.float32)
    rigid = G.track_geodesic(rigid_track(v, f), a, b)
    assert rigid.shape == (3, 3) and rigid.dtype == np.float32 and np.isfinite(rigid).all() and (rigid > 0.1).all()
    assert ulps(rigid[1], rigid[0]).max() <= 1 and ulps(rigid[2], rigid[0]).max() <= 1
    scaled = G.track_geodesic(rigid_track(v, f, scaled=True), a, b)
    assert np.array_equal(scaled[0], rigid[0]) and np.array_equal(scaled[2], 2.0 * rigid[0])
    # the paired form is the diagonal of the full one, whatever the reference frame is called
    full = G.mesh_geodesic(rigid_track(v, f)["vertices"], f, a, targets=b, reference=-3)
    assert full["target_distance"].shape == (3, 3, 3) and np.array_equal(full["target_distance"][:, [0, 1, 2], [0, 1, 2]], rigid)
    assert full["distance"].shape == (3, 3, len(v)) and full["sweeps"] <= len(v)
    with pytest.raises(ValueError):
        G.track_geodesic(rigid_track(v, f), a, b[:2])


def test_arguments():
    v, f = grid_mesh(3)
    for bad in (dict(vertices=v[:, :2]), dict(sources=np.zeros((2, 2))), dict(sources=np.zeros(0, np.int64)), dict(reference=1)):
        kw = dict(vertices=v, triangles=f, sources=np.array([0]))
        kw.update(bad)
        ref = kw.pop("reference", 0)
        with pytest.raises(ValueError):
            G.mesh_geodesic(kw["vertices"], kw["triangles"], kw["sources"], reference=ref)
    with pytest.raises(ValueError):
        G.mesh_geodesic(v, f.astype(np.float32), np.array([0]))
