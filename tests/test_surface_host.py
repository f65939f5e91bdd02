"""CPU: the numpy twin of csrc/surface.hip (endosurf_amd.meshing.point_to_mesh, the specification of DESIGN.md 7f) against an
independently written form and against answers known exactly, the sphere probe behind the metric, and the library's argument checks."""
import ctypes as C

import numpy as np
import pytest

from endosurf_amd import data as D
from endosurf_amd import meshing as M
from surface_util import D2_TOL, check_exact, ericson_d2, exact_cases, soup, sphere_probe


def test_twin_against_ericsons_seven_regions():
    """|d2_twin - d2_other| <= 2^-40 (both fp64, ~20 operations on magnitudes up to L^2 <= 12: below 2^-44 L^2, 16 x margin), and the
    twin's triangle is a minimiser of the other form within the same bound."""
    v, f, q = soup(200, 400, seed=7)
    assert len(f) == 200 and len(q) == 400 and np.abs(q).max() <= 1.0
    dist, arg, at, d2 = M.point_to_mesh(q, v, f, return_d2=True)
    other = ericson_d2(q, v, f)
    assert d2.shape == other.shape == (400, 200)
    j = np.arange(400)
    err = np.abs(d2.min(1) - other.min(1)).max()
    slack = (other[j, arg] - other.min(1)).max()
    print(f"SURFACE_MEASURED twin vs Ericson: max |d2 - d2'| = {err:.3e}, chosen triangle above the minimum by {slack:.3e} (bound {D2_TOL:.3e})")
    assert err <= D2_TOL and slack <= D2_TOL
    assert np.abs(d2 - other).max() <= D2_TOL                               # every pair, not only the winners
    # the outputs are the matrix's minimum, its first place, and a point at that distance on the chosen triangle
    assert np.array_equal(arg, d2.argmin(1)) and np.array_equal(dist, np.sqrt(d2.min(1)).astype(np.float32))
    assert np.abs(((q.astype(np.float64) - at) ** 2).sum(1) - d2.min(1)).max() <= 2.0 ** -20
    # on a vertex, in an edge, in a face: distance 0 up to the rounding of the query to fp32
    assert dist[140:230].max() <= 2.0 ** -22
    # chunking does not show
    d1 = M.point_to_mesh(q, v, f, chunk=1000)
    assert all(np.array_equal(a, b) for a, b in zip(d1, (dist, arg, at)))


@pytest.mark.parametrize("name", list(exact_cases()))
def test_exact_cases(name):
    v, f, q = exact_cases()[name][:3]
    check_exact(name, M.point_to_mesh(q, v, f))


def test_the_answer_does_not_depend_on_the_order_of_the_triangles():
    v, f, q = soup(60, 300, seed=3)
    dist, arg, at, d2 = M.point_to_mesh(q, v, f, return_d2=True)
    perm = np.random.default_rng(1).permutation(len(f))
    dist2, arg2, at2 = M.point_to_mesh(q, v, f[perm])
    assert np.array_equal(dist, dist2) and np.array_equal(at, at2)
    assert np.array_equal(d2[np.arange(len(q)), perm[arg2]], d2.min(1))          # a tie may name another triangle, never a farther one
    with pytest.raises(ValueError):
        M.point_to_mesh(q, v, f.astype(np.float32))
    with pytest.raises(ValueError):
        M.point_to_mesh(q, v, f[:, :2])


@pytest.fixture(scope="module")
def probe():
    return sphere_probe()


@pytest.mark.parametrize("clustered", [False, True])
def test_sphere_probe_surface_distance_is_far_below_the_vertex_distance(probe, clustered):
    """Points ON the sphere: the distance to the nearest vertex reports a quarter of a lattice cell, the distance to the triangles what
    the triangulation really misses.  mean(dist) < 0.2 x the mean nearest-vertex distance (measured: 0.089 extracted, 0.107 clustered)."""
    v, f, q, h = probe
    if clustered:
        v, f = M.cluster_vertices(v, f, cell=h)[:2]
    dist, arg, at = M.point_to_mesh(q, v, f)
    vert = M.nearest(q, v)[0]
    surf, near = float(dist.astype(np.float64).mean()), float(vert.astype(np.float64).mean())
    print(f"SURFACE_MEASURED sphere probe clustered={clustered}: V={len(v)} T={len(f)} vertex {near:.5f} surface {surf:.5f} ratio {surf / near:.3f}")
    assert np.isfinite(dist).all() and (arg >= 0).all()
    assert surf < 0.2 * near
    assert (dist <= vert * (1 + 2.0 ** -20)).all()                          # the surface contains its vertices
    k = slice(0, 64)
    assert abs(D.cal_surface_error(q[k], v, f, 2.5) - 2.5 * float(dist[k].astype(np.float64).mean())) <= 1e-12
    assert abs(D.cal_geometric_error(q, v, 2.5) - 2.5 * near) <= 1e-12


def test_cal_surface_error_edge_cases():
    v, f, q = exact_cases()["duplicates"][:3]
    assert D.cal_surface_error(q, v, f, 2.0) == 1.0
    assert np.isnan(D.cal_surface_error(np.zeros((0, 3), np.float32), v, f))
    assert D.cal_surface_error(q, v, np.zeros((0, 3), np.int64)) == float("inf")


# ---- the library's argument checks (no GPU: every call must fail before it launches) -------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from endosurf_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_surface_entry_points_check_their_arguments(lib):
    assert lib.es_abi_version() == 14          # additive: the version does not move
    buf = np.zeros(256, np.float64)
    p = C.c_void_p(buf.ctypes.data // 16 * 16 + 16)          # (a host address: never dereferenced)
    odd = C.c_void_p(p.value + 4)

    def fails(status, word):
        assert status == 1 and word in lib.es_last_error(), (status, lib.es_last_error())

    assert lib.es_surf_scratch_bytes(10, 20) > 0 and lib.es_surf_scratch_bytes(0, 0) > 0
    assert lib.es_surf_scratch_bytes(10, 20) % 16 == 0
    assert lib.es_surf_scratch_bytes(10, 20) > lib.es_nn_scratch_bytes(20)
    assert lib.es_surf_scratch_bytes(-1, 2) == -1 and b"negative" in lib.es_last_error()
    assert lib.es_surf_scratch_bytes(1, -2) == -1 and b"negative" in lib.es_last_error()
    assert lib.es_surf_scratch_bytes(1 << 31, 2) == -1 and b"2^31" in lib.es_last_error()
    assert lib.es_surf_scratch_bytes(1, 1 << 31) == -1 and b"2^31" in lib.es_last_error()
    fails(lib.es_surf_build(None, p, 4, 2, p, None), b"verts")
    fails(lib.es_surf_build(p, None, 4, 2, p, None), b"tris")
    fails(lib.es_surf_build(p, p, 4, 2, None, None), b"scratch")
    fails(lib.es_surf_build(p, p, 4, 2, odd, None), b"aligned")
    fails(lib.es_surf_build(p, p, -4, 2, p, None), b"negative")
    fails(lib.es_surf_build(p, p, 4, -2, p, None), b"negative")
    fails(lib.es_surf_build(p, p, 1 << 31, 2, p, None), b"2^31")
    fails(lib.es_surf_build(p, p, 4, 1 << 31, p, None), b"2^31")
    fails(lib.es_surf_query(None, 3, p, p, 4, 2, p, p, p, p, None, None), b"query")
    fails(lib.es_surf_query(p, 3, None, p, 4, 2, p, p, p, p, None, None), b"verts")
    fails(lib.es_surf_query(p, 3, p, None, 4, 2, p, p, p, p, None, None), b"tris")
    fails(lib.es_surf_query(p, 3, p, p, 4, 2, None, p, p, p, None, None), b"scratch")
    fails(lib.es_surf_query(p, 3, p, p, 4, 2, odd, p, p, p, None, None), b"aligned")
    fails(lib.es_surf_query(p, 3, p, p, 4, 2, p, None, p, p, None, None), b"dist")
    fails(lib.es_surf_query(p, 3, p, p, 4, 2, p, p, None, p, None, None), b"triangle")
    fails(lib.es_surf_query(p, 3, p, p, 4, 2, p, p, p, None, None, None), b"closest")
    fails(lib.es_surf_query(p, -3, p, p, 4, 2, p, p, p, p, None, None), b"negative")
    fails(lib.es_surf_query(p, 1 << 31, p, p, 4, 2, p, p, p, p, None, None), b"2^31")
    fails(lib.es_surf_query(p, 3, p, p, 1 << 31, 2, p, p, p, p, None, None), b"2^31")
    fails(lib.es_surf_query(p, 3, p, p, 4, 1 << 31, p, p, p, p, None, None), b"2^31")
    assert lib.es_surf_query(None, 0, None, None, 0, 0, None, None, None, None, None, None) == 0          # Q == 0 writes nothing
