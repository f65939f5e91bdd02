"""The cube triangulation on the device (csrc/cubes.hip, Engine.iso_surface(method="cubes"), the ``method`` keyword of
EndoSurfRenderer.extract_observation_geometry / extract_observation_mesh / export_observation_mesh) against its numpy twin
endosurf_amd.meshing.marching_cubes: edge_ends and triangles equal as arrays, positions within 1 fp32 ulp."""
import ctypes as C

import numpy as np
import pytest
import torch

from cubes_util import compare_with_twin, edge_balance, euler_number
from iso_util import fields

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from endosurf_amd.engine import Engine
    return Engine("cuda")


def _mesh(eng, u, thr, method="cubes"):
    v, f, e = eng.iso_surface(torch.from_numpy(np.ascontiguousarray(u)).cuda(), thr, method)
    assert v.is_cuda and v.dtype == torch.float32 and f.dtype == torch.int32 and e.dtype == torch.int32
    assert v.shape == (e.shape[0], 3) and f.shape[1] == 3 and e.shape[1] == 2
    return v.cpu().numpy(), f.cpu().numpy(), e.cpu().numpy()


CASES = [("sphere", (64, 64, 64), 0.0), ("sphere", (33, 33, 33), 0.2), ("sphere", (33, 33, 33), -0.2), ("torus", (96, 96, 96), 0.0),
         ("two_spheres", (65, 65, 65), 0.0), ("gyroid", (96, 80, 72), 0.0), ("random", (70, 50, 90), 0.0), ("random", (17, 40, 9), 0.0),
         ("random", (9, 17, 130), 0.2), ("random", (2, 2, 2), 0.1), ("sphere", (2, 3, 2), 0.9), ("plane_on_grid", (20, 12, 70), 0.0),
         ("ties", (40, 40, 40), 0.5)]


@pytest.mark.parametrize("name,shape,thr", CASES)
def test_exact_against_the_twin(eng, name, shape, thr):
    u = fields(name, shape, seed=7)
    V, T = compare_with_twin(u, thr, *_mesh(eng, u, thr))
    assert V > 0 and T > 0


def test_nan_patch_and_infinities(eng):
    u = fields("random", (40, 36, 44), seed=11)
    u[10:14, 8:20, 30:33] = np.nan          # NaN is outside; the vertices next to it are NaN on the host as well
    u[30, 30, 5] = np.inf
    u[5, 5, 40] = -np.inf
    V, T = compare_with_twin(u, 0.0, *_mesh(eng, u, 0.0))
    assert V > 0 and T > 0


def test_vertices_are_the_tetrahedra_extractor_s(eng):
    """The cube vertices are, bit for bit, the vertices Engine.iso_surface's default method puts on the same grid edges."""
    u = fields("gyroid", (70, 61, 67))
    cv, _, ce = _mesh(eng, u, 0.1)
    tv, _, te = _mesh(eng, u, 0.1, "tetrahedra")
    ck, tk = ce[:, 0].astype(np.int64) * u.size + ce[:, 1], te[:, 0].astype(np.int64) * u.size + te[:, 1]
    order = np.argsort(tk)
    pos = np.searchsorted(tk[order], ck)
    assert np.array_equal(tk[order][pos], ck)
    assert np.array_equal(cv.view(np.uint32), tv[order][pos].view(np.uint32))
    assert 0.28 * len(tv) < len(cv) < 0.40 * len(tv)


@pytest.mark.parametrize("name,euler", [("sphere", 2), ("torus", 0)])
def test_topology_of_the_device_mesh_alone(eng, name, euler):
    u = fields(name, (80, 80, 80))
    v, f, e = _mesh(eng, u, 0.0)
    assert f.min() >= 0 and f.max() < len(v)
    assert ((f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])).all()
    uses, balance = edge_balance(f)
    assert (uses == 2).all() and (balance == 0).all()          # closed surface inside the grid: watertight, consistently oriented
    assert euler_number(v, f) == euler
    # vertex order: ascending (owner = the smaller end, direction)
    owner = e.min(axis=1).astype(np.int64)
    assert (np.diff(owner * (2 * u.size) + (e.max(axis=1) - owner)) > 0).all()
    # oriented towards increasing u: outward for these two
    p0, p1, p2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    n = np.cross(p1 - p0, p2 - p0).astype(np.float64)
    c = (p0 + p1 + p2) / 3 - 39.5
    if name == "sphere":
        assert (np.einsum("ij,ij->i", n, c) > 0).all()
        area = 0.5 * np.linalg.norm(n, axis=1).sum() * (2 / 79) ** 2
        assert abs(area - 4 * np.pi * 0.36) < 0.01 * 4 * np.pi * 0.36
    else:
        assert np.einsum("ij,ij->i", p0 - 39.5, np.cross(p1 - 39.5, p2 - 39.5)).sum() > 0          # positive signed volume


def test_empty_fields_and_bad_arguments(eng):
    u = fields("sphere", (12, 12, 12))
    for thr in (-5.0, 5.0, float("nan")):          # all outside, all inside, a threshold nothing is below
        v, f, e = _mesh(eng, u, thr)
        assert v.shape == (0, 3) and f.shape == (0, 3) and e.shape == (0, 2)
    lib = eng.lib
    dummy = torch.zeros(64, device="cuda")
    p = C.c_void_p(dummy.data_ptr())
    assert lib.es_cubes_count(None, 4, 4, 4, 0.0, p, p, None) == 1 and b"field" in lib.es_last_error()
    assert lib.es_cubes_count(p, 4, 1, 4, 0.0, p, p, None) == 1 and b"at least 2" in lib.es_last_error()
    assert lib.es_cubes_count(p, 2048, 1024, 1024, 0.0, p, p, None) == 1 and b"2^31" in lib.es_last_error()          # argument check only
    assert lib.es_cubes_emit(p, 2048, 1024, 1024, 0.0, p, 1, 1, p, p, p, None) == 1
    assert lib.es_cubes_emit(p, 4, 4, 4, 0.0, p, 1 << 31, 0, p, p, p, None) == 1 and b"int32" in lib.es_last_error()
    assert lib.es_cubes_emit(p, 4, 4, 4, 0.0, p, 1, 1, None, p, p, None) == 1
    assert lib.es_cubes_scratch_bytes(1, 8, 8) == -1 and lib.es_cubes_scratch_bytes(2048, 1024, 1024) == -1
    assert lib.es_cubes_scratch_bytes(8, 8, 8) > 0
    with pytest.raises(Exception):
        eng.iso_surface(torch.zeros(4, 4, device="cuda"), 0.0, "cubes")
    with pytest.raises(Exception):
        eng.iso_surface(torch.zeros(4, 1, 4, device="cuda"), 0.0, "cubes")
    with pytest.raises(Exception):
        eng.iso_surface(torch.from_numpy(u).cuda(), 0.0, method="nope")
    with pytest.raises(Exception):
        eng.iso_surface_band(lambda x: x[:, 0], [torch.linspace(-1, 1, 9, device="cuda")] * 3, method="nope")


def test_bit_identical_scratch_contents_and_capacity(eng):
    u = torch.from_numpy(fields("gyroid", (70, 61, 67))).cuda()
    a = eng.iso_surface(u, 0.1, "cubes")
    b = eng.iso_surface(u, 0.1, "cubes")
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    # the C calls with a scratch buffer full of NaN bit patterns, then full of zeros
    lib, st = eng.lib, eng.st()
    nx, ny, nz = u.shape
    nbytes = lib.es_cubes_scratch_bytes(nx, ny, nz)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    V, T = a[0].shape[0], a[1].shape[0]
    for fill in (0xFF, 0x00):
        scratch = torch.full((nbytes,), fill, dtype=torch.uint8, device="cuda")
        totals = torch.full((2,), -7, dtype=torch.int64, device="cuda")
        assert lib.es_cubes_count(ptr(u), nx, ny, nz, 0.1, ptr(scratch), ptr(totals), st) == 0
        assert tuple(totals.tolist()) == (V, T)
        v = torch.full((V, 3), float("nan"), device="cuda")
        e = torch.full((V, 2), -1, dtype=torch.int32, device="cuda")
        f = torch.full((T, 3), -1, dtype=torch.int32, device="cuda")
        assert lib.es_cubes_emit(ptr(u), nx, ny, nz, 0.1, ptr(scratch), V, T, ptr(v), ptr(e), ptr(f), st) == 0
        assert all(torch.equal(x, y) for x, y in zip(a, (v, f, e)))
    # output buffers one vertex, or one triangle, short of the mesh: refused, and nothing is written -- not inside the stated capacity,
    # not in the word behind it
    v = torch.full((V * 3 + 1,), 7.0, device="cuda")
    e = torch.full((V * 2 + 1,), -1, dtype=torch.int32, device="cuda")
    f = torch.full((T * 3 + 1,), -1, dtype=torch.int32, device="cuda")
    assert lib.es_cubes_emit(ptr(u), nx, ny, nz, 0.1, ptr(scratch), V - 1, T, ptr(v), ptr(e), ptr(f), st) == 1
    assert b"capacity" in lib.es_last_error()
    assert lib.es_cubes_emit(ptr(u), nx, ny, nz, 0.1, ptr(scratch), V, T - 1, ptr(v), ptr(e), ptr(f), st) == 1
    torch.cuda.synchronize()
    assert bool((v == 7.0).all()) and bool((e == -1).all()) and bool((f == -1).all())
    # at the exact capacity the word behind each buffer stays what it was
    assert lib.es_cubes_emit(ptr(u), nx, ny, nz, 0.1, ptr(scratch), V, T, ptr(v), ptr(e), ptr(f), st) == 0
    assert torch.equal(v[:-1].view(V, 3), a[0]) and torch.equal(f[:-1].view(T, 3), a[1]) and torch.equal(e[:-1].view(V, 2), a[2])
    assert float(v[-1]) == 7.0 and int(e[-1]) == -1 and int(f[-1]) == -1


# ---- through the renderer --------------------------------------------------------------------------------------------------------------
BMIN, BMAX, VIEW = [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0], [0.1, -0.2, -1.5]
MESH_KEYS = ("vertices", "triangles", "normals", "sdf", "colors")


@pytest.fixture(scope="module")
def scene():
    from gpu_util import renderer_for_case
    from oracle_util import load_case
    return renderer_for_case(load_case("trained_deform")), torch.tensor([0.37])


def test_band_mesh_equals_the_dense_mesh(scene):
    r, t = scene
    R = 129
    dense = r.extract_observation_mesh(t, BMIN, BMAX, R, view_point=VIEW, method="cubes")
    band = r.extract_observation_mesh(t, BMIN, BMAX, R, view_point=VIEW, band=dict(block=8), method="cubes")
    assert set(dense) == set(MESH_KEYS) | {"method"} and set(band) == set(dense) | {"stats"}
    assert dense["method"] == band["method"] == "cubes" and dense["vertices"].shape[0] > 3000
    for k in MESH_KEYS:
        assert torch.equal(band[k], dense[k]), k
    assert not band["stats"]["fallback"] and band["stats"]["evaluated_points"] < 0.30 * R ** 3


def test_observation_mesh(scene, tmp_path):
    from endosurf_amd import data as D
    r, t = scene
    R = 65
    tet = r.extract_observation_mesh(t, BMIN, BMAX, R, view_point=VIEW, method="tetrahedra")
    m0 = r.extract_observation_mesh(t, BMIN, BMAX, R, view_point=VIEW, method="cubes")
    V, Vt = m0["vertices"].shape[0], tet["vertices"].shape[0]
    print(f"CUBES_MEASURED R={R} cubes V={V} T={m0['triangles'].shape[0]}, tetrahedra V={Vt} T={tet['triangles'].shape[0]}, ratio {V / Vt:.4f}")
    assert 0.28 * Vt < V < 0.40 * Vt
    assert "method" not in tet and m0["method"] == "cubes"
    assert m0["normals"].shape == (V, 3) and m0["colors"].shape == (V, 3) and m0["sdf"].shape == (V,)
    # the geometry call gives the same mesh; the host path has no cube extractor
    vg, fg = r.extract_observation_geometry(t, BMIN, BMAX, R, cpu=False, on_device=True, method="cubes")
    assert torch.equal(vg, m0["vertices"]) and torch.equal(fg, m0["triangles"])
    with pytest.raises(ValueError):
        r.extract_observation_geometry(t, BMIN, BMAX, R, method="cubes")
    with pytest.raises(ValueError):
        r.extract_observation_mesh(t, BMIN, BMAX, R, method="nope")
    # one Newton step pulls the vertices onto the level set
    m1 = r.extract_observation_mesh(t, BMIN, BMAX, R, view_point=VIEW, refine_steps=1, method="cubes")
    med0, med1 = float(m0["sdf"].abs().median()), float(m1["sdf"].abs().median())
    print(f"CUBES_MEASURED median|sdf| {med0:.3e} -> {med1:.3e}")
    assert torch.equal(m1["triangles"], m0["triangles"]) and med1 < med0
    # the later stages run unchanged on the smaller mesh
    s = r.extract_observation_mesh(t, BMIN, BMAX, R, view_point=VIEW, components=0.9, clean=True, simplify="grid", method="cubes")
    assert set(s) == set(MESH_KEYS) | {"method", "components", "clean", "simplify"}
    assert 0 < s["triangles"].shape[0] == s["simplify"]["kept_triangles"] < m0["triangles"].shape[0]
    assert s["vertices"].shape[0] == s["simplify"]["cells"] and int(s["triangles"].max()) < s["vertices"].shape[0]
    # the three files, read back
    x = r.export_observation_mesh(str(tmp_path / "cubes"), t, BMIN, BMAX, R, view_point=VIEW, method="cubes")
    v, f = x["vertices"].cpu().numpy(), x["triangles"].cpu().numpy()
    assert x["method"] == "cubes" and 0 < len(v) <= V
    for k in ("geometry", "color", "normal"):
        got = D.read_ply(x["paths"][k])
        assert got["vertices"].shape == v.shape and got["triangles"].shape == f.shape
        assert np.array_equal(got["vertices"], v) and np.array_equal(got["triangles"], f)


def test_the_default_is_the_tetrahedra_method(eng, scene):
    """Nothing existing changed: no ``method`` is ``method="tetrahedra"``, bit for bit."""
    u = torch.from_numpy(fields("gyroid", (48, 40, 56))).cuda()
    for x, y in zip(eng.iso_surface(u, 0.1), eng.iso_surface(u, 0.1, method="tetrahedra")):
        assert torch.equal(x, y)
    assert eng.iso_surface(u, 0.1)[0].shape[0] > eng.iso_surface(u, 0.1, "cubes")[0].shape[0] > 0
    r, t = scene
    a = r.extract_observation_mesh(t, BMIN, BMAX, 48, view_point=VIEW)
    b = r.extract_observation_mesh(t, BMIN, BMAX, 48, view_point=VIEW, method="tetrahedra")
    assert set(a) == set(b) == set(MESH_KEYS)
    for k in MESH_KEYS:
        assert torch.equal(a[k], b[k]), k
    va, fa = r.extract_observation_geometry(t, BMIN, BMAX, 48, cpu=False, on_device=True)
    assert torch.equal(va, a["vertices"]) and torch.equal(fa, a["triangles"])
