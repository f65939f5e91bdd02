"""Mesh clean-up and geometric error on the device (csrc/mesh.hip: Engine.mesh_components / keep_components / nearest, the
``components`` keyword of EndoSurfRenderer.extract_observation_mesh / extract_observation_geometry, EndoSurfRenderer.geometric_error)
against the numpy twins in endosurf_amd.meshing, which tests/test_mesh_host.py checks against independent formulations."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from endosurf_amd import data as D
from endosurf_amd import meshing as M
from iso_util import fields
from mesh_util import FIELD_CASES, field, hand_meshes, mt_mesh, nearest64, strip

pytestmark = pytest.mark.gpu

HAND = hand_meshes()


@pytest.fixture(scope="module")
def eng():
    from endosurf_amd.engine import Engine
    return Engine("cuda")


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def same(t, a):
    a = np.asarray(a)
    return tuple(t.shape) == a.shape and np.array_equal(t.cpu().numpy(), a)


def check_against_twin(eng, v, f, ratios=(0.9,)):
    """Engine.mesh_components and keep_components (both forms) of a device mesh equal the twins exactly; returns the stats."""
    vn, fn = v.cpu().numpy(), f.cpu().numpy()
    vl, tl, ct, st = eng.mesh_components(f, v.shape[0])
    evl, etl, ect = M.mesh_components(fn, len(vn))
    assert vl.dtype == tl.dtype == ct.dtype == torch.int32
    assert same(vl, evl) and same(tl, etl) and same(ct, ect)
    assert st["components"] == int((ect > 0).sum()) and st["max_triangles"] == (int(ect.max()) if len(ect) else 0)
    assert st["degenerate"] == int((etl < 0).sum()) and st["kept_triangles"] == len(fn) - st["degenerate"] and st["rounds"] >= 1
    for ratio in ratios:
        for compact in (True, False):
            kv, kf, vmap, kst = eng.keep_components(v, f, ratio, compact)
            ev, ef, emap, est = M.keep_components(vn, fn, ratio, compact)
            assert kv.dtype == torch.float32 and kf.dtype == torch.int32 and vmap.dtype == torch.int64
            assert same(kv, ev) and same(kf, ef) and same(vmap, emap), (ratio, compact)
            assert {k: kst[k] for k in kst if k != "rounds"} == {k: est[k] for k in est if k != "rounds"}
    return st


@pytest.mark.parametrize("name", list(HAND))
def test_hand_made_meshes_equal_the_twin(eng, name):
    v, f = HAND[name]
    check_against_twin(eng, dev(v), dev(f), ratios=(0.9, 0.8, 0.0, 1.0))
    check_against_twin(eng, dev(v), dev(f, torch.int32))


@pytest.mark.parametrize("name,shape,thr", FIELD_CASES)
def test_host_extracted_meshes_equal_the_twin(eng, name, shape, thr):
    v, f = mt_mesh(name, shape, thr)
    st = check_against_twin(eng, dev(v), dev(f), ratios=(0.9, 0.3))
    assert st["components"] >= 1


ISO_CASES = [("sphere", (40, 40, 40), 0.0), ("torus", (48, 52, 44), 0.0), ("two_spheres", (65, 65, 65), 0.0), ("gyroid", (70, 61, 67), 0.1),
             ("random", (64, 64, 64), 0.2), ("random", (50, 81, 33), -0.4), ("ties", (40, 36, 44), 0.5), ("plane_on_grid", (20, 24, 28), 0.0),
             ("two_disjoint_spheres", (80, 80, 80), 0.0), ("sphere_and_floaters", (97, 97, 97), 0.0), ("sphere_and_floaters", (60, 50, 40), 0.02),
             ("random", (129, 129, 129), 0.9), ("sphere", (257, 257, 257), 0.0)]


@pytest.mark.parametrize("name,shape,thr", ISO_CASES)
def test_device_extracted_meshes_equal_the_twin(eng, name, shape, thr):
    u = dev(fields("random", shape, seed=shape[1]) if name == "random" else field(name, shape))
    v, f, _ = eng.iso_surface(u, thr)
    assert f.shape[0] > 100
    st = check_against_twin(eng, v, f)
    if name == "sphere_and_floaters":
        assert st["components"] == 4
        kv, kf, vmap, kst = eng.keep_components(v, f)
        assert kst["kept_triangles"] == st["max_triangles"] < f.shape[0]
    print(f"MESH_MEASURED {name} {shape}: V={v.shape[0]} T={f.shape[0]} {st}")


def test_a_planted_floater_goes_and_attributes_follow(eng):
    u = dev(field("sphere", (64, 64, 64)))
    v, f, _ = eng.iso_surface(u, 0.0)
    tiny_v, tiny_f, _ = eng.iso_surface(dev(field("sphere", (9, 9, 9))), 0.0)
    V = v.shape[0]
    both_v = torch.cat([tiny_v * 0.2 + 70.0, v])          # the floater first: the big piece's label is not 0
    both_f = torch.cat([tiny_f, f + tiny_v.shape[0]])
    kv, kf, vmap, st = eng.keep_components(both_v, both_f)
    assert st["components"] == 2 and st["kept_triangles"] == f.shape[0] and torch.equal(kv, v) and torch.equal(kf, f)
    assert torch.equal(vmap, torch.arange(tiny_v.shape[0], tiny_v.shape[0] + V, device="cuda"))
    colors = torch.rand(both_v.shape[0], 3, device="cuda")
    assert torch.equal(colors.index_select(0, vmap)[kf.long()], colors[both_f[tiny_f.shape[0]:].long()])
    kv2, kf2, vmap2, st2 = eng.keep_components(both_v, both_f, compact=False)
    assert torch.equal(kv2, both_v) and torch.equal(kf2, both_f[tiny_f.shape[0]:]) and vmap2.shape[0] == both_v.shape[0]


def test_rounds_stay_logarithmic(eng):
    """Hook-and-jump, not label propagation: a 513 x 513 sheet has a graph diameter of ~1000 and the strips of ~10 000."""
    x = np.broadcast_to(np.arange(3, dtype=np.float32)[None, None, :] - 0.5, (513, 513, 3)).copy()
    v, f, _ = eng.iso_surface(dev(x), 0.0)
    assert f.shape[0] >= 2 * 512 * 512 and v.shape[0] > 512 * 512
    cases = [("sheet", f, v.shape[0]), ("strip", dev(strip(10000)), 20002), ("strip_shuffled", dev(strip(10000, seed=5)), 20002),
             ("sheet_shuffled", torch.randperm(v.shape[0], device="cuda", generator=torch.Generator("cuda").manual_seed(1))[f.long()], v.shape[0])]
    for name, tris, V in cases:
        vl, tl, ct, st = eng.mesh_components(tris, V)
        bound = 2 * math.ceil(math.log2(V)) + 4
        print(f"MESH_MEASURED rounds {name}: V={V} T={tris.shape[0]} rounds={st['rounds']} (bound {bound})")
        assert st["components"] == 1 and st["max_triangles"] == tris.shape[0] and int(vl.max()) == 0
        assert st["rounds"] <= bound, (name, st)


def test_bit_identical_and_independent_of_scratch_contents(eng):
    u = dev(field("sphere_and_floaters", (70, 61, 67)))
    v, f, _ = eng.iso_surface(u, 0.01)
    a, b = eng.keep_components(v, f), eng.keep_components(v, f)
    assert all(torch.equal(x, y) for x, y in zip(a[:3], b[:3]))
    la, lb = eng.mesh_components(f, v.shape[0]), eng.mesh_components(f, v.shape[0])
    assert all(torch.equal(x, y) for x, y in zip(la[:3], lb[:3]))
    q = torch.rand(5000, 3, device="cuda") * 70
    na, nb = eng.nearest(q, v), eng.nearest(q, v)
    assert torch.equal(na[0], nb[0]) and torch.equal(na[1], nb[1])
    # the C calls with scratch buffers of 0xFF bytes, then of zeros
    lib, st = eng.lib, eng.st()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    V, T = v.shape[0], f.shape[0]
    for fill in (0xFF, 0x00):
        scratch = torch.full((lib.es_mesh_scratch_bytes(V, T),), fill, dtype=torch.uint8, device="cuda")
        changed = torch.full((1,), -3, dtype=torch.int32, device="cuda")
        totals = torch.full((3,), -7, dtype=torch.int64, device="cuda")
        vl, tl, ct = (torch.full((n,), -9, dtype=torch.int32, device="cuda") for n in (V, T, V))
        assert lib.es_mesh_cc_begin(ptr(f), V, T, ptr(scratch), st) == 0
        for _ in range(64):
            assert lib.es_mesh_cc_round(ptr(f), V, T, ptr(scratch), ptr(changed), st) == 0
            if int(changed.item()) == 0:
                break
        assert int(changed.item()) == 0
        assert lib.es_mesh_cc_finish(ptr(f), V, T, ptr(scratch), ptr(vl), ptr(tl), ptr(ct), ptr(totals), st) == 0
        assert torch.equal(vl, la[0]) and torch.equal(tl, la[1]) and torch.equal(ct, la[2])
        ncomp, biggest, ndeg = totals.tolist()
        assert (ncomp, biggest, ndeg) == (la[3]["components"], la[3]["max_triangles"], la[3]["degenerate"])
        for compact in (1, 0):
            kt = torch.full((2,), -7, dtype=torch.int64, device="cuda")
            assert lib.es_mesh_keep_count(ptr(f), V, T, ptr(tl), ptr(ct), 0.9, biggest, compact, ptr(scratch), ptr(kt), st) == 0
            V2, T2 = kt.tolist()
            ref = a if compact else eng.keep_components(v, f, 0.9, False)
            assert (V2, T2) == (ref[0].shape[0], ref[1].shape[0])
            # capacity one short of the result: nothing is written beyond it
            ov = torch.full((V2, 3), float("nan"), device="cuda")
            of = torch.full((T2, 3), -5, dtype=torch.int32, device="cuda")
            om = torch.full((V2,), -5, dtype=torch.int64, device="cuda")
            assert lib.es_mesh_keep_emit(ptr(v), ptr(f), V, T, ptr(scratch), V2 - 1, T2 - 1, ptr(ov), ptr(of), ptr(om), st) == 0
            assert torch.equal(ov[:-1], ref[0][:-1]) and torch.equal(of[:-1], ref[1][:-1]) and torch.equal(om[:-1], ref[2][:-1])
            assert bool(ov[-1].isnan().all()) and bool((of[-1] == -5).all()) and int(om[-1]) == -5
            assert lib.es_mesh_keep_emit(ptr(v), ptr(f), V, T, ptr(scratch), V2, T2, ptr(ov), ptr(of), ptr(om), st) == 0
            assert torch.equal(ov, ref[0]) and torch.equal(of, ref[1]) and torch.equal(om, ref[2])
        # nearest: a scratch that was never built answers inf / -1; a built one the twin's answer, whatever it held before
        nscr = torch.full((lib.es_nn_scratch_bytes(V),), fill, dtype=torch.uint8, device="cuda")
        dist = torch.full((q.shape[0],), -1.0, device="cuda")
        idx = torch.full((q.shape[0],), -9, dtype=torch.int32, device="cuda")
        assert lib.es_nn_query(ptr(q), q.shape[0], V, ptr(nscr), ptr(dist), ptr(idx), st) == 0
        assert bool(dist.isinf().all()) and bool((idx == -1).all())
        assert lib.es_nn_build(ptr(v), V, ptr(nscr), st) == 0
        assert lib.es_nn_query(ptr(q), q.shape[0], V, ptr(nscr), ptr(dist), ptr(idx), st) == 0
        assert torch.equal(dist, na[0]) and torch.equal(idx, na[1])


# ---- nearest ------------------------------------------------------------------------------------------------------------------------
def check_nearest(eng, q, p, twin=True):
    """Engine.nearest against the fp64 brute force (distance to 1e-6, index wherever fp64 can tell) and against the twin."""
    qn, pn = np.ascontiguousarray(q, np.float32), np.ascontiguousarray(p, np.float32)
    dist, idx = eng.nearest(dev(qn).reshape(-1, 3), dev(pn).reshape(-1, 3))
    assert dist.dtype == torch.float32 and idx.dtype == torch.int32 and dist.shape == idx.shape == (len(qn),)
    dist, idx = dist.cpu().numpy(), idx.cpu().numpy()
    d64, i64, gap = nearest64(qn, pn)
    none = i64 < 0
    assert (idx[none] == -1).all() and np.isinf(dist[none]).all()
    ok = ~none
    assert (idx[ok] >= 0).all() and np.allclose(dist[ok], d64[ok], rtol=1e-6, atol=1e-30)
    clear = ok & (gap > 1e-6)
    assert np.array_equal(idx[clear], i64[clear])
    pd = np.linalg.norm(qn.astype(np.float64)[ok] - pn.astype(np.float64)[idx[ok]], axis=1)
    assert np.allclose(pd, d64[ok], rtol=2e-6, atol=1e-30)
    if twin:          # the numpy twin: the same point wherever fp64 can tell, the same distance to an ulp of fp32
        td, ti = M.nearest(qn, pn)
        assert np.array_equal(ti[clear], idx[clear]) and np.array_equal(ti < 0, idx < 0)
        assert np.allclose(td[ok], dist[ok], rtol=2.5e-7, atol=1e-30)
    return dist, idx


@pytest.mark.parametrize("P,Q", [(1, 100), (2, 100), (3, 64), (17, 1000), (1000, 4096), (30000, 4096), (200000, 1024)])
def test_nearest_on_random_clouds(eng, P, Q):
    rng = np.random.default_rng(P)
    p = (rng.normal(size=(P, 3)) * [1.0, 0.6, 0.3] + [0.2, -0.1, 3.0]).astype(np.float32)
    q = np.concatenate([rng.normal(size=(Q // 2, 3)) * [1.0, 0.6, 0.3] + [0.2, -0.1, 3.0], rng.uniform(-4, 6, size=(Q - Q // 2, 3))])
    check_nearest(eng, q, p)


def test_nearest_on_a_surface_cloud(eng):
    """The product shape: mesh vertices (a 2-D sheet in the box) against points near them, pixel-ordered."""
    v, _, _ = eng.iso_surface(dev(field("sphere_and_floaters", (97, 97, 97))), 0.0)
    vn = v.cpu().numpy()
    rng = np.random.default_rng(0)
    q = vn[rng.integers(0, len(vn), 6000)] + rng.normal(size=(6000, 3)).astype(np.float32) * 0.7
    check_nearest(eng, q, vn)


def test_nearest_degenerate_clouds_and_queries(eng):
    rng = np.random.default_rng(7)
    q = rng.uniform(-2, 2, size=(1500, 3)).astype(np.float32)
    plane = rng.uniform(-1, 1, size=(5000, 3)).astype(np.float32)
    plane[:, 1] = 0.25
    check_nearest(eng, q, plane)                                            # all points on one plane
    line = np.zeros((3000, 3), np.float32)
    line[:, 2] = rng.uniform(-1, 1, size=3000)
    check_nearest(eng, q, line)                                             # on one line
    d, i = check_nearest(eng, q, np.tile(np.array([[0.3, -0.2, 0.1]], np.float32), (1000, 1)))
    assert (i == 0).all()                                                   # all points identical: the smallest index
    cloud = rng.uniform(-1, 1, size=(20000, 3)).astype(np.float32)
    far = (rng.normal(size=(256, 3)) * 50 + [300, -200, 100]).astype(np.float32)
    check_nearest(eng, far, cloud)                                          # queries far outside the box: a scan, not a hang
    on = cloud[rng.integers(0, len(cloud), 2000)]
    d, i = check_nearest(eng, on, cloud)
    assert (d == 0).all()                                                   # queries exactly on points
    lattice = np.stack(np.meshgrid(*[np.arange(12, dtype=np.float32)] * 3, indexing="ij"), -1).reshape(-1, 3)
    centres = lattice[rng.integers(0, len(lattice), 1500)] + 0.5            # 8 corners at the same distance (inside the lattice)
    d, i = check_nearest(eng, centres, np.concatenate([lattice, lattice]))
    assert (i < len(lattice)).all()                                         # exact ties: the smallest index, never the duplicate


def test_nearest_nan_rows_and_empty_inputs(eng):
    rng = np.random.default_rng(9)
    p = rng.normal(size=(4000, 3)).astype(np.float32)
    p[::7, 0] = np.nan
    p[3::11, 2] = np.inf
    q = rng.normal(size=(1000, 3)).astype(np.float32)
    q[::13, 1] = np.nan
    q[5::17, 0] = -np.inf
    d, i = check_nearest(eng, q, p)
    assert (i[::13] == -1).all() and np.isinf(d[5::17]).all() and np.isfinite(p[i[i >= 0]]).all()
    d, i = check_nearest(eng, q, np.full((50, 3), np.nan, np.float32))
    assert (i == -1).all()
    d, i = eng.nearest(dev(q), torch.zeros(0, 3, device="cuda"))                         # P == 0
    assert d.shape == (1000,) and bool(d.isinf().all()) and bool((i == -1).all())
    d, i = eng.nearest(torch.zeros(0, 3, device="cuda"), dev(p))                         # Q == 0
    assert d.shape == (0,) and i.shape == (0,) and d.dtype == torch.float32 and i.dtype == torch.int32


def test_argument_errors(eng):
    from endosurf_amd._lib import EndoSurfHipError
    v = torch.zeros(5, 3, device="cuda")
    f = torch.tensor([[0, 1, 2], [2, 3, 4]], device="cuda")
    with pytest.raises(EndoSurfHipError, match="outside"):
        eng.mesh_components(torch.tensor([[0, 1, 5]], device="cuda"), 5)
    with pytest.raises(EndoSurfHipError, match="outside"):
        eng.keep_components(v, torch.tensor([[0, -1, 2]], device="cuda"))
    with pytest.raises(EndoSurfHipError, match="keep_ratio"):
        eng.keep_components(v, f, keep_ratio=1.5)
    with pytest.raises(EndoSurfHipError, match="keep_ratio"):
        eng.keep_components(v, f, keep_ratio=float("nan"))
    with pytest.raises(EndoSurfHipError):
        eng.keep_components(v.cpu(), f)
    with pytest.raises(EndoSurfHipError):
        eng.mesh_components(f.float(), 5)
    with pytest.raises(EndoSurfHipError):
        eng.mesh_components(f.reshape(-1), 5)
    with pytest.raises(EndoSurfHipError):
        eng.nearest(v, torch.zeros(4, 2, device="cuda"))
    with pytest.raises(EndoSurfHipError):
        eng.nearest(v.cpu(), v)
    lib = eng.lib
    dummy = torch.zeros(4096, device="cuda")
    p = C.c_void_p(dummy.data_ptr())
    assert lib.es_mesh_scratch_bytes(10, 10) > 0 and lib.es_mesh_scratch_bytes(-1, 10) == -1 and b"negative" in lib.es_last_error()
    assert lib.es_mesh_scratch_bytes(1 << 31, 10) == -1 and b"2^31" in lib.es_last_error()
    assert lib.es_nn_scratch_bytes(0) > 0 and lib.es_nn_scratch_bytes(1 << 31) == -1 and b"2^31" in lib.es_last_error()
    assert lib.es_mesh_cc_begin(None, 4, 2, p, None) == 1 and b"tris" in lib.es_last_error()
    assert lib.es_mesh_cc_begin(p, 4, 2, None, None) == 1 and b"scratch" in lib.es_last_error()
    assert lib.es_mesh_cc_begin(p, 4, 2, C.c_void_p(dummy.data_ptr() + 4), None) == 1 and b"aligned" in lib.es_last_error()
    assert lib.es_mesh_cc_round(p, 4, 2, p, None, None) == 1 and b"changed" in lib.es_last_error()
    assert lib.es_mesh_cc_round(p, 4, -2, p, p, None) == 1 and b"negative" in lib.es_last_error()
    assert lib.es_mesh_cc_finish(p, 4, 2, p, None, p, p, p, None) == 1 and b"vertex_label" in lib.es_last_error()
    assert lib.es_mesh_keep_count(p, 4, 2, p, p, 1.5, 2, 1, p, p, None) == 1 and b"keep_ratio" in lib.es_last_error()
    assert lib.es_mesh_keep_count(p, 4, 2, p, p, float("nan"), 2, 1, p, p, None) == 1 and b"keep_ratio" in lib.es_last_error()
    assert lib.es_mesh_keep_count(p, 4, 2, p, p, 0.9, 3, 1, p, p, None) == 1 and b"max_triangles" in lib.es_last_error()
    assert lib.es_mesh_keep_emit(p, p, 4, 2, p, 5, 2, p, p, p, None) == 1 and b"kept counts" in lib.es_last_error()
    assert lib.es_mesh_keep_emit(p, p, 4, 2, p, 4, 2, p, None, p, None) == 1 and b"tris_out" in lib.es_last_error()
    assert lib.es_nn_build(None, 4, p, None) == 1 and b"points" in lib.es_last_error()
    assert lib.es_nn_build(p, -4, p, None) == 1 and b"negative" in lib.es_last_error()
    assert lib.es_nn_query(p, 4, 4, p, None, p, None) == 1 and b"dist" in lib.es_last_error()
    assert lib.es_nn_query(None, 0, 4, None, None, None, None) == 0                     # Q == 0: nothing to do


# ---- through the renderer, on the trained goldens ------------------------------------------------------------------------------------
BMIN, BMAX, VIEW = [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0], [0.1, -0.2, -1.5]
MESH_KEYS = ("vertices", "triangles", "normals", "sdf", "colors")


@pytest.fixture(scope="module")
def scene():
    from gpu_util import renderer_for_case
    from oracle_util import load_case
    return renderer_for_case(load_case("trained_deform")), torch.tensor([0.37])


@pytest.mark.parametrize("thr", [0.0, 0.05])
def test_observation_mesh_with_components(scene, thr):
    r, t = scene
    R = 129
    full = r.extract_observation_mesh(t, BMIN, BMAX, R, threshold=thr, view_point=VIEW)
    kept = r.extract_observation_mesh(t, BMIN, BMAX, R, threshold=thr, view_point=VIEW, components=0.9)
    assert set(full) == set(MESH_KEYS) and set(kept) == set(MESH_KEYS) | {"components"}
    kv, kf, vmap, st = r.engine.keep_components(full["vertices"], full["triangles"], 0.9)
    assert torch.equal(kept["vertices"], kv) and torch.equal(kept["triangles"], kf)
    assert {k: v for k, v in kept["components"].items() if k != "rounds"} == {k: v for k, v in st.items() if k != "rounds"}
    assert st["components"] >= 1 and st["kept_triangles"] >= st["max_triangles"] > 1000
    print(f"MESH_MEASURED trained R={R} thr={thr}: V={full['vertices'].shape[0]} T={full['triangles'].shape[0]} {kept['components']}")
    # attributes computed on the kept vertices only = the unfiltered attributes moved along by vertex_map
    for k in ("normals", "sdf", "colors"):
        assert torch.allclose(kept[k], full[k].index_select(0, vmap), rtol=1e-4, atol=1e-5), k
    for spelling in (True, dict(keep_ratio=0.9), dict(keep_ratio=0.9, compact=True)):
        again = r.extract_observation_mesh(t, BMIN, BMAX, R, threshold=thr, components=spelling)
        assert torch.equal(again["vertices"], kv) and torch.equal(again["triangles"], kf)
    loose = r.extract_observation_mesh(t, BMIN, BMAX, R, threshold=thr, components=dict(keep_ratio=0.9, compact=False))
    assert torch.equal(loose["vertices"], full["vertices"]) and loose["triangles"].shape == kf.shape
    assert torch.equal(loose["vertices"][loose["triangles"].long()], kv[kf.long()])
    vg, fg = r.extract_observation_geometry(t, BMIN, BMAX, R, threshold=thr, cpu=False, on_device=True, components=0.9)
    assert torch.equal(vg, kv) and torch.equal(fg, kf)
    vn, fn = r.extract_observation_geometry(t, BMIN, BMAX, R, threshold=thr, on_device=True, components=True)
    assert isinstance(vn, np.ndarray) and np.array_equal(vn, kv.cpu().numpy()) and np.array_equal(fn, kf.cpu().numpy())


def test_without_components_nothing_changed(scene):
    r, t = scene
    R = 96
    v, f = r._mesh_on_device(t, BMIN, BMAX, R, 0.0, 1 << 22)
    for kw in (dict(), dict(components=None), dict(components=False)):
        m = r.extract_observation_mesh(t, BMIN, BMAX, R, **kw)
        assert set(m) == {"vertices", "triangles", "normals", "sdf"} and torch.equal(m["vertices"], v) and torch.equal(m["triangles"], f)
        vg, fg = r.extract_observation_geometry(t, BMIN, BMAX, R, cpu=False, on_device=True, **kw)
        assert torch.equal(vg, v) and torch.equal(fg, f)
    with pytest.raises(ValueError):
        r.extract_observation_geometry(t, BMIN, BMAX, R, components=0.9)          # the host path has no filter
    with pytest.raises(TypeError):
        r.extract_observation_mesh(t, BMIN, BMAX, R, components=dict(ratio=0.9))
    e = r.extract_observation_mesh(t, BMIN, BMAX, 65, threshold=50.0, view_point=VIEW, components=0.9)          # an empty level set
    assert e["vertices"].shape == (0, 3) and e["triangles"].shape == (0, 3) and e["components"]["components"] == 0


def test_band_and_filter_close_the_limit_of_the_band(scene):
    """with lipschitz = 0 the band can lose closed floaters smaller than a block -- which the filter removes anyway."""
    r, t = scene
    R = 129
    dense = r.extract_observation_mesh(t, BMIN, BMAX, R, view_point=VIEW, components=0.9)
    band = r.extract_observation_mesh(t, BMIN, BMAX, R, view_point=VIEW, components=0.9, band=dict(lipschitz=0.0))
    assert set(band) == set(MESH_KEYS) | {"components", "stats"}
    for k in MESH_KEYS:
        assert torch.equal(band[k], dense[k]), k
    assert band["components"]["kept_triangles"] == dense["components"]["kept_triangles"] > 1000


def test_geometric_error_of_a_rendered_depth_map(scene):
    r, t = scene
    h, w = 40, 48
    K = torch.tensor([[60.0, 0, 23.5, 0], [0, 60.0, 19.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    pose = torch.eye(4)
    pose[:3, 3] = torch.tensor([0.0, 0.0, -1.5])
    rays = D.assemble_rays(D.get_rays(K[None].cuda(), pose[None].cuda(), w, h), torch.zeros(1, 2, device="cuda"))
    rays[..., 8] = float(t)
    out = r.render_frames(rays, iter_step=1, ray_chunk=512, perturb_overwrite=False, use_graph=False)
    depth = out["depth"].reshape(h, w)
    trunc = float(depth.median())          # drops about half of the pixels
    mesh = r.extract_observation_mesh(t, BMIN, BMAX, 97, components=0.9)
    got = r.geometric_error(mesh, depth, K, pose, trunc, depth_scale=2.5)
    pts = D.depth_points(depth, K, pose, trunc)
    assert pts.is_cuda and 0 < pts.shape[0] < h * w
    assert torch.allclose(pts.cpu(), D.depth_points(depth.cpu(), K, pose, trunc), rtol=1e-5, atol=1e-6)
    td, ti = M.nearest(pts.cpu().numpy(), mesh["vertices"].cpu().numpy())
    want = float(td.astype(np.float64).mean()) * 2.5
    assert math.isfinite(got) and abs(got - want) <= 1e-6 * want
    assert abs(r.geometric_error(mesh["vertices"], depth.cpu().numpy(), K, pose, trunc, 2.5) - want) <= 1e-6 * want
    assert abs(D.cal_geometric_error(pts, mesh["vertices"], 2.5) - want) <= 1e-6 * want
    assert abs(D.cal_geometric_error(pts.cpu(), mesh["vertices"].cpu(), 2.5) - want) <= 1e-6 * want
    print(f"MESH_MEASURED geometric error: {pts.shape[0]} points against {mesh['vertices'].shape[0]} vertices = {got:.6f}")
