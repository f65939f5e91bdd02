"""Narrow-band mesh extraction on the device (csrc/band.hip, Engine.band_field / iso_surface_band, the ``band`` keyword of
EndoSurfRenderer.extract_observation_mesh / extract_observation_geometry) against the host twin endosurf_amd.meshing.band_field and
against the dense path, whose mesh it must reproduce bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_band_host import lookup

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from endosurf_amd.engine import Engine
    return Engine("cuda")


# ---- analytic samplers (separate element-wise launches: a point's value does not depend on the batch it arrives in) --------------------
def _r(x, c=(0.0, 0.0, 0.0)):
    return torch.sqrt((x[:, 0] - c[0]) ** 2 + (x[:, 1] - c[1]) ** 2 + (x[:, 2] - c[2]) ** 2)


def sphere(x):
    return _r(x) - 0.6


def steep_sphere(x):          # |grad| = 4: the default lipschitz bound is violated
    return 4.0 * (_r(x) - 0.6)


def torus(x):
    return torch.sqrt((torch.sqrt(x[:, 0] ** 2 + x[:, 1] ** 2) - 0.55) ** 2 + x[:, 2] ** 2) - 0.25


def gyroid(x):
    k = 2.5 * np.pi
    a, b, c = k * x[:, 0], k * x[:, 1], k * x[:, 2]
    return torch.sin(a) * torch.cos(b) + torch.sin(b) * torch.cos(c) + torch.sin(c) * torch.cos(a)


def capsule(x):          # a thin, tilted capsule: with lipschitz = 0 one block corner sees it and the growth walks along it
    a = torch.tensor([-0.33, -0.33, -0.34], device=x.device)
    d = torch.tensor([0.59, 0.11, 0.24], device=x.device)
    s = (((x - a) * d).sum(1) / float((d * d).sum())).clamp(0, 1)
    q = x - a - s[:, None] * d
    return torch.sqrt(q[:, 0] ** 2 + q[:, 1] ** 2 + q[:, 2] ** 2) - 0.048


def blobs(x):          # a wavy field with many sign changes
    return torch.sin(5.1 * x[:, 0] + 0.3) * torch.sin(4.3 * x[:, 1] - 0.2) + 0.8 * torch.sin(3.7 * x[:, 2] + 4.9 * x[:, 0]) + 0.1


def _axes(shape):
    return [torch.linspace(-1, 1, n, device="cuda") for n in shape]


def _dense(fn, axes):
    g = torch.meshgrid(*axes, indexing="ij")
    return fn(torch.stack([a.reshape(-1) for a in g], -1)).reshape(g[0].shape).contiguous()


# (sampler, shape, threshold, keywords of band_field)
CASES = [(sphere, (96, 96, 96), 0.0, dict()), (sphere, (97, 97, 97), 0.1, dict(block=4, net_chunk=5000)),
         (steep_sphere, (70, 50, 90), 0.0, dict()), (torus, (70, 50, 90), 0.0, dict(block=7)),
         (capsule, (97, 97, 97), 0.0, dict(lipschitz=0.0)), (capsule, (97, 97, 97), 0.0, dict(block=5, net_chunk=777)),
         (gyroid, (64, 48, 40), 0.0, dict()), (gyroid, (64, 48, 40), 0.2, dict(lipschitz=0.0, max_fraction=1.0, block=6)),
         (blobs, (70, 50, 90), 0.0, dict(lipschitz=0.0, max_fraction=1.0)), (blobs, (33, 61, 47), -0.3, dict(block=3, lipschitz=0.3)),
         (sphere, (9, 17, 130), 0.0, dict(block=16)), (torus, (9, 17, 130), 0.0, dict(block=32, max_fraction=1.0)),
         (sphere, (2, 3, 2), 0.9, dict(block=2, max_fraction=1.0))]


@pytest.mark.parametrize("fn,shape,thr,kw", CASES, ids=[f"{c[0].__name__}-{'x'.join(map(str, c[1]))}-{i}" for i, c in enumerate(CASES)])
def test_engine_equals_the_host_twin_and_the_dense_mesh(eng, fn, shape, thr, kw):
    from endosurf_amd.meshing import band_field
    axes = _axes(shape)
    u = _dense(fn, axes)
    field, stats, rounds = eng.band_field(fn, axes, thr, **kw)
    assert field.is_cuda and field.shape == u.shape and field.dtype == torch.float32 and rounds.dtype == torch.int32
    # the host twin on the same values: same block sets, same counts, same assembled field
    host_kw = {k: v for k, v in kw.items() if k != "net_chunk"}
    ax_np = [a.cpu().numpy() for a in axes]
    hf, hs, hr = band_field(lookup(u.cpu().numpy(), ax_np), ax_np, thr, return_blocks=True, **host_kw)
    assert stats == hs, (stats, hs)
    assert np.array_equal(rounds.cpu().numpy(), hr)
    assert np.array_equal(field.cpu().numpy(), hf, equal_nan=True)
    # the mesh is the dense field's
    dv, dt, de = eng.iso_surface(u, thr)
    bv, bt, be, bs = eng.iso_surface_band(fn, axes, thr, **kw)
    assert bs == stats and dv.shape[0] > 0
    assert torch.equal(bv, dv) and torch.equal(bt, dt) and torch.equal(be, de)
    # twice the same
    f2, s2, r2 = eng.band_field(fn, axes, thr, **kw)
    assert torch.equal(f2, field) and s2 == stats and torch.equal(r2, rounds)


def test_the_cases_cover_growth_fallback_and_culling(eng):
    st = lambda fn, shape, thr=0.0, **kw: eng.band_field(fn, _axes(shape), thr, **kw)[1]
    s = st(sphere, (96, 96, 96))
    assert not s["fallback"] and s["rounds"] == 0 and s["evaluated_points"] < 0.35 * s["dense_points"]
    s = st(capsule, (97, 97, 97), lipschitz=0.0)
    assert 0 < s["seed_blocks"] <= 16 and s["active_blocks"] > s["seed_blocks"] and s["rounds"] >= 3 and s["evaluated_points"] < 0.03 * s["dense_points"]
    s = st(steep_sphere, (70, 50, 90))
    assert not s["fallback"] and s["seed_blocks"] < st(sphere, (70, 50, 90))["seed_blocks"]
    s = st(gyroid, (64, 48, 40))
    assert s["fallback"] and s["active_blocks"] == s["blocks"] and s["evaluated_points"] == s["dense_points"] + 9 * 7 * 6
    s = st(blobs, (70, 50, 90), lipschitz=0.0, max_fraction=1.0)
    assert not s["fallback"] and s["rounds"] >= 1


def test_nan_values_are_outside_and_force_their_blocks(eng):
    from endosurf_amd.meshing import band_field
    axes = _axes((65, 65, 65))

    def fn(x):
        u = sphere(x)
        return torch.where((x[:, 0] < -0.7) & (x[:, 1] < -0.7) & (x[:, 2] < -0.7), torch.full_like(u, float("nan")), u)

    u = _dense(fn, axes)
    field, stats, rounds = eng.band_field(fn, axes, 0.0)
    ax_np = [a.cpu().numpy() for a in axes]
    hf, hs, hr = band_field(lookup(u.cpu().numpy(), ax_np), ax_np, 0.0, return_blocks=True)
    assert stats == hs and np.array_equal(rounds.cpu().numpy(), hr) and np.array_equal(field.cpu().numpy(), hf, equal_nan=True)
    assert int(rounds[0, 0, 0]) == 1 and int(rounds[1, 1, 1]) == 1 and bool(torch.isnan(field[:9, :9, :9]).any())
    dv, dt, _ = eng.iso_surface(u, 0.0)
    bv, bt, _ = eng.iso_surface(field, 0.0)
    assert torch.equal(bt, dt) and np.array_equal(bv.cpu().numpy(), dv.cpu().numpy(), equal_nan=True)


def test_bad_arguments(eng):
    from endosurf_amd._lib import EndoSurfHipError
    axes = _axes((12, 12, 12))
    with pytest.raises(EndoSurfHipError, match="on cuda"):
        eng.band_field(sphere, [a.cpu() for a in axes])
    for block in (1, 33):
        with pytest.raises(EndoSurfHipError, match="2..32"):
            eng.band_field(sphere, axes, block=block)
    with pytest.raises(EndoSurfHipError, match="at least 2"):
        eng.iso_surface_band(sphere, [axes[0][:1], axes[1], axes[2]])
    lib = eng.lib
    dummy = torch.zeros(4096, device="cuda")
    p = C.c_void_p(dummy.data_ptr())
    assert lib.es_band_scratch_bytes(8, 8, 8, 8) > 0 and lib.es_band_scratch_bytes(8, 1, 8, 8) == -1 and lib.es_band_scratch_bytes(8, 8, 8, 64) == -1
    assert lib.es_band_scratch_bytes(2048, 1024, 1024, 8) == -1 and b"2^31" in lib.es_last_error()
    assert lib.es_band_scratch_bytes(1290, 1290, 1290, 2) == -1 and b"blocks hold 2^31" in lib.es_last_error()
    assert lib.es_band_seed(None, 8, 8, 8, 4, 0.0, 0.0, p, p, None) == 1 and b"coarse" in lib.es_last_error()
    assert lib.es_band_seed(p, 8, 8, 8, 4, 0.0, 0.0, C.c_void_p(dummy.data_ptr() + 4), p, None) == 1 and b"aligned" in lib.es_last_error()
    assert lib.es_band_lattice_points(p, p, p, 8, 8, 8, 1, 500, 13, p, None) == 1 and b"outside the lattice" in lib.es_last_error()
    assert lib.es_band_lattice_points(p, p, p, 8, 8, 8, 4, 0, 28, p, None) == 1          # the coarse lattice of 8^3 with 4-cell blocks has 27 points
    assert lib.es_band_points(p, p, p, 8, 8, 8, 4, p, 0, 0, 5, p, None) == 1 and b"out of range" in lib.es_last_error()
    assert lib.es_band_scatter(p, 8, 8, 8, 4, p, 9, 0, 5, p, None) == 1          # 8 blocks only
    assert lib.es_band_grow(p, 8, 8, 8, 4, 0.0, 0, p, p, None) == 1 and b"round" in lib.es_last_error()
    assert lib.es_band_fill(8, 8, 8, 4, p, None, None) == 1


# ---- through the renderer, on the trained goldens ------------------------------------------------------------------------------------
BMIN, BMAX, VIEW = [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0], [0.1, -0.2, -1.5]
MESH_KEYS = ("vertices", "triangles", "normals", "sdf", "colors")
# evaluated / dense points (coarse lattice and duplicated faces included), upper bounds: DESIGN 7a quotes the measured values
FRACTION_BOUND = {(129, 8): 0.30, (129, 4): 0.22, (257, 8): 0.15, (257, 4): 0.12}


@pytest.fixture(scope="module", params=["trained_deform", "trained_nodeform"])
def scene(request):
    from gpu_util import renderer_for_case
    from oracle_util import load_case
    return request.param, renderer_for_case(load_case(request.param)), torch.tensor([0.37])


@pytest.fixture(scope="module")
def dense_meshes(scene):
    name, r, t = scene
    return {R: r.extract_observation_mesh(t, BMIN, BMAX, R, view_point=VIEW) for R in (129, 257)}


@pytest.mark.parametrize("R", [129, 257])
@pytest.mark.parametrize("block", [8, 4])
def test_band_mesh_equals_the_dense_mesh_on_a_trained_field(scene, dense_meshes, R, block):
    name, r, t = scene
    dense = dense_meshes[R]
    band = r.extract_observation_mesh(t, BMIN, BMAX, R, view_point=VIEW, band=dict(block=block))
    st = band["stats"]
    print(f"BAND_MEASURED {name} R={R} block={block} V={dense['vertices'].shape[0]} {st}")
    assert set(band) == set(MESH_KEYS) | {"stats"} and set(dense) == set(MESH_KEYS)
    assert dense["vertices"].shape[0] > 10000
    for k in MESH_KEYS:
        assert torch.equal(band[k], dense[k]), k
    assert not st["fallback"] and st["dense_points"] == R ** 3 and st["active_blocks"] >= st["seed_blocks"] > 0
    assert st["evaluated_points"] < FRACTION_BOUND[R, block] * st["dense_points"], st


@pytest.mark.parametrize("R", [129, 257])
def test_sign_changes_only_gives_whole_components(scene, R):
    """lipschitz = 0: the contract instead of equality -- the band vertices (named by the lattice edge they sit on) are dense vertices,
    bit for bit and in the dense order, and no dense triangle joins a kept vertex with a dropped one."""
    name, r, t = scene
    dv, dt, de = r.engine.iso_surface(r._field_on_device(BMIN, BMAX, R, t), 0.0)
    ub, st = r._band_field_on_device(BMIN, BMAX, R, t, 0.0, 1 << 22, dict(lipschitz=0.0))
    bv, bt, be = r.engine.iso_surface(ub, 0.0)
    assert 0 < bv.shape[0] <= dv.shape[0] and st["seed_blocks"] > 0
    key = lambda e: e[:, 0].long() * R ** 3 + e[:, 1].long()
    dk, bk = key(de), key(be)
    order = torch.argsort(dk)
    pos = torch.searchsorted(dk[order], bk).clamp(max=dk.numel() - 1)
    where = order[pos]
    assert torch.equal(dk[where], bk) and bool((where[1:] > where[:-1]).all())          # a subset, in the dense order
    assert torch.equal(dv[where], bv)
    kept = torch.zeros(dv.shape[0], dtype=torch.bool, device=dv.device)
    kept[where] = True
    k = kept[dt.long()]
    assert bool((k.all(1) | ~k.any(1)).all()) and int(k.all(1).sum()) == bt.shape[0]
    print(f"BAND_MEASURED {name} R={R} lipschitz=0: {bv.shape[0]} of {dv.shape[0]} vertices, {st}")


def test_refine_geometry_and_empty_level_set(scene, dense_meshes):
    name, r, t = scene
    R = 129
    d1 = r.extract_observation_mesh(t, BMIN, BMAX, R, view_point=VIEW, refine_steps=1)
    b1 = r.extract_observation_mesh(t, BMIN, BMAX, R, view_point=VIEW, refine_steps=1, band=True)
    for k in MESH_KEYS:
        assert torch.equal(b1[k], d1[k]), k
    assert float(b1["sdf"].abs().median()) < float(dense_meshes[R]["sdf"].abs().median())
    v, f = r.extract_observation_geometry(t, BMIN, BMAX, R, on_device=True, band=True)
    assert isinstance(v, np.ndarray) and np.array_equal(v, dense_meshes[R]["vertices"].cpu().numpy())
    assert np.array_equal(f, dense_meshes[R]["triangles"].cpu().numpy())
    with pytest.raises(ValueError):
        r.extract_observation_geometry(t, BMIN, BMAX, R, band=True)          # the host path has no band
    with pytest.raises(TypeError):
        r.extract_observation_mesh(t, BMIN, BMAX, R, band=dict(blocks=8))
    e = r.extract_observation_mesh(t, BMIN, BMAX, 65, threshold=50.0, view_point=VIEW, band=True)
    assert set(e) == set(MESH_KEYS) | {"stats"}
    assert e["vertices"].shape == (0, 3) and e["triangles"].shape == (0, 3) and e["normals"].shape == (0, 3) and e["sdf"].shape == (0,)
    assert e["stats"]["seed_blocks"] == 0 and e["stats"]["evaluated_points"] == 9 ** 3


def test_without_band_nothing_changed(scene):
    name, r, t = scene
    R = 96
    v, f = r._mesh_on_device(t, BMIN, BMAX, R, 0.0, 1 << 22)
    for kw in (dict(), dict(band=None), dict(band=False)):
        m = r.extract_observation_mesh(t, BMIN, BMAX, R, **kw)
        assert set(m) == {"vertices", "triangles", "normals", "sdf"} and torch.equal(m["vertices"], v) and torch.equal(m["triangles"], f)
        vg, fg = r.extract_observation_geometry(t, BMIN, BMAX, R, cpu=False, on_device=True, **kw)
        assert torch.equal(vg, v) and torch.equal(fg, f)
    u = r._field_on_device(BMIN, BMAX, R, t)
    iv, it, _ = r.engine.iso_surface(u, 0.0)
    assert torch.equal(it, f) and torch.equal(iv / (R - 1.0) * 2.0 - 1.0, v)
