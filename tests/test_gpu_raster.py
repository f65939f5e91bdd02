"""Mesh rasteriser on the device (csrc/raster.hip: Engine.project_vertices / rasterize_projected / rasterize,
EndoSurfRenderer.render_mesh / mesh_depth_error) against the numpy twins in endosurf_amd.meshing, which tests/test_raster_host.py checks
against independent formulations.  Stage B is compared on the device's OWN snapped vertices, so that its promise is tested on its own:
the same integers in, the same picture out."""
import ctypes as C

import numpy as np
import pytest
import torch

from endosurf_amd import data as D
from endosurf_amd import meshing as M
from mesh_util import hand_meshes
from raster_util import camera, fill_rule_case, mt_world, rotation, tetrahedron

pytestmark = pytest.mark.gpu

H, W = 96, 128


@pytest.fixture(scope="module")
def eng():
    from endosurf_amd.engine import Engine
    return Engine("cuda")


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def _cases():
    hand = hand_meshes()
    out = {"tetrahedron": tetrahedron(), "sphere": mt_world("sphere", 41), "torus": mt_world("torus", 49), "gyroid": mt_world("gyroid", 28)}
    for name in ("fans_touching_in_a_vertex", "degenerate", "nine_and_ten"):
        v, f = hand[name]
        out[name] = (v * 0.35, f)
    return out


CASES = _cases()
CAM = camera(H, W, 150.0, eye=(0.05, -0.1, -2.2), rot=rotation((0.2, 1.0, 0.1), 0.15))


def ulps(a, b):
    """Distance in fp32 steps between two arrays of positive floats (inf == inf: 0)."""
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


def against_twin(got, xy, zc, f, h, w, attrs=None, exact=False, **kw):
    """A device result against the twin's stage B on the same snapped vertices: ``triangle`` equal except where the twin's best and
    second-best depth are within one fp32 step (never with ``exact``), depth within one step, bary / attributes to 1e-5."""
    want = M.rasterize_projected(xy.cpu().numpy(), zc.cpu().numpy(), f, h, w, attributes=attrs, runner_up=True, **kw)
    tri, depth = got["triangle"].cpu().numpy(), got["depth"].cpu().numpy()
    assert tri.dtype == np.int32 and depth.dtype == np.float32 and tri.shape == (h, w)
    assert np.array_equal(tri >= 0, want["triangle"] >= 0)
    hit = tri >= 0
    differ = tri != want["triangle"]
    close = np.zeros_like(hit)
    close[hit] = ulps(want["depth"][hit], np.where(np.isfinite(want["second_depth"][hit]), want["second_depth"][hit], np.float32(3e38))) <= 1
    assert not (differ & ~close).any() and not (exact and differ.any()), int(differ.sum())
    assert np.isinf(depth[~hit]).all() and (ulps(depth[hit], want["depth"][hit]) <= 1).all()
    same = hit & ~differ
    assert np.abs(got["bary"].cpu().numpy()[same] - want["bary"][same]).max(initial=0) <= 1e-5
    assert (got["bary"].cpu().numpy()[~hit] == 0).all()
    if attrs is not None:
        a = got["attributes"].cpu().numpy()
        scale = max(1.0, float(np.abs(attrs).max()))
        assert a.shape == want["attributes"].shape and np.abs(a[same] - want["attributes"][same]).max(initial=0) <= 1e-5 * scale and (a[~hit] == 0).all()
    assert got["stats"] == want["stats"], (got["stats"], want["stats"])
    return int(differ.sum()), int((depth[hit] != want["depth"][hit]).sum()), want


@pytest.mark.parametrize("name", sorted(CASES))
def test_projection_equals_the_twin(eng, name):
    v, f = CASES[name]
    v = np.concatenate([v, np.array([[np.nan, 0, 0], [0, np.inf, 1], [0.05, -0.1, -2.2], [3, 3, -9]], np.float32)])          # bad rows, the eye, behind
    xy, zc = eng.project_vertices(dev(v), *CAM)
    wxy, wzc = M.project_vertices(v, *CAM)
    assert xy.dtype == torch.int32 and tuple(xy.shape) == (len(v), 2) and zc.dtype == torch.float32
    ok = np.isfinite(wzc) & (np.abs(wzc) > 1e-3)
    assert np.abs(xy.cpu().numpy()[ok].astype(np.int64) - wxy[ok]).max() <= 1
    assert np.allclose(zc.cpu().numpy()[ok], wzc[ok], rtol=1e-6, atol=0)
    assert np.array_equal(np.isnan(zc.cpu().numpy()), np.isnan(wzc)) and int(xy.abs().max()) <= 1 << 22
    print(f"RASTER_MEASURED project {name}: {int((xy.cpu().numpy()[ok] != wxy[ok]).sum())} of {2 * ok.sum()} coordinates differ by one unit")


@pytest.mark.parametrize("cull", ["none", "back", "front"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_rasterize_equals_the_twin(eng, name, cull):
    v, f = CASES[name]
    attrs = np.concatenate([v, np.cos(7 * v)], 1).astype(np.float32)          # C = 6
    xy, zc = eng.project_vertices(dev(v), *CAM)
    got = eng.rasterize_projected(xy, zc, dev(f), H, W, attributes=dev(attrs), cull=cull)
    n_tri, n_depth, want = against_twin(got, xy, zc, f, H, W, attrs, cull=cull)
    whole = eng.rasterize(dev(v), dev(f).int(), *CAM, H, W, attributes=dev(attrs), cull=cull)
    for k in ("depth", "triangle", "bary", "attributes"):
        assert torch.equal(whole[k], got[k]), k
    assert whole["stats"] == got["stats"] and (cull != "none" or got["stats"]["covered_pixels"] > 40)
    print(f"RASTER_MEASURED {name} cull={cull}: {got['stats']} ids differing {n_tri}, depths differing {n_depth}")


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_fill_rule_exactly(eng, seed):
    """Coplanar triangles that tile a rectangle: no pixel has two candidates, so the ids must be the twin's with no exception."""
    xy, f, (x0, x1, y0, y1) = fill_rule_case(seed, n_points=200)
    h, w = 20, 24
    zc = torch.full((len(xy),), 2.0, device="cuda")
    got = eng.rasterize_projected(dev(xy), zc, dev(f), h, w)
    n_tri, n_depth, want = against_twin(got, dev(xy), zc, f, h, w, exact=True)
    assert n_tri == 0 and n_depth == 0
    inside = np.zeros((h, w), bool)
    inside[y0:y1, x0:x1] = True
    assert np.array_equal(got["triangle"].cpu().numpy() >= 0, inside) and got["stats"]["covered_pixels"] == inside.sum()
    assert (got["depth"].cpu().numpy()[inside] == 2.0).all()


def test_bit_identical_and_order_independent(eng):
    v, f = CASES["torus"]
    a = eng.rasterize(dev(v), dev(f), *CAM, H, W, attributes=dev(v))
    b = eng.rasterize(dev(v), dev(f), *CAM, H, W, attributes=dev(v))
    for k in ("depth", "triangle", "bary", "attributes"):
        assert torch.equal(a[k], b[k]), k
    # the keys themselves, through the C ABI: two fills of the same mesh leave the same key image
    lib, st = eng.lib, eng.st()
    xy, zc = eng.project_vertices(dev(v), *CAM)
    t32 = dev(f).int().contiguous()
    V, T = len(v), len(f)
    keys = []
    for fill in (0x00, 0xAB):          # whatever the scratch holds on entry
        scratch = torch.full((lib.es_rast_scratch_bytes(V, T, H, W),), fill, dtype=torch.uint8, device="cuda")
        totals = torch.zeros(8, dtype=torch.int64, device="cuda")
        p = lambda t: C.c_void_p(t.data_ptr())
        assert lib.es_rast_count(p(t32), V, T, p(xy), p(zc), H, W, 1e-6, 0, p(scratch), p(totals), st) == 0
        assert lib.es_rast_fill(p(t32), V, T, p(xy), p(zc), H, W, 1e-6, 0, p(scratch), int(totals[0]), st) == 0
        torch.cuda.synchronize()
        keys.append(scratch[:8 * H * W].clone().view(torch.int64))
    assert torch.equal(keys[0], keys[1])
    assert torch.equal((keys[0] >> 32).to(torch.int32).view(torch.float32).view(H, W)[a["triangle"] >= 0], a["depth"][a["triangle"] >= 0])
    # a shuffled triangle list: the same picture, the ids mapped back -- except where two triangles tie in depth (the smaller index wins)
    perm = torch.randperm(T, device="cuda", generator=torch.Generator("cuda").manual_seed(3))
    c = eng.rasterize(dev(v), dev(f)[perm], *CAM, H, W, attributes=dev(v))
    assert torch.equal(c["depth"], a["depth"])
    back = torch.where(c["triangle"] >= 0, perm[c["triangle"].long().clamp_min(0)].int(), c["triangle"])
    ties = int((back != a["triangle"]).sum())
    want = M.rasterize_projected(xy.cpu().numpy(), zc.cpu().numpy(), f, H, W, runner_up=True)
    tie_ok = dev(want["second_depth"] == want["depth"])
    assert bool(((back == a["triangle"]) | tie_ok).all()), ties
    same = back == a["triangle"]
    assert torch.equal(c["bary"][same], a["bary"][same]) and torch.equal(c["attributes"][same], a["attributes"][same])


def test_large_triangles_and_a_large_sheet(eng):
    """A screen-filling quad is thousands of work items, not one thread walking the screen; the 513 x 513 sheet of
    tests/test_gpu_mesh.py is half a million triangles of about a pixel."""
    h, w = 512, 640
    K, pose = camera(h, w, 500.0, eye=(0.0, 0.0, -1.0))
    quad = np.array([[-9, -9, 1], [9, -9, 1.5], [9, 9, 2], [-9, 9, 1.5]], np.float32)
    qf = np.array([[0, 2, 1], [0, 3, 2]])
    xy, zc = eng.project_vertices(dev(quad), K, pose)
    got = eng.rasterize_projected(xy, zc, dev(qf), h, w, attributes=dev(quad))
    assert got["stats"]["covered_pixels"] == h * w and got["stats"]["work_items"] >= (h // 8) * (w // 8)
    against_twin(got, xy, zc, qf, h, w, quad)
    x = np.broadcast_to(np.arange(3, dtype=np.float32)[None, None, :] - 0.5, (513, 513, 3)).copy()
    v, f, _ = eng.iso_surface(dev(x), 0.0)
    assert f.shape[0] >= 2 * 512 * 512
    world = (v / 256.0 - 1.0) * torch.tensor([1.0, 0.8, 0.1], device="cuda") + torch.tensor([0.0, 0.0, 0.4 * 0.1], device="cuda")
    world[:, 2] += 0.3 * world[:, 0]          # tilted: depth varies across the sheet
    xy, zc = eng.project_vertices(world, K, pose)
    got = eng.rasterize_projected(xy, zc, f, h, w, attributes=world)
    n_tri, n_depth, want = against_twin(got, xy, zc, f.cpu().numpy(), h, w, world.cpu().numpy())
    assert got["stats"]["covered_pixels"] > 0.5 * h * w
    print(f"RASTER_MEASURED sheet: T={f.shape[0]} {got['stats']} ids differing {n_tri}, depths differing {n_depth}")


def test_empty_and_bad_input(eng):
    v, f = tetrahedron()
    K, pose = camera(8, 9, 20.0)
    before = __import__("endosurf_amd")._lib.calls
    for vv, ff in ((torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int64)), (torch.from_numpy(v), torch.zeros(0, 3, dtype=torch.int32))):
        out = eng.rasterize_projected(torch.zeros(len(vv), 2, dtype=torch.int32, device="cuda"), torch.ones(len(vv), device="cuda"), ff.cuda(), 8, 9,
                                      attributes=torch.zeros(len(vv), 2, device="cuda"))
        assert bool(torch.isinf(out["depth"]).all()) and bool((out["triangle"] == -1).all()) and tuple(out["attributes"].shape) == (8, 9, 2)
        assert tuple(out["bary"].shape) == (8, 9, 3) and out["stats"]["covered_pixels"] == 0
    assert __import__("endosurf_amd")._lib.calls == before          # no library call: nothing was launched
    one = eng.rasterize(dev(v), dev(f), *camera(1, 1, 60.0), 1, 1)
    assert int(one["triangle"][0, 0]) >= 0 and one["stats"]["covered_pixels"] == 1
    bad = np.concatenate([f, [[0, 1, 7], [0, -1, 2], [2, 2, 1]]])          # indices out of range: counted, never dereferenced
    out = eng.rasterize(dev(v), dev(bad), K, pose, 8, 9)
    assert out["stats"]["invalid"] == 3 and out["stats"] == M.rasterize(v, bad, K, pose, 8, 9)["stats"]
    from endosurf_amd._lib import EndoSurfHipError
    for kw in (dict(height=0), dict(width=8193), dict(cull="both")):
        with pytest.raises(EndoSurfHipError):
            eng.rasterize(dev(v), dev(f), K, pose, **{**dict(height=8, width=9), **kw})
    with pytest.raises(EndoSurfHipError):
        eng.rasterize(dev(v), dev(f), K, pose, 8, 9, attributes=torch.zeros(4, 9, device="cuda"))
    with pytest.raises(EndoSurfHipError):
        eng.rasterize(dev(v), dev(f), K, pose, 8, 9, near=-1.0)
    with pytest.raises(ValueError):
        eng.rasterize(dev(v), dev(f), K, pose * 2, 8, 9)


def test_bad_arguments_return_error_codes(eng):
    lib = eng.lib
    dummy = torch.zeros(4096, dtype=torch.int32, device="cuda")
    p = C.c_void_p(dummy.data_ptr())
    cam = (C.c_double * 17)(1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 50, 0, 4, 50, 4)
    assert lib.es_rast_scratch_bytes(10, 10, 8, 8) > 8 * 64 and lib.es_rast_scratch_bytes(-1, 10, 8, 8) == -1 and b"negative" in lib.es_last_error()
    assert lib.es_rast_scratch_bytes(1 << 31, 10, 8, 8) == -1 and b"2^31" in lib.es_last_error()
    assert lib.es_rast_scratch_bytes(10, 10, 8, 8193) == -1 and b"8192" in lib.es_last_error()
    assert lib.es_rast_project(None, 4, cam, p, p, None) == 1 and b"verts" in lib.es_last_error()
    assert lib.es_rast_project(p, 4, None, p, p, None) == 1 and b"camera" in lib.es_last_error()
    nan_cam = (C.c_double * 17)(*([float("nan")] + list(cam)[1:]))
    assert lib.es_rast_project(p, 4, nan_cam, p, p, None) == 1 and b"finite" in lib.es_last_error()
    flipped = (C.c_double * 17)(*(list(cam)[:12] + [-50, 0, 4, 50, 4]))
    assert lib.es_rast_project(p, 4, flipped, p, p, None) == 1 and b"focal" in lib.es_last_error()
    assert lib.es_rast_project(None, 0, cam, None, None, None) == 0                                   # V == 0: nothing to do
    assert lib.es_rast_count(None, 4, 2, p, p, 8, 8, 1e-6, 0, p, p, None) == 1 and b"tris" in lib.es_last_error()
    assert lib.es_rast_count(p, 4, 2, p, p, 8, 8, 1e-6, 0, None, p, None) == 1 and b"scratch" in lib.es_last_error()
    assert lib.es_rast_count(p, 4, 2, p, p, 8, 8, 1e-6, 0, C.c_void_p(dummy.data_ptr() + 4), p, None) == 1 and b"aligned" in lib.es_last_error()
    assert lib.es_rast_count(p, 4, 2, p, p, 8, 8, 1e-6, 0, p, None, None) == 1 and b"totals" in lib.es_last_error()
    assert lib.es_rast_count(p, 4, 2, p, p, 8, 8, 1e-6, 3, p, p, None) == 1 and b"cull" in lib.es_last_error()
    assert lib.es_rast_count(p, 4, 2, p, p, 8, 8, float("nan"), 0, p, p, None) == 1 and b"near" in lib.es_last_error()
    assert lib.es_rast_count(p, 4, 2, p, p, 0, 8, 1e-6, 0, p, p, None) == 1 and b"8192" in lib.es_last_error()
    assert lib.es_rast_fill(p, 4, 2, p, p, 8, 8, 1e-6, 0, p, 1 << 31, None) == 1 and b"work items" in lib.es_last_error()
    assert lib.es_rast_fill(p, 4, 2, p, p, 8, 8, 1e-6, 0, p, -1, None) == 1 and b"negative" in lib.es_last_error()
    assert lib.es_rast_fill(p, 4, 2, p, p, 8, 8, 1e-6, 0, None, 5, None) == 1 and b"scratch" in lib.es_last_error()
    assert lib.es_rast_fill(None, 4, 2, None, None, 8, 8, 1e-6, 0, None, 0, None) == 0                 # no work: nothing to do
    assert lib.es_rast_resolve(p, 4, 2, p, p, p, 9, 8, 8, 1e-6, 0, p, p, p, p, p, p, None) == 1 and b"n_attrs" in lib.es_last_error()
    assert lib.es_rast_resolve(p, 4, 2, p, p, None, 3, 8, 8, 1e-6, 0, p, p, p, p, p, p, None) == 1 and b"attrs" in lib.es_last_error()
    assert lib.es_rast_resolve(p, 4, 2, p, p, None, 0, 8, 8, 1e-6, 0, p, None, p, p, None, p, None) == 1 and b"depth" in lib.es_last_error()
    torch.cuda.synchronize()
    assert int(dummy.abs().sum()) == 0          # nothing was launched on the dummy buffer


# ---- through the renderer, on the trained golden ---------------------------------------------------------------------------------------
BMIN, BMAX, VIEW = [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0], [0.0, 0.0, -1.5]


@pytest.fixture(scope="module")
def scene():
    from gpu_util import renderer_for_case
    from oracle_util import load_case
    return renderer_for_case(load_case("trained_deform")), torch.tensor([0.37])


def test_pictures_and_depth_of_the_trained_mesh(scene):
    """The extracted mesh seen from a training-style camera: three pictures, and its depth against the volume-rendered depth_map of the
    same camera.  Measured on MI355X at R = 129, 40 x 48 pixels: the median |mesh depth - depth_map| over the 1770 pixels both reach is
    0.0068 = 0.435 grid cells (the mesh is the zero level set, depth_map the weighted mean of the samples around it); the bound is one
    cell, a margin of 2.3 x."""
    r, t = scene
    h, w, R = 40, 48, 129
    K = torch.tensor([[60.0, 0, 23.5, 0], [0, 60.0, 19.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    pose = torch.eye(4)
    pose[:3, 3] = torch.tensor(VIEW)
    rays = D.assemble_rays(D.get_rays(K[None].cuda(), pose[None].cuda(), w, h), torch.zeros(1, 2, device="cuda"))
    rays[..., 8] = float(t)
    vol = r.render_frames(rays, iter_step=1, ray_chunk=512, perturb_overwrite=False, use_graph=False)["depth"].reshape(h, w)
    mesh = r.extract_observation_mesh(t, BMIN, BMAX, R, view_point=VIEW, band=True, components=0.9)
    pics = r.render_mesh(mesh, K, pose, h, w, view_point=VIEW)
    hit = pics["mask"]
    assert hit.dtype == torch.bool and torch.equal(hit, pics["triangle"] >= 0) and 0.1 * h * w < int(hit.sum())
    for k in ("color", "normal", "geometry"):
        img = pics[k]
        assert tuple(img.shape) == (h, w, 3) and bool(torch.isfinite(img).all()) and float(img.min()) >= 0.0 and float(img.max()) <= 1.0
        assert bool((img[~hit] == 1.0).all()), k
        assert D.to8b(img).shape == (h, w, 3)
    assert float(pics["geometry"][hit].std()) > 0.01 and float(pics["color"][hit].std()) > 0.0
    assert bool(torch.isinf(pics["depth"][~hit]).all()) and bool((pics["depth"][hit] > 0).all())
    plain = r.render_mesh((mesh["vertices"], mesh["triangles"]), K, pose, h, w)          # no colours, no analytic normals
    assert torch.equal(plain["depth"], pics["depth"]) and bool(((plain["color"][hit] - 0.7).abs() < 1e-5).all())
    cos = (((plain["normal"] - 0.5) * (pics["normal"] - 0.5)).sum(-1) / ((plain["normal"] - 0.5).norm(dim=-1) * (pics["normal"] - 0.5).norm(dim=-1)))[hit]
    assert float(cos.median()) > 0.9          # area-weighted triangle normals point where the analytic ones do
    both = hit & torch.isfinite(vol) & (vol > 0)
    cell = 2.0 / (R - 1)
    diff = (pics["depth"] - vol)[both].abs()
    med = float(diff.median())
    print(f"RASTER_MEASURED trained R={R}: {pics['stats']} pixels compared {int(both.sum())} median |mesh depth - depth_map| = {med:.5f} "
          f"= {med / cell:.3f} cells, max {float(diff.max()):.4f}")
    assert int(both.sum()) > 0.1 * h * w and med < 1.0 * cell
    err = r.mesh_depth_error(mesh, vol, both, K, pose, depth_scale=2.5)
    want = D.cal_rmse(pics["depth"].nan_to_num(posinf=0.0) * both, vol * both, both.float()) * 2.5
    assert abs(err["rmse"] - want) <= 1e-6 * want and err["coverage"] == 1.0
    half = r.mesh_depth_error(mesh, vol[..., None], torch.ones(h, w, 1), K, pose)
    assert half["coverage"] == pytest.approx(float(hit.float().mean())) and half["rmse"] > 0
