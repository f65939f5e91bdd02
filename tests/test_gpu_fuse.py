"""GPU: depth fusion on the device (csrc/fuse.hip) -- the integration kernel against the host twin on every fixture of
``fuse_util``, the bit-equality of its state under any split of the frames and of the voxels, the volume sampler against the twin, and
``fuse_depth`` / ``fused_mesh`` / ``mesh_coverage`` of the renderer against the composition of the public calls they are made of."""
import numpy as np
import pytest
import torch

import fuse_util as U
from gpu_util import renderer_for

from endosurf_amd import flow as FL
from endosurf_amd import fusion as FU

pytestmark = pytest.mark.gpu

TIMES = [0.2, 0.5, 0.8]
R = 17
VOLUME_KEYS = ("tsdf", "weight", "color")


@pytest.fixture(scope="module")
def eng():
    from endosurf_amd.engine import Engine
    return Engine("cuda")


@pytest.fixture(scope="module", params=[True, False], ids=["deform", "static"])
def rr(request):
    return renderer_for(11, "trained", request.param)


def dev(a, dtype=None):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def device_integrate(eng, c, frames=None, rows=None, state=None):
    """The case ``c`` (or the frames / voxel rows of it given as slices) through ``Engine.tsdf_integrate`` into ``state``."""
    ff, nn = frames or slice(0, c["F"]), rows or slice(0, c["N"])
    pos = c["positions"][ff, nn] if c["positions"].ndim == 3 else c["positions"][nn]
    state = eng.tsdf_state(pos.shape[-2]) if state is None else state
    return eng.tsdf_integrate(state, dev(pos), dev(c["depth"][ff]), eng.flow_cameras(c["cameras"][ff]), dev(c["color"][ff]), dev(c["mask"][ff]),
                              None if c["valid"] is None else dev(c["valid"][ff, nn]), c["trunc"], c["depth_trunc"])


def host(state):
    return {k: v.cpu().numpy() for k, v in state.items() if v is not None}


def same_bits(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a) and sorted(a) == sorted(b)


@pytest.mark.parametrize("p", U.CASES, ids=U.case_id)
def test_kernel_against_the_twin(eng, p):
    c = U.case(*p)
    N, F = c["N"], c["F"]
    state = device_integrate(eng, c)
    got, want = host(state), c["state"]
    ok = ~c["ambiguous"]
    assert ok.sum() >= 0.995 * N
    n_w = int((got["weight"][ok] != want["weight"][ok]).sum())
    d_t = float(np.abs(got["tsdf_sum"][ok].astype(np.float64) - want["tsdf_sum"][ok]).max()) if ok.any() else 0.0
    n_c = int((got["color_sum"][ok] != want["color_sum"][ok]).sum())
    fin = eng.tsdf_finalize(state)
    seen = ok & (want["weight"] > 0)
    ulp_t = U.ulps32(fin["tsdf"].cpu().numpy()[seen], c["final"]["tsdf"][seen])
    ulp_c = U.ulps32(fin["color"].cpu().numpy()[seen], c["final"]["color"][seen])
    worst = max(float(ulp_t.max()), float(ulp_c.max())) if seen.any() else 0.0
    print(f"\n{U.case_id(p)}: {N} voxels, {int((want['weight'] > 0).sum())} observed, {int(c['ambiguous'].sum())} ambiguous; weight differs on "
          f"{n_w}, |tsdf_sum - twin| max {d_t:.2e} (bound {F * 2.0 ** -23:.2e}), color_sum differs on {n_c}, finalised worst {worst:.2f} ulp")
    assert n_w == 0
    # each term is a value of magnitude <= 1 whose fp64 preimage may differ in the last place; the additions are the same, in the same order
    assert d_t <= F * 2.0 ** -23
    assert n_c == 0
    assert worst <= 1.0
    unseen = ok & (want["weight"] == 0)
    assert bool((fin["tsdf"].cpu().numpy()[unseen] == 1).all()) and not fin["color"].cpu().numpy()[unseen].any()
    assert fin["weight"] is state["weight"]


@pytest.mark.parametrize("per_frame", [False, True], ids=["shared", "warped"])
def test_bit_equality_under_any_split(eng, per_frame):
    c = U.case("sphere", 5, "lattice", per_frame)
    N = c["N"]
    whole = host(device_integrate(eng, c))
    assert whole["weight"].max() == 5 and same_bits(host(device_integrate(eng, c)), whole)          # two calls, the same bits
    for blocks in ((2, 2, 1), (1,) * 5):
        state, f0 = eng.tsdf_state(N), 0
        for fb in blocks:
            device_integrate(eng, c, frames=slice(f0, f0 + fb), state=state)
            f0 += fb
        assert same_bits(host(state), whole), blocks
    for chunk in (256, 1000):
        state = eng.tsdf_state(N)
        for n0 in range(0, N, chunk):
            nn = slice(n0, min(n0 + chunk, N))
            device_integrate(eng, c, rows=nn, state={k: v[nn] for k, v in state.items()})
        assert same_bits(host(state), whole), chunk
    # the state without colour takes the same sums
    bare = eng.tsdf_integrate(eng.tsdf_state(N, False), dev(c["positions"]), dev(c["depth"]), eng.flow_cameras(c["cameras"]), None, dev(c["mask"]),
                              None if c["valid"] is None else dev(c["valid"]), c["trunc"], c["depth_trunc"])
    assert bare["color_sum"] is None and np.array_equal(bare["tsdf_sum"].cpu().numpy(), whole["tsdf_sum"])
    assert np.array_equal(bare["weight"].cpu().numpy(), whole["weight"])


def test_an_empty_call_leaves_the_state_untouched(eng):
    c = U.case("sphere", 3, "lattice", False)
    marks = {"tsdf_sum": torch.full((7,), 0.25).cuda(), "weight": torch.full((7,), 3.0).cuda(), "color_sum": torch.full((7, 3), 0.5).cuda()}
    view = {k: v[:0] for k, v in marks.items()}
    eng.tsdf_integrate(view, dev(np.zeros((0, 3), np.float32)), dev(c["depth"]), eng.flow_cameras(c["cameras"]), dev(c["color"]), None, None,
                       c["trunc"])
    fin = eng.tsdf_finalize(view)
    torch.cuda.synchronize()
    assert fin["tsdf"].shape == (0,) and fin["color"].shape == (0, 3)
    assert bool((marks["tsdf_sum"] == 0.25).all()) and bool((marks["weight"] == 3.0).all()) and bool((marks["color_sum"] == 0.5).all())
    with pytest.raises(ValueError, match="trunc"):
        eng.tsdf_integrate(eng.tsdf_state(1), dev(np.zeros((1, 3), np.float32)), dev(c["depth"]), eng.flow_cameras(c["cameras"]), dev(c["color"]),
                           trunc=0.0)
    with pytest.raises(ValueError, match="go together"):
        eng.tsdf_integrate(eng.tsdf_state(1, False), dev(np.zeros((1, 3), np.float32)), dev(c["depth"]), eng.flow_cameras(c["cameras"]),
                           dev(c["color"]), trunc=0.1)
    with pytest.raises(ValueError, match="device tensors only"):
        eng.tsdf_integrate(eng.tsdf_state(1), torch.zeros(1, 3), dev(c["depth"]), eng.flow_cameras(c["cameras"]), dev(c["color"]), trunc=0.1)


@pytest.mark.parametrize("M", [0, 1, 300])
def test_sample_volume_against_the_twin(eng, M):
    vol = U.sphere_volume()
    lo, hi = vol["bound_min"], vol["bound_max"]
    rng = np.random.default_rng(M)
    p = (lo + (rng.uniform(size=(M, 3)) * 1.2 - 0.1) * (hi - lo)).astype(np.float32)          # one row in three lies outside
    if M >= 300:
        p[:6] = np.array([lo, hi, [lo[0], hi[1], 0.0], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, hi[2] + 1e-3]], np.float32)
    for field in (vol["weight"], vol["color"], vol["tsdf"]):
        want, inside = FU.sample_volume(field, p, lo, hi)
        got, got_in = eng.sample_volume(dev(field), dev(p), lo, hi)
        assert got.shape == want.shape and got.dtype == torch.float32 and got_in.dtype == torch.bool
        assert np.array_equal(got_in.cpu().numpy(), inside)
        if M:
            ulp = U.ulps32(got.cpu().numpy(), want.astype(np.float32))
            assert float(ulp.max()) <= 1.0, float(ulp.max())
            assert not got.cpu().numpy()[~inside].any()
    if M >= 300:
        assert 0 < inside.sum() < M


# ---- the renderer ------------------------------------------------------------------------------------------------------------------------------
def compose(r, depth, color, times, max_iters=64, tol=None):
    """``fuse_depth`` spelled out in the public calls it is made of, all voxels and all frames at once."""
    from endosurf_amd.renderer_track import TRACK_TOL
    eng = r.engine
    pts = FU.lattice_points(FU.lattice_axes(*U.MESH_BOUNDS, R, "cuda"))
    N, F = pts.shape[0], len(times)
    trunc = FU.default_trunc(*U.MESH_BOUNDS, R)
    cams = eng.flow_cameras(FL.camera_table(U.KF, U.MESH_POSES)[0])
    state = eng.tsdf_state(N, color is not None)
    pos, valid = pts, None
    if r.use_deform:
        ob = r.to_observed(pts.repeat(F, 1), torch.tensor(times, device="cuda").repeat_interleave(N), max_iters=max_iters,
                           tol=TRACK_TOL if tol is None else tol)
        pos, valid = ob["points"].reshape(F, N, 3), ob["converged"].reshape(F, N)
    eng.tsdf_integrate(state, pos, dev(depth), cams, dev(color), None, valid, trunc)
    fin = eng.tsdf_finalize(state)
    return {"tsdf": fin["tsdf"].view(R, R, R), "weight": fin["weight"].view(R, R, R),
            "color": None if color is None else fin["color"].view(R, R, R, 3), "valid": valid}


def same_volume(a, b):
    return all((a[k] is None and b[k] is None) or torch.equal(a[k], b[k]) for k in VOLUME_KEYS)


def test_fuse_depth_is_the_composition_of_its_public_calls(rr):
    depth, color = U.sphere_frames()
    out = rr.fuse_depth(depth, U.KF, U.MESH_POSES, TIMES, *U.MESH_BOUNDS, R, colors=color, voxel_chunk=2000, frame_block=2)
    want = compose(rr, depth, color, TIMES)
    assert out["space"] == ("canonical" if rr.use_deform else "static") and out["trunc"] == FU.default_trunc(*U.MESH_BOUNDS, R)
    assert all(out[k].is_cuda and not out[k].requires_grad for k in VOLUME_KEYS) and out["tsdf"].shape == (R, R, R) and out["color"].shape == (R, R, R, 3)
    assert same_volume(out, want)
    w = out["weight"]
    print(f"\nfuse_depth ({out['space']}, {R}^3, 3 frames): {int((w > 0).sum())} of {w.numel()} voxels observed, weight max {float(w.max()):.0f}"
          + (f", {int((~want['valid']).sum())} of {want['valid'].numel()} rows not converged" if rr.use_deform else ""))
    assert float(w.max()) == 3 and 0 < int((w > 0).sum()) < w.numel()
    assert same_volume(rr.fuse_depth(depth, U.KF, U.MESH_POSES, TIMES, *U.MESH_BOUNDS, R, colors=color), out)          # any chunking, the same bits
    bare = rr.fuse_depth(depth, U.KF, U.MESH_POSES, TIMES, *U.MESH_BOUNDS, R)
    assert bare["color"] is None and torch.equal(bare["tsdf"], out["tsdf"]) and torch.equal(bare["weight"], out["weight"])
    if not rr.use_deform:          # without a deformation network "canonical" is "static"
        static = rr.fuse_depth(depth, U.KF, U.MESH_POSES, TIMES, *U.MESH_BOUNDS, R, colors=color, space="static")
        assert static["space"] == "static" and same_volume(static, out)
        twin = twin_volume_17()
        ok = ~twin["ambiguous"].reshape(R, R, R)
        assert np.array_equal(out["weight"].cpu().numpy()[ok], twin["weight"][ok])
    else:          # max_iters = 1: rows come back unconverged, and contribute no weight
        one = rr.fuse_depth(depth, U.KF, U.MESH_POSES, TIMES, *U.MESH_BOUNDS, R, colors=color, max_iters=1)
        ref = compose(rr, depth, color, TIMES, max_iters=1)
        lost = ~ref["valid"]
        assert int(lost.sum()) > 0 and same_volume(one, ref)
        never = lost.all(0).reshape(R, R, R)
        assert int(never.sum()) > 0 and bool((one["weight"][never] == 0).all()) and bool((one["tsdf"][never] == 1).all())
        assert bool((one["weight"].reshape(-1) <= ref["valid"].sum(0)).all())
    with pytest.raises(ValueError, match="space"):
        rr.fuse_depth(depth, U.KF, U.MESH_POSES, TIMES, *U.MESH_BOUNDS, R, space="observed")
    with pytest.raises(ValueError, match="poses"):
        rr.fuse_depth(depth, U.KF, U.MESH_POSES[:2], TIMES, *U.MESH_BOUNDS, R)


def twin_volume_17():
    """The twin's static volume on the 17^3 lattice with its ambiguous voxels."""
    depth, color = U.sphere_frames()
    vol = FU.fuse_depth(None, depth, color, None, U.KF, U.MESH_POSES, np.zeros(3), *U.MESH_BOUNDS, R)
    pts = FU.lattice_points(FU.lattice_axes(*U.MESH_BOUNDS, R)).numpy()
    cams = FL.camera_table(U.KF, U.MESH_POSES)[0]
    vol["ambiguous"] = FU.ambiguous_rows(pts, None, depth, cams, vol["trunc"])
    return vol


def test_host_inputs_and_split_precision_change_nothing(rr):
    depth, color = U.sphere_frames()
    out = rr.fuse_depth(dev(depth), U.KF, U.MESH_POSES, TIMES, *U.MESH_BOUNDS, R, colors=dev(color), masks=dev(np.ones(depth.shape, np.float32)))
    rr.engine.split_precision = True
    try:
        split = rr.fuse_depth(depth, U.KF, U.MESH_POSES, TIMES, *U.MESH_BOUNDS, R, colors=color)
    finally:
        rr.engine.split_precision = False
    others = (split,
              rr.fuse_depth(depth.astype(np.float64), torch.from_numpy(U.KF), torch.from_numpy(U.MESH_POSES).cuda(), np.array(TIMES),
                            np.array(U.MESH_BOUNDS[0]), torch.tensor(U.MESH_BOUNDS[1]), R, colors=torch.from_numpy(color).double(),
                            masks=np.ones(depth.shape, bool)),
              rr.fuse_depth(torch.from_numpy(depth), U.KF, U.MESH_POSES, torch.tensor(TIMES, dtype=torch.float64), *U.MESH_BOUNDS, R,
                            colors=torch.from_numpy(color)))
    for other in others:
        assert all(other[k].is_cuda for k in VOLUME_KEYS) and same_volume(other, out)


def test_fused_mesh_on_the_analytic_sphere():
    r = renderer_for(11, "trained", False)
    depth, color = U.sphere_frames()
    twin_vol = U.sphere_volume()
    vol = r.fuse_depth(depth, U.KF, U.MESH_POSES, [0.0, 0.0, 0.0], *U.MESH_BOUNDS, U.MESH_R, colors=color)
    for method in ("tetrahedra", "cubes"):
        twin = FU.fused_mesh(twin_vol, 1.0, iso=method)
        want = U.radial_error(twin["vertices"])
        mesh = r.fused_mesh(vol, 1.0, method=method)
        V = mesh["vertices"].shape[0]
        got = U.radial_error(mesh["vertices"].cpu().numpy())
        print(f"\nfused sphere on the device ({method}): {V} vertices (twin {len(twin['vertices'])}), mean radial error {got:.4e} (twin {want:.4e})")
        assert abs(got - want) <= 0.01 * want          # the reference is the twin; the margin covers the fp32 rounding of vertices
        w = vol["weight"].reshape(-1)
        ends = mesh["edge_ends"].long()
        assert bool((w[ends] >= 1.0).all()) and mesh["triangles"].dtype == torch.int32
        assert V > 100 and mesh["triangles"].shape[0] > 100 and 0 <= int(mesh["triangles"].min()) and int(mesh["triangles"].max()) < V
        assert mesh["colors"].shape == (V, 3) and mesh["weight"].shape == (V,) and bool((mesh["weight"] >= 1.0).all())
        assert r.fused_mesh(vol, 0.0, method=method)["vertices"].shape[0] > V          # the false sheet is there without the filter
        assert "canonical" not in mesh
        at = r.fused_mesh(twin_vol, 1.0, method=method, t=0.3)                         # the host twin's volume is taken as well
        assert at["observed_vertices"].shape == at["vertices"].shape and bool(at["converged"].all())


def test_export_fused_mesh(tmp_path):
    from endosurf_amd.data import read_ply
    r = renderer_for(11, "trained", True)
    depth, color = U.sphere_frames()
    vol = r.fuse_depth(depth, U.KF, U.MESH_POSES, TIMES, *U.MESH_BOUNDS, R, colors=color)
    mesh = r.export_fused_mesh(tmp_path / "fused", vol, t=0.5)
    assert sorted(mesh["paths"]) == ["color", "geometry"] and "canonical" in mesh
    geo, col = read_ply(mesh["paths"]["geometry"]), read_ply(mesh["paths"]["color"])
    assert np.array_equal(geo["vertices"], mesh["observed_vertices"].cpu().numpy()) and np.array_equal(geo["triangles"], mesh["triangles"].cpu().numpy())
    assert col["colors"].shape == (geo["vertices"].shape[0], 3)
    want = r.to_observed(mesh["vertices"], 0.5)
    assert torch.equal(mesh["observed_vertices"], want["points"])


def test_mesh_coverage():
    r = renderer_for(11, "trained", True)
    depth, color = U.sphere_frames()
    vol = r.fuse_depth(depth, U.KF, U.MESH_POSES, TIMES, *U.MESH_BOUNDS, R, colors=color)
    lo, hi = vol["bound_min"], vol["bound_max"]
    rng = np.random.default_rng(3)
    verts = torch.from_numpy((rng.uniform(-0.55, 0.55, (500, 3))).astype(np.float32)).cuda()
    tris = torch.from_numpy(rng.integers(0, 500, (200, 3)).astype(np.int32)).cuda()
    t = 0.4
    cov = r.mesh_coverage(verts, vol, t=t)
    want, inside = r.engine.sample_volume(vol["weight"], r.to_canonical(verts, t), lo, hi)
    assert cov["coverage"].shape == (500,) and torch.equal(cov["coverage"], want) and torch.equal(cov["inside"], inside)
    assert 0 < int(inside.sum()) < 500 and float(cov["coverage"].max()) > 0 and bool((cov["coverage"][~inside] == 0).all())
    assert torch.equal(r.mesh_coverage({"vertices": verts.cpu().numpy(), "triangles": tris}, vol, t=t)["coverage"], want)
    # a track: one coverage for every frame, read at the track's canonical vertices
    track = r.track_mesh(verts, tris, t=t, times=TIMES)
    tc = r.mesh_coverage(track, vol)
    want_c, inside_c = r.engine.sample_volume(vol["weight"], track["canonical"], lo, hi)
    assert tc["coverage"].shape == (500,) and torch.equal(tc["coverage"], want_c) and torch.equal(tc["inside"], inside_c)
    assert torch.equal(want_c, want)          # the track's canonical vertices are to_canonical(vertices, t)
    # against the twin's sampler on the same volume and points
    twin, twin_in = FU.sample_volume(vol["weight"].cpu().numpy(), track["canonical"].cpu().numpy(), lo, hi)
    assert np.array_equal(twin_in, inside_c.cpu().numpy()) and float(U.ulps32(want_c.cpu().numpy(), twin.astype(np.float32)).max()) <= 1.0
    # a static volume takes the vertices as they are
    static = dict(vol, space="static")
    sc = r.mesh_coverage(verts, static)
    assert torch.equal(sc["coverage"], r.engine.sample_volume(vol["weight"], verts, lo, hi)[0])
    with pytest.raises(TypeError, match="needs t"):
        r.mesh_coverage(verts, vol)
