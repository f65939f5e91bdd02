"""CPU: the host twin of the depth fusion (endosurf_amd/fusion.py) against closed forms -- a fronto-parallel plane, an
affine field, the analytic sphere --, the bit-equality of its state under any split of the frames and of the voxels, the share of
ambiguous rows in every fixture of the device tests, and the refusals of the three C entries (host addresses, nothing dereferenced)."""
import ctypes as C

import numpy as np
import pytest

import fuse_util as U
from flow_util import POSE

from endosurf_amd import flow as FL
from endosurf_amd import fusion as FU


# ---- a plane seen fronto-parallel ----------------------------------------------------------------------------------------------------------
Z0, TRUNC = 0.125, 0.2          # the plane z = 1/8; lattice z values are multiples of 1/16, so s = Z0 - z is exact


def frontal(F):
    """F cameras looking along +z from z = -1.5 (identity rotation), shifted sideways; the plane z = Z0 has depth Z0 + 1.5 in every pixel."""
    poses = np.stack([POSE.copy() for _ in range(F)])
    poses[:, 0, 3] = 0.0173 + 0.0291 * np.arange(F)
    poses[:, 1, 3] = -0.0117 + 0.0077 * np.arange(F)
    depth = np.full((F, U.H, U.W), Z0 + 1.5, np.float32)
    return poses, depth, FL.camera_table(U.KC, poses)[0]


def frontal_lattice():
    ax = FU.lattice_axes((-0.25, -0.1875, -0.5), (0.25, 0.1875, 0.5), 17)
    return FU.lattice_points(ax).numpy()


@pytest.mark.parametrize("F", [1, 3, 5])
def test_plane_seen_fronto_parallel(F):
    poses, depth, cams = frontal(F)
    pts = frontal_lattice()
    assert FU.ambiguous_rows(pts, None, depth, cams, TRUNC).mean() <= 0.005
    st = FU.integrate(FU.new_state(len(pts), False), pts, None, depth, None, None, cams, TRUNC)
    out = FU.finalize(st)
    s = Z0 - pts[:, 2].astype(np.float64)
    seen = s >= -TRUNC
    assert seen.any() and (~seen).any() and (s > TRUNC).any()
    assert np.array_equal(out["weight"][seen], np.full(seen.sum(), F, np.float32))          # every voxel projects into every image
    assert np.array_equal(out["tsdf"][seen], np.minimum(1.0, s[seen] / TRUNC).astype(np.float32))
    assert np.array_equal(out["weight"][~seen], np.zeros((~seen).sum(), np.float32))
    assert np.array_equal(out["tsdf"][~seen], np.ones((~seen).sum(), np.float32))


@pytest.mark.parametrize("kind", ["hole", "masked", "nan", "far"])
def test_pixels_that_do_not_count(kind):
    poses, depth, cams = frontal(3)
    pts = frontal_lattice()
    mask = np.ones(depth.shape, np.float32)
    if kind == "masked":
        mask[:] = 0
    else:
        depth[:] = {"hole": 0.0, "nan": np.nan, "far": 1.7}[kind]
    color = np.ones(depth.shape + (3,), np.float32)
    out = FU.finalize(FU.integrate(FU.new_state(len(pts)), pts, None, depth, color, mask, cams, TRUNC, depth_trunc=1.65))
    assert not out["weight"].any() and (out["tsdf"] == 1).all() and not out["color"].any()


def test_colour_is_the_mean_of_the_gathered_pixels():
    poses, depth, cams = frontal(3)
    pts = frontal_lattice()
    color = np.stack([np.full((U.H, U.W, 3), v, np.float32) for v in (0.25, 0.5, 0.75)])
    out = FU.finalize(FU.integrate(FU.new_state(len(pts)), pts, None, depth, color, None, cams, TRUNC))
    seen = out["weight"] > 0
    assert np.array_equal(out["color"][seen], np.full((seen.sum(), 3), 0.5, np.float32))


# ---- bit equality under any split ------------------------------------------------------------------------------------------------------------
def integrate_split(c, frame_blocks, voxel_chunk):
    N, F = c["N"], c["F"]
    st = FU.new_state(N)
    per_frame = c["positions"].ndim == 3
    for n0 in range(0, max(N, 1), voxel_chunk):
        nn = slice(n0, min(n0 + voxel_chunk, N))
        part = {k: v[nn] for k, v in st.items()}
        f0 = 0
        for fb in frame_blocks:
            ff = slice(f0, f0 + fb)
            f0 += fb
            FU.integrate(part, c["positions"][ff, nn] if per_frame else c["positions"][nn], None if c["valid"] is None else c["valid"][ff, nn],
                         c["depth"][ff], c["color"][ff], c["mask"][ff], c["cameras"][ff], c["trunc"], c["depth_trunc"])
        assert f0 == F
    return st


@pytest.mark.parametrize("per_frame", [False, True])
@pytest.mark.parametrize("scene", ["sphere", "plane"])
def test_any_split_of_frames_and_voxels_gives_the_same_bits(scene, per_frame):
    c = U.case(scene, 5, "lattice", per_frame)
    assert c["state"]["weight"].max() == 5 and (c["state"]["weight"] == 0).any()
    for blocks, chunk in (((5,), c["N"]), ((2, 2, 1), c["N"]), ((1,) * 5, c["N"]), ((5,), 256), ((5,), 1000), ((2, 3), 777)):
        st = integrate_split(c, blocks, chunk)
        for k in FU.STATE_KEYS:
            assert np.array_equal(st[k], c["state"][k]), (blocks, chunk, k)


# ---- the fixtures of the device tests ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", U.CASES, ids=U.case_id)
def test_ambiguity_cap_holds_for_every_fixture(p):
    """A condition on the fixtures, met by the twin alone: at most 0.5 % of the rows hang on the last bits of an fp64 expression."""
    c = U.case(*p)
    assert c["ambiguous"].shape == (c["N"],)
    assert c["ambiguous"].sum() <= 0.005 * c["N"], int(c["ambiguous"].sum())


def test_fixtures_exercise_every_skip():
    c = U.case("sphere", 5, "lattice", False)
    d = c["depth"]
    assert (d == 0).any() and np.isnan(d).sum() == 1 and (d > c["depth_trunc"]).any() and (c["mask"] == 0).any()
    behind, outside = 0, 0
    for cam in c["cameras"]:
        z, _, _, ok, _, _ = FU._project(c["positions"], cam, c["H"], c["W"])
        behind += int((z <= 0).sum())
        outside += int(((z > 0) & ~ok).sum())
    assert behind > 0 and outside > 0
    w = c["state"]["weight"]
    assert 0 < (w > 0).mean() < 1 and len(np.unique(w)) == 6          # every count from 0 to 5 occurs
    assert U.case("skew", 3, "lattice", False)["K"][0, 1] != 0
    assert U.case("pixel", 3, "lattice", False)["state"]["weight"].sum() > 0
    assert U.case("sphere", 3, "one", False)["state"]["weight"][0] > 0


# ---- the sampler -----------------------------------------------------------------------------------------------------------------------------------
def test_sample_volume_reproduces_an_affine_field():
    """Lattice coordinates and coefficients are dyadic, so the field is exact in fp32 at the lattice points; trilinear interpolation
    reproduces an affine field, here to the rounding of the fp64 blends."""
    R = 9
    lo, hi = np.array([-1.0, -0.5, 0.0]), np.array([1.0, 1.5, 2.0])
    X = np.stack(np.meshgrid(*[np.linspace(lo[k], hi[k], R) for k in range(3)], indexing="ij"), -1)
    coef, off = np.array([[0.5, -0.25, 2.0], [1.0, 0.75, -0.5]]), np.array([0.125, -1.0])
    vol = X @ coef.T + off
    assert np.array_equal(vol.astype(np.float32).astype(np.float64), vol)
    rng = np.random.default_rng(5)
    p = (lo + rng.uniform(size=(300, 3)) * (hi - lo)).astype(np.float32)
    p[:3] = np.array([lo, hi, [lo[0], hi[1], 0.75]], np.float32)          # corners and a lattice point
    val, inside = FU.sample_volume(vol, p, lo, hi)
    assert inside.all() and val.shape == (300, 2)
    assert np.abs(val - (p.astype(np.float64) @ coef.T + off)).max() <= 1e-12
    one, _ = FU.sample_volume(vol[..., 0], p, lo, hi)
    assert one.shape == (300,) and np.array_equal(one, val[:, 0])


def test_sample_volume_outside_and_non_finite_points():
    R = 5
    vol = np.arange(R ** 3, dtype=np.float32).reshape(R, R, R) + 1
    lo, hi = np.array([-1.0, -1.0, -1.0]), np.array([1.0, 1.0, 1.0])
    p = np.array([[0, 0, 0], [1.0001, 0, 0], [0, -1.5, 0], [np.nan, 0, 0], [0, np.inf, 0], [1, 1, 1], [-1, -1, -1]], np.float32)
    val, inside = FU.sample_volume(vol, p, lo, hi)
    assert inside.tolist() == [True, False, False, False, False, True, True]
    assert (val[~inside] == 0).all() and val[5] == R ** 3 and val[6] == 1 and val[0] == vol[2, 2, 2]
    v4, i4 = FU.sample_volume(np.stack([vol, -vol], -1), p, lo, hi)
    assert v4.shape == (7, 2) and np.array_equal(v4[:, 0], val) and np.array_equal(v4[:, 1], -val) and np.array_equal(i4, inside)


# ---- the mesh ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iso", ["tetrahedra", "cubes"])
def test_fused_mesh_on_the_sphere(iso):
    vol = U.sphere_volume()
    assert vol["space"] == "static" and vol["tsdf"].shape == (U.MESH_R,) * 3
    cell = float(((vol["bound_max"] - vol["bound_min"]) / (U.MESH_R - 1)).max())
    assert vol["trunc"] == 4.0 * cell
    mesh = FU.fused_mesh(vol, min_weight=1.0, iso=iso)
    V = len(mesh["vertices"])
    assert V > 100 and len(mesh["triangles"]) > 100 and 0 <= mesh["triangles"].min() and mesh["triangles"].max() < V
    w = vol["weight"].reshape(-1)
    assert (w[mesh["edge_ends"]] >= 1.0).all()                     # no kept vertex has an end that was never observed
    u = vol["tsdf"].reshape(-1)
    assert (u[mesh["edge_ends"][:, 0]] < 0).all() and (u[mesh["edge_ends"][:, 1]] >= 0).all()
    assert (mesh["weight"] >= 1.0).all() and (mesh["weight"] <= 3.0).all()
    assert mesh["colors"].shape == (V, 3) and (mesh["colors"] >= 0).all() and (mesh["colors"] <= 1).all()
    # without the filter the extractor also meshes the sheet between observed and never-observed voxels
    every = FU.fused_mesh(vol, min_weight=0.0, iso=iso)
    assert len(every["vertices"]) > V
    err = U.radial_error(mesh["vertices"])
    print(f"fused sphere ({iso}, {U.MESH_R}^3, 3 frames of {U.WF} x {U.HF}): {V} vertices, mean radial error {err:.3e}, cell side {cell:.3e}, "
          f"unfiltered {U.radial_error(every['vertices']):.3e}")
    # the zero crossing lies on a lattice edge between a positive and a negative end: the bound is the edge length, not a tuned number
    assert err < cell


def test_fuse_depth_canonical_path():
    """With D = 0 the canonical volume is the static one bit for bit, whatever the chunking; with a map that never converges no row
    may count."""
    import torch
    depth, color = U.sphere_frames()
    times = np.array([0.0, 0.5, 1.0])
    still = lambda y, t: torch.zeros_like(y)
    a = FU.fuse_depth(still, depth, color, None, U.KF, U.MESH_POSES, times, *U.MESH_BOUNDS, 9, voxel_chunk=200, frame_block=2)
    b = FU.fuse_depth(None, depth, color, None, U.KF, U.MESH_POSES, times, *U.MESH_BOUNDS, 9)
    assert a["space"] == "canonical" and b["space"] == "static" and b["weight"].max() == 3
    for k in ("tsdf", "weight", "color"):
        assert np.array_equal(a[k], b[k]), k
    wild = lambda y, t: -2.0 * y + 0.3          # Lipschitz 2: the iteration's step doubles
    c = FU.fuse_depth(wild, depth, color, None, U.KF, U.MESH_POSES, times, *U.MESH_BOUNDS, 9, max_iters=3)
    assert not c["weight"].any() and (c["tsdf"] == 1).all()


# ---- the C entries' refusals -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from endosurf_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def integrate_call(lib, **over):
    buf = np.zeros(64, np.float64)
    b = buf.ctypes.data          # a host address, 8-byte aligned: never dereferenced, every call below fails on its argument check
    a = dict(positions=b, frame_stride=0, valid=None, N=256, F=2, depth=b, color=b, mask=None, cameras=b, height=12, width=16, trunc=0.1,
             depth_trunc=float("inf"), tsdf_sum=b, weight=b, color_sum=b)
    a.update(over)
    return lib.es_tsdf_integrate(a["positions"], a["frame_stride"], a["valid"], a["N"], a["F"], a["depth"], a["color"], a["mask"], a["cameras"],
                                 a["height"], a["width"], a["trunc"], a["depth_trunc"], a["tsdf_sum"], a["weight"], a["color_sum"], None), buf


REFUSALS = [
    (dict(positions=None), b"null buffer"), (dict(depth=None), b"null buffer"), (dict(cameras=None), b"null buffer"),
    (dict(tsdf_sum=None), b"null buffer"), (dict(weight=None), b"null buffer"),
    (dict(misalign="cameras"), b"8-byte aligned"), (dict(misalign="depth"), b"4-byte aligned"), (dict(misalign="tsdf_sum"), b"4-byte aligned"),
    (dict(color_sum=None), b"go together"), (dict(color=None), b"go together"),
    (dict(height=0), b"[1, 8192]"), (dict(width=8193), b"[1, 8192]"), (dict(height=-1), b"[1, 8192]"),
    (dict(F=1 << 12, height=1 << 10, width=1 << 9), b"F H W"), (dict(N=(1 << 31) // 3 + 1), b"3 N"), (dict(N=1 << 20, F=1 << 11), b"F N"),
    (dict(N=-1), b"negative"), (dict(F=-1), b"negative"),
    (dict(trunc=0.0), b"trunc"), (dict(trunc=-1.0), b"trunc"), (dict(trunc=float("inf")), b"trunc"), (dict(trunc=float("nan")), b"trunc"),
    (dict(depth_trunc=0.0), b"depth_trunc"), (dict(depth_trunc=float("nan")), b"depth_trunc"), (dict(depth_trunc=-2.0), b"depth_trunc"),
    (dict(frame_stride=255), b"frame_stride"), (dict(frame_stride=-256), b"frame_stride"),
]


@pytest.mark.parametrize("over,message", REFUSALS, ids=[f"{i}-{'-'.join(o)}" for i, (o, _) in enumerate(REFUSALS)])
def test_integrate_refuses_bad_arguments_before_launch(lib, over, message):
    over = dict(over)
    name = over.pop("misalign", None)
    if name:
        buf = np.zeros(64, np.float64)
        over[name] = buf.ctypes.data + (4 if name == "cameras" else 2)
        over["_keep"] = buf
    keep = over.pop("_keep", None)
    status, _ = integrate_call(lib, **over)
    assert status == 1
    assert message in lib.es_last_error(), lib.es_last_error()


def test_empty_calls_return_zero_and_launch_nothing(lib):
    assert integrate_call(lib, N=0)[0] == 0 and integrate_call(lib, F=0)[0] == 0
    assert integrate_call(lib, N=0, positions=None, depth=None, tsdf_sum=None, weight=None, cameras=None)[0] == 0
    assert lib.es_tsdf_finalize(None, None, None, 0, None, None, None) == 0
    bounds = (C.c_double * 6)(-1, -1, -1, 1, 1, 1)
    assert lib.es_volume_sample(None, 5, 1, None, 0, bounds, None, None, None) == 0
    assert integrate_call(lib, frame_stride=256, F=0)[0] == 0


def test_finalize_and_sample_refuse_bad_arguments_before_launch(lib):
    buf = np.zeros(64, np.float64)
    b = buf.ctypes.data
    assert lib.es_tsdf_finalize(b, b, b, 16, b, None, None) == 1 and b"go together" in lib.es_last_error()
    assert lib.es_tsdf_finalize(b, b, None, 16, b, b, None) == 1 and b"go together" in lib.es_last_error()
    assert lib.es_tsdf_finalize(b, None, None, 16, b, None, None) == 1 and b"null buffer" in lib.es_last_error()
    assert lib.es_tsdf_finalize(b, b, None, -1, b, None, None) == 1 and b"negative" in lib.es_last_error()
    good = (C.c_double * 6)(-1, -1, -1, 1, 1, 1)
    sample = lambda R=5, Cn=1, M=16, bounds=good, vol=b: lib.es_volume_sample(vol, R, Cn, b, M, bounds, b, b, None)
    assert sample(R=1) == 1 and b"resolution" in lib.es_last_error()
    assert sample(R=2049) == 1 and b"resolution" in lib.es_last_error()
    assert sample(Cn=0) == 1 and b"channels" in lib.es_last_error()
    assert sample(Cn=9) == 1 and b"channels" in lib.es_last_error()
    assert sample(R=1024, Cn=2) == 1 and b"resolution^3 channels" in lib.es_last_error()
    assert sample(M=-1) == 1 and b"negative" in lib.es_last_error()
    assert sample(M=1 << 28) == 1 and b"8 M" in lib.es_last_error()
    assert sample(bounds=None) == 1 and b"bounds" in lib.es_last_error()
    assert sample(bounds=(C.c_double * 6)(-1, -1, -1, 1, -1, 1)) == 1 and b"bound_max > bound_min" in lib.es_last_error()
    assert sample(bounds=(C.c_double * 6)(-1, -1, float("nan"), 1, 1, 1)) == 1 and b"bound_max > bound_min" in lib.es_last_error()
    assert sample(vol=None) == 1 and b"null buffer" in lib.es_last_error()
