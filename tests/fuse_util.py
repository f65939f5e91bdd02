"""Shared by the depth-fusion tests: the coarse 16 x 12 camera of the pixel-track tests, five poses, the 17^3 lattice,
analytic depth frames of a sphere and of a plane made in closed form, with every kind of pixel and voxel the rule skips -- and the host
twin's results on them, computed once per process and never written to."""
import functools

import numpy as np

from flow_util import POSE, rotated_pose

from endosurf_amd import flow as FL
from endosurf_amd import fusion as FU

KC = np.array([[20.0, 0.0, 7.5], [0.0, 20.0, 5.5], [0.0, 0.0, 1.0]])          # the coarse 12 x 16 camera of test_gpu_flow.py
KS = np.array([[20.0, 0.7, 7.5], [0.0, 20.0, 5.5], [0.0, 0.0, 1.0]])          # the same with a skew term, K01 != 0
K1 = np.array([[20.0, 0.0, 0.0], [0.0, 20.0, 0.0], [0.0, 0.0, 1.0]])          # a 1 x 1 image: the pixel around the optical axis
KF = np.array([[80.0, 0.0, 31.5], [0.0, 80.0, 23.5], [0.0, 0.0, 1.0]])        # a finer 48 x 64 camera, for the mesh
H, W = 12, 16
HF, WF = 48, 64


def _inside_pose():
    """A camera inside the lattice: the voxels with z below its own are behind it."""
    P = rotated_pose(0.0519, -0.0733)
    P[2, 3] = -0.4537
    return P


# three poses with irrational-looking angles and shifts, one inside the lattice, one more
POSES = np.stack([rotated_pose(0.0731, 0.0417), rotated_pose(-0.1193, -0.0873), rotated_pose(0.0377, 0.1291), _inside_pose(),
                  rotated_pose(-0.0291, 0.0613)])
POSES[:, 1, 3] = (0.0171, -0.0239, 0.0317, -0.0113, 0.0457)          # (the lattice holds y = 0: no camera may sit at that height)
BOUND_MIN, BOUND_MAX = (-0.6, -0.5, -0.55), (0.6, 0.5, 0.55)
RADIUS = 0.35
PLANE_N, PLANE_C = np.array([0.12, -0.07, 1.0]) / np.linalg.norm([0.12, -0.07, 1.0]), 0.0831
DEPTH_TRUNC = 3.0
FRAMES = (1, 3, 5)
SIZES = ("lattice", "one", "none")


def pixel_dirs(K, pose, height, width):
    """World directions [H,W,3] of the pixel centres' rays with camera z = 1 (so the ray parameter IS the z-depth) and the origin."""
    jj, ii = np.meshgrid(np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64))
    y = (ii - K[1, 2]) / K[1, 1]
    x = (jj - K[0, 2] - K[0, 1] * y) / K[0, 0]
    d = np.stack([x, y, np.ones_like(x)], -1) @ pose[:3, :3].T
    return d, pose[:3, 3]


def sphere_depth(K, pose, height, width, radius=RADIUS):
    """The z-depth of the sphere |x| = radius in every pixel, 0 where the ray misses: the smaller root of |o + z d|^2 = r^2."""
    d, o = pixel_dirs(K, pose, height, width)
    a, b, c = (d * d).sum(-1), (d * o).sum(-1), (o * o).sum() - radius * radius
    disc = b * b - a * c
    z = (-b - np.sqrt(np.maximum(disc, 0.0))) / a
    return np.where((disc > 0) & (z > 0), z, 0.0).astype(np.float32)


def plane_depth(K, pose, height, width, normal=PLANE_N, offset=PLANE_C):
    """The z-depth of the plane normal . x = offset in every pixel, 0 where the ray does not meet it in front of the camera."""
    d, o = pixel_dirs(K, pose, height, width)
    den = d @ normal
    with np.errstate(all="ignore"):
        z = (offset - o @ normal) / den
    return np.where(np.isfinite(z) & (z > 0), z, 0.0).astype(np.float32)


def lattice(resolution=17):
    """[R^3, 3] fp32, the package's own lattice (z runs fastest): 17^3 = 4913 = 19 workgroups of 256 and a tail of 49."""
    return FU.lattice_points(FU.lattice_axes(BOUND_MIN, BOUND_MAX, resolution)).numpy()


def positions_for(size):
    if size == "lattice":
        return lattice()
    if size == "one":
        return np.array([[0.0131, -0.0217, -0.3013]], np.float32)
    return np.zeros((0, 3), np.float32)


@functools.lru_cache(maxsize=None)
def case(scene, F, size, per_frame):
    """One fixture: dict(positions [N,3] or [F,N,3], valid [F,N] or None, depth, color, mask, cameras, trunc, depth_trunc, H, W) and the
    twin's ``state``, ``final`` and ``ambiguous`` rows.  ``scene``: "sphere", "plane", "skew" (the sphere through KS) or "pixel" (the
    plane in a 1 x 1 image).  The frames hold zero-depth holes (the sphere's background and punched ones), masked pixels, one NaN and
    pixels beyond ``depth_trunc``; pose 3 has voxels behind it, and the lattice is wider than every camera's field of view."""
    K = {"sphere": KC, "plane": KC, "skew": KS, "pixel": K1}[scene]
    h, w = (1, 1) if scene == "pixel" else (H, W)
    maker = plane_depth if scene in ("plane", "pixel") else sphere_depth
    poses = POSES[:F]
    depth = np.stack([maker(K, P, h, w) for P in poses])
    rng = np.random.default_rng(1000 * F + len(scene))
    color = rng.uniform(0, 1, (F, h, w, 3)).astype(np.float32)
    mask = np.ones((F, h, w), np.float32)
    if scene != "pixel":
        depth[:, 5, 6] = 0.0                     # a punched hole
        depth[0, 4, 9] = np.nan                  # one NaN
        depth[:, 7, 8:10] = 5.0                  # beyond depth_trunc
        mask[:, 6, 3:12:2] = 0.0                 # masked pixels
    base = positions_for(size)
    N = base.shape[0]
    positions, valid = base, None
    if per_frame:
        # the lattice displaced smoothly, differently in every frame, and nine rows in ten valid
        f = np.arange(F, dtype=np.float64)[:, None, None]
        b = base.astype(np.float64)[None]
        positions = (b + 0.031 * np.sin(2.3 * b[..., ::-1] + 0.7 * f + 0.2)).astype(np.float32)
        valid = rng.uniform(size=(F, N)) < 0.9
    cameras, _ = FL.camera_table(K, poses)
    trunc = FU.default_trunc(BOUND_MIN, BOUND_MAX, 17)
    c = dict(positions=positions, valid=valid, depth=depth, color=color, mask=mask, cameras=cameras, trunc=trunc, depth_trunc=DEPTH_TRUNC,
             H=h, W=w, N=N, F=F, K=K, poses=poses)
    state = FU.integrate(FU.new_state(N), positions, valid, depth, color, mask, cameras, trunc, DEPTH_TRUNC)
    c.update(state=state, final=FU.finalize(state), ambiguous=FU.ambiguous_rows(positions, valid, depth, cameras, trunc))
    for a in (*state.values(), *c["final"].values(), c["ambiguous"], depth, color, mask):
        a.setflags(write=False)
    return c


CASES = [(scene, F, size, per_frame) for scene in ("sphere", "plane", "skew") for F in FRAMES for size in SIZES for per_frame in (False, True)
         if size == "lattice" or (scene == "sphere" and F == 3)] + [("pixel", 3, "lattice", False), ("pixel", 1, "one", True)]


def case_id(p):
    return f"{p[0]}-F{p[1]}-{p[2]}-{'warped' if p[3] else 'shared'}"


# ---- the sphere for the mesh ---------------------------------------------------------------------------------------------------------------
MESH_R = 25
MESH_BOUNDS = ((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5))
MESH_POSES = POSES[[0, 1, 2]]


@functools.lru_cache(maxsize=None)
def sphere_frames():
    """Three frames of the sphere through the finer camera, with a colour that is a function of the pixel."""
    depth = np.stack([sphere_depth(KF, P, HF, WF) for P in MESH_POSES])
    jj, ii = np.meshgrid(np.arange(WF), np.arange(HF))
    color = np.broadcast_to(np.stack([jj / (WF - 1), ii / (HF - 1), 0.5 + 0 * jj], -1).astype(np.float32), (3, HF, WF, 3)).copy()
    depth.setflags(write=False), color.setflags(write=False)
    return depth, color


@functools.lru_cache(maxsize=None)
def sphere_volume():
    """The twin's static fusion of ``sphere_frames`` on the 25^3 lattice of MESH_BOUNDS."""
    depth, color = sphere_frames()
    return FU.fuse_depth(None, depth, color, None, KF, MESH_POSES, np.zeros(3), *MESH_BOUNDS, MESH_R)


def radial_error(vertices, radius=RADIUS):
    """The mean of | |v| - radius | over the vertices [V,3], in fp64."""
    v = np.asarray(vertices, np.float64)
    return float(np.abs(np.sqrt((v * v).sum(-1)) - radius).mean())


def ulps32(got, want):
    """|got - want| in units of the last place of ``want`` (fp32), elementwise."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
