"""Shared by the stereo tests: the small cases at which a kernel can still go wrong, their seeded image pairs, the twin's
results on them (computed once per case and kept unchanged), and three analytic scenes with ground-truth disparity in closed form."""
import functools

import numpy as np

from endosurf_amd import stereo as ST

# (H, W, D, dmin, paths)
CASES = [
    (1, 1, 1, 0, 8),           # smallest possible
    (7, 9, 4, 0, 8),           # the image equals the census window
    (5, 6, 3, 0, 4),           # smaller than the window
    (24, 33, 16, 0, 8),
    (24, 33, 16, 3, 8),        # dmin > 0
    (20, 40, 64, 0, 8),        # D > W
    (37, 70, 48, 0, 4),        # D is not a lane multiple
    (16, 130, 70, 5, 8),       # W > 2 * 64
    (12, 65, 129, 0, 8),
    (9, 31, 256, 0, 8),        # the largest D
]
KINDS = ("noise", "constant")
SPECKLE_SIZE = 8
P1, P2, UNIQUENESS, LR_MAX = 7, 60, 10, 1


def case_id(p):
    return "x".join(str(v) for v in p[:3]) + f"-dmin{p[3]}-p{p[4]}"


def pair(H, W, D, dmin, kind, seed=0):
    """(left, right) uint8 [H,W].  noise: the left image is uniform noise, every row of the right image is that row of the left image
    shifted by one random disparity of the searched range (where it fits the row), with fresh noise where the shift leaves the image.
    constant: both images hold one value, so every argmin ties."""
    rng = np.random.default_rng([seed, H, W, D, dmin])
    if kind == "constant":
        v = int(rng.integers(0, 256))
        return np.full((H, W), v, np.uint8), np.full((H, W), v, np.uint8)
    left = rng.integers(0, 256, (H, W), dtype=np.uint8)
    right = rng.integers(0, 256, (H, W), dtype=np.uint8)
    for y in range(H):
        s = dmin + int(rng.integers(0, D))
        s = min(s, max(W - 1, 0))
        right[y, :W - s] = left[y, s:]
    return left, right


@functools.lru_cache(maxsize=None)
def case(H, W, D, dmin, paths, kind):
    """The pair of a case and everything the twin makes of it (read-only)."""
    left, right = pair(H, W, D, dmin, kind)
    cl, cr = ST.census(left), ST.census(right)
    C = ST.cost_volume(cl, cr, D, dmin)
    S = ST.aggregate(C, P1, P2, paths)
    sel = ST.select(S, dmin, UNIQUENESS, LR_MAX, True)
    out = {"left": left, "right": right, "census_left": cl, "census_right": cr, "C": C, "S": S, "select": sel,
           "speckle": {r: ST.speckle_keep(sel["d0"], sel["valid"], SPECKLE_SIZE, r) for r in (0, 1)},
           "full": ST.select(S, dmin, UNIQUENESS, LR_MAX, True, SPECKLE_SIZE, 1)}
    for v in out.values():
        for a in (v.values() if isinstance(v, dict) else [v]):
            a.setflags(write=False)
    return out


def flags_seen():
    """(bits set somewhere, bits clear somewhere) over the whole case list with the speckle filter on."""
    on = off = 0
    for p in CASES:
        for kind in KINDS:
            f = case(*p, kind)["full"]["flags"]
            on |= int(np.bitwise_or.reduce(f.reshape(-1)))
            off |= int(np.bitwise_or.reduce((~f & 7).reshape(-1)))
    return on, off


# ---- analytic scenes: a pinhole pair over a textured height field ---------------------------------------------------------------------------
SCENE_H, SCENE_W, SCENE_D, FOCAL, BASELINE = 48, 96, 32, 120.0, 8.0
SCENES = {
    "plane": lambda X, Y: 60.0 + 0.0 * X,
    "slant": lambda X, Y: 60.0 + 0.35 * X + 0.2 * Y,
    "bump": lambda X, Y: 70.0 + 0.25 * X - 14.0 * np.exp(-(X * X + Y * Y) / (2.0 * 9.0 ** 2)),
}


def _hash01(ix, iy, octave):
    """A value in [0, 1) per integer lattice point: an integer hash (fixed multipliers, xor-shifts), uint32 arithmetic."""
    h = (ix.astype(np.int64) * 374761393 + iy.astype(np.int64) * 668265263 + (octave + 1) * 2246822519) & 0xFFFFFFFF
    h = ((h ^ (h >> 13)) * 1274126177) & 0xFFFFFFFF
    h = (h ^ (h >> 16)) & 0xFFFFFFFF
    return h.astype(np.float64) / 4294967296.0


def texture(X, Y, cells=(0.5, 1.0, 2.0)):
    """Three octaves of hashed value noise over the surface coordinates (X, Y), equal amplitudes, bilinear; in [0, 1)."""
    out = np.zeros_like(X)
    for o, cell in enumerate(cells):
        u, v = X / cell, Y / cell
        iu, iv = np.floor(u), np.floor(v)
        fu, fv = u - iu, v - iv
        iu, iv = iu.astype(np.int64), iv.astype(np.int64)
        a, b = _hash01(iu, iv, o), _hash01(iu + 1, iv, o)
        c, d = _hash01(iu, iv + 1, o), _hash01(iu + 1, iv + 1, o)
        out += (a + fu * (b - a)) + fv * ((c + fu * (d - c)) - (a + fu * (b - a)))
    return out / len(cells)


def _view(z_of, cam_x, cells):
    """(uint8 image, z-depth) of the height field seen by the camera at (cam_x, 0, 0) looking along +z: per pixel the fixed point
    z <- z_of(X(z), Y(z)), 60 iterations."""
    j, i = np.meshgrid(np.arange(SCENE_W, dtype=np.float64), np.arange(SCENE_H, dtype=np.float64))
    rx, ry = (j - (SCENE_W - 1) / 2.0) / FOCAL, (i - (SCENE_H - 1) / 2.0) / FOCAL
    z = np.full_like(rx, 60.0)
    for _ in range(60):
        z = z_of(cam_x + rx * z, ry * z)
    X, Y = cam_x + rx * z, ry * z
    return np.minimum(np.floor(texture(X, Y, cells) * 256.0), 255).astype(np.uint8), z


@functools.lru_cache(maxsize=None)
def scene(name, cells=(0.5, 1.0, 2.0)):
    """dict(left, right uint8 [48,96]; truth: the disparity f b / z_left, fp64; depth: z_left)."""
    left, z = _view(SCENES[name], 0.0, cells)
    right, _ = _view(SCENES[name], BASELINE, cells)
    out = {"left": left, "right": right, "truth": FOCAL * BASELINE / z, "depth": z}
    for a in out.values():
        a.setflags(write=False)
    return out


def scene_errors(name, paths, cells=(0.5, 1.0, 2.0)):
    """``stereo_errors`` of the twin on a scene over the columns >= D, where the whole searched range lies in the image."""
    s = scene(name, cells)
    r = ST.stereo_disparity(s["left"], s["right"], SCENE_D, 0, P1, P2, paths, UNIQUENESS, LR_MAX, True)
    cols = np.zeros((SCENE_H, SCENE_W), bool)
    cols[:, SCENE_D:] = True
    return ST.stereo_errors(r["disparity"], r["valid"], s["truth"], cols, thresholds=(0.5, 1, 2, 3))
