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


def pair(H, W, D, dmin, kind, seed=0, rng=None):
    """(left, right) uint8 [H,W].  noise: the left image is uniform noise, every row of the right image is that row of the left image
    shifted by one random disparity of the searched range (where it fits the row), with fresh noise where the shift leaves the image.
    constant: both images hold one value, so every argmin ties.  levels: as noise, with the three grey levels 0 / 100 / 200 only, for
    many ties.  ramp: left = (5 x + 3 y) % 256, the right image that ramp shifted row by row."""
    rng = np.random.default_rng([seed, H, W, D, dmin]) if rng is None else rng
    if kind == "constant":
        v = int(rng.integers(0, 256))
        return np.full((H, W), v, np.uint8), np.full((H, W), v, np.uint8)
    if kind == "ramp":
        y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        s = np.minimum(dmin + rng.integers(0, D, (H, 1)), max(W - 1, 0))
        return ((5 * x + 3 * y) % 256).astype(np.uint8), ((5 * (x + s) + 3 * y) % 256).astype(np.uint8)
    if kind == "levels":
        left, right = (100 * rng.integers(0, 3, (2, H, W))).astype(np.uint8)
    else:
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


# ---- the argument sweep: every stage on inputs from the whole space the contract admits ------------------------------------------------------
SWEEP_D = (1, 2, 3, 4, 5, 16, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256)
SWEEP_PENALTIES = (0, 1, 7, 60, 61, 1023, 1024)
SWEEP_KINDS = ("noise", "constant", "levels", "ramp")
SWEEP_DRAWN = 48
SWEEP_MAX_CELLS = 60000


def _draw(i):
    """Configuration i: (H, W, D, dmin, p1, p2, paths, uniqueness, lr_max, speckle_size, speckle_range, kind)."""
    rng = np.random.default_rng([2026, i])
    pick = lambda values: values[int(rng.integers(0, len(values)))]
    D = pick(SWEEP_D)
    H = int(rng.integers(1, 25))
    W = int(rng.integers(1, min(140, SWEEP_MAX_CELLS // (H * D)) + 1))
    dmin = pick((0, 1, 3, W - 1, W, W + 5))
    p1, p2 = sorted((pick(SWEEP_PENALTIES), pick(SWEEP_PENALTIES)))
    return (H, W, D, dmin, p1, p2, pick((4, 8)), pick((0, 1, 10, 50, 99, 100)), pick((0, 1, 2, D, 1000)),
            pick((0, 1, 2, 8, H * W, H * W + 1)), pick((0, 1, 2, 300)), pick(SWEEP_KINDS))


# the draws cover all that test_stereo_host.test_sweep_covers_what_it_claims asks for; a hand-chosen configuration would be appended here
SWEEP = [_draw(i) for i in range(SWEEP_DRAWN)]


def sweep_id(q):
    H, W, D, dmin, p1, p2, paths, uniqueness, lr_max, size, srange, kind = q
    return f"{H}x{W}x{D}-dmin{dmin}-P{p1}.{p2}-p{paths}-u{uniqueness}-lr{lr_max}-s{size}.{srange}-{kind}"


@functools.lru_cache(maxsize=None)
def sweep_case(i):
    """The pair of ``SWEEP[i]`` and everything the twin makes of it (read-only)."""
    H, W, D, dmin, p1, p2, paths, uniqueness, lr_max, size, srange, kind = SWEEP[i]
    left, right = pair(H, W, D, dmin, kind, rng=np.random.default_rng([2026, 1000 + i]))
    cl, cr = ST.census(left), ST.census(right)
    C = ST.cost_volume(cl, cr, D, dmin)
    S = ST.aggregate(C, p1, p2, paths)
    out = {"left": left, "right": right, "census_left": cl, "census_right": cr, "C": C, "S": S, "dR": ST.right_argmin(S, dmin),
           "select": ST.select(S, dmin, uniqueness, lr_max, True), "select_whole": ST.select(S, dmin, uniqueness, lr_max, False),
           "full": ST.select(S, dmin, uniqueness, lr_max, True, size, srange)}
    for v in out.values():
        for a in (v.values() if isinstance(v, dict) else [v]):
            a.setflags(write=False)
    return out


def path_costs_scalar(C, direction, p1, p2):
    """L_r [H,W,D] of one direction as a list of lists of lists of Python integers, pixel by pixel and disparity by disparity from the
    formula in include/endosurf_hip.h: L_r(p,d) = C(p,d) + min(L_r(p-r,d), L_r(p-r,d-1) + p1, L_r(p-r,d+1) + p1, m + p2) - m with
    m = min_k L_r(p-r,k), d -+ 1 outside [0, D) left out, L_r = C where p - r is outside the image."""
    H, W, D = len(C), len(C[0]), len(C[0][0])
    dy, dx = direction
    L = [[None] * W for _ in range(H)]
    for y in (range(H) if dy >= 0 else range(H - 1, -1, -1)):          # p - r is always visited before p
        for x in (range(W) if dx >= 0 else range(W - 1, -1, -1)):
            py, px = y - dy, x - dx
            if not (0 <= py < H and 0 <= px < W):
                L[y][x] = [int(C[y][x][d]) for d in range(D)]
                continue
            prev = L[py][px]
            m = min(prev)
            L[y][x] = []
            for d in range(D):
                terms = [prev[d], m + p2]
                if d - 1 >= 0:
                    terms.append(prev[d - 1] + p1)
                if d + 1 < D:
                    terms.append(prev[d + 1] + p1)
                L[y][x].append(int(C[y][x][d]) + min(terms) - m)
    return L


def saturating_volume():
    """13 x 13 x 4 bytes, 0 at d = 0 and 255 elsewhere: with P1 = P2 = 1024 every path that has a predecessor costs 255 + 1024 at d >= 1,
    and the centre pixel has one in all eight directions."""
    C = np.full((13, 13, 4), 255, np.uint8)
    C[..., 0] = 0
    return C


SELECT_VOLUMES = ("uniform", "edge", "max", "high")
SELECT_D = (1, 2, 3, 64, 65, 256)
SELECT_H, SELECT_W = 3, 70          # wider than 65 disparities, so the right view's argmin sees columns at every d of four of the six D


def select_volume(kind, D):
    """S uint16 [3,70,D] over the whole uint16 range: uniform over [0, 65535]; only 32767 and 32768 (the two sides of a signed 16-bit
    edge); all 65535; uniform over [32768, 65535] (every row's minimum is at least 2^15)."""
    rng = np.random.default_rng([2026, 200 + 10 * SELECT_VOLUMES.index(kind) + SELECT_D.index(D)])
    shape = (SELECT_H, SELECT_W, D)
    if kind == "uniform":
        return rng.integers(0, 65536, shape).astype(np.uint16)
    if kind == "edge":
        return (32767 + rng.integers(0, 2, shape)).astype(np.uint16)
    if kind == "max":
        return np.full(shape, 65535, np.uint16)
    return rng.integers(32768, 65536, shape).astype(np.uint16)


def speckle_fields():
    """The hand-made fields of the speckle tests: (name, d0 int32 [H,W], valid bool [H,W], size, range, expected keep or None)."""
    out = []
    snake = np.zeros((9, 31), bool)
    snake[0::2] = True
    snake[1::4, 30] = snake[3::4, 0] = True          # one segment of 5 * 31 + 4 = 159 pixels
    for size, kept in ((159, snake), (160, np.zeros_like(snake))):
        out.append((f"snake-{size}", np.zeros((9, 31), np.int32), snake, size, 0, kept))
    y, x = np.meshgrid(np.arange(7), np.arange(10), indexing="ij")
    board = (x + y) % 2 == 0
    out.append(("checkerboard-1", np.zeros((7, 10), np.int32), board, 1, 1, board))
    out.append(("checkerboard-2", np.zeros((7, 10), np.int32), board, 2, 1, np.zeros_like(board)))
    stairs = np.tile(np.array([0, 0, 1, 1, 3, 3, 3, 6, 6, 8, 9, 10], np.int32), (3, 1))
    cols = lambda *values: np.tile(np.isin(stairs[0], values), (3, 1))
    # range 0: segments of 6, 6, 9, 6, 3, 3, 3 pixels; range 1: 12, 9, 6, 9; range 2: 21 and 15
    out.append(("staircase-0", stairs, np.ones((3, 12), bool), 5, 0, cols(0, 1, 3, 6)))
    out.append(("staircase-1", stairs, np.ones((3, 12), bool), 7, 1, cols(0, 1, 3, 8, 9, 10)))
    out.append(("staircase-2", stairs, np.ones((3, 12), bool), 16, 2, cols(0, 1, 3)))
    extreme = np.array([[2 ** 31 - 1, -2 ** 31, 5, 6]], np.int32)          # the first two differ by 2^32 - 1, which wraps to 1 in int32
    kept = np.array([[False, False, True, True]])
    out.append(("extreme-row", extreme, np.ones((1, 4), bool), 2, 1, kept))
    out.append(("extreme-column", extreme.T.copy(), np.ones((4, 1), bool), 2, 1, kept.T.copy()))
    rng = np.random.default_rng([2026, 300])
    some = rng.uniform(size=(11, 14)) < 0.6
    out.append(("size-0", rng.integers(-1, 4, (11, 14)).astype(np.int32), some, 0, 1, some))
    return out


def speckle_stack():
    """(d0 [2,4,5], valid, {size: expected keep}): the last row of the first image and the first row of the second are valid with equal
    d0, and so are the last pixel of a row and the first pixel of the next, twice.  Segments: two rows of 5 and four single pixels."""
    rows = np.zeros((2, 4, 5), bool)
    rows[0, 3] = rows[1, 0] = True
    single = np.zeros_like(rows)
    single[0, 0, 4] = single[0, 1, 0] = single[1, 2, 4] = single[1, 3, 0] = True
    return np.full((2, 4, 5), 4, np.int32), rows | single, {1: rows | single, 2: rows, 6: np.zeros_like(rows)}


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
