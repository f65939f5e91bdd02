"""Stereo disparity by semi-global matching over a census cost: the numpy specification and twin of csrc/stereo.hip.

Input is a rectified pair; the left image is the reference view and a point at left column x appears in the right image at column
x - disparity, disparity >= 0.  Everything up to the sub-pixel step is integer arithmetic, and the sub-pixel step is one fp64 division
and one fp64 addition, so the kernels are held to these functions bit for bit.

  grey      uint8 [H,W]; uint8 RGB by (77 R + 150 G + 29 B + 128) >> 8; a float image in [0,1] by the rule of ``data.to8b`` first
  census    9 wide x 7 high, replicated border, bit = neighbour < centre, row-major, centre skipped, first neighbour = bit 61; int64
  cost      C[y,x,d] = popcount(cl[y,x] ^ cr[y, x - dmin - d]), 63 where that column is left of the image; uint8
  paths     L_r(p,d) = C(p,d) + min(L_r(p-r,d), L_r(p-r,d-1) + P1, L_r(p-r,d+1) + P1, m + P2) - m, m = min_k L_r(p-r,k); L_r = C where
            p - r is outside the image; S = sum over ``DIRECTIONS[:paths]``, uint16
  select    argmin (smallest d on ties), uniqueness, left-right consistency, parabola sub-pixel, speckle segments
"""
from __future__ import annotations

import numpy as np

CENSUS_W, CENSUS_H, CENSUS_BITS = 9, 7, 62
COST_OUTSIDE = 63
MAX_DISPARITIES, MAX_PENALTY, MAX_SIZE = 256, 1024, 8192
DIRECTIONS = ((0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (-1, -1), (1, -1), (-1, 1))          # (dy, dx); paths=4 takes the first four
FLAG_UNIQUENESS, FLAG_LEFT_RIGHT, FLAG_SPECKLE = 1, 2, 4
MATCHER_ARGS = ("min_disparity", "p1", "p2", "paths", "uniqueness", "lr_max", "subpixel", "speckle_size", "speckle_range")


def check_matcher(max_disparity, min_disparity=0, p1=7, p2=60, paths=8, uniqueness=10, lr_max=1, speckle_size=0, speckle_range=1):
    """The matcher's arguments as integers, or ValueError naming the one that is out of range (the library refuses the same)."""
    D, dmin, p1, p2, paths = int(max_disparity), int(min_disparity), int(p1), int(p2), int(paths)
    uniqueness, lr_max, speckle_size, speckle_range = int(uniqueness), int(lr_max), int(speckle_size), int(speckle_range)
    if not 1 <= D <= MAX_DISPARITIES:
        raise ValueError(f"max_disparity must be in [1, {MAX_DISPARITIES}] (got {D})")
    if not 0 <= dmin <= MAX_SIZE:          # (every min_disparity >= W already means "no column", so the bound loses nothing)
        raise ValueError(f"min_disparity must be in [0, {MAX_SIZE}] (got {dmin})")
    if not 0 <= p1 <= p2 <= MAX_PENALTY:
        raise ValueError(f"the penalties must satisfy 0 <= p1 <= p2 <= {MAX_PENALTY} (got p1 {p1}, p2 {p2})")
    if paths not in (4, 8):
        raise ValueError(f"paths must be 4 or 8 (got {paths})")
    if not 0 <= uniqueness <= 100:
        raise ValueError(f"uniqueness must be in [0, 100] (got {uniqueness})")
    if lr_max < 0 or speckle_size < 0 or speckle_range < 0:
        raise ValueError(f"lr_max, speckle_size and speckle_range must not be negative (got {lr_max}, {speckle_size}, {speckle_range})")
    return D, dmin, p1, p2, paths, uniqueness, lr_max, speckle_size, speckle_range


def to_grey(image) -> np.ndarray:
    """uint8 grey [..., H, W] of an image or a stack: uint8 [..., H, W] as it is, uint8 [..., H, W, 3] by the integer luma above, a float
    image (grey or RGB) in [0, 1] truncated to uint8 first by ``data.to8b``'s rule on fp32."""
    x = np.asarray(image)
    if np.issubdtype(x.dtype, np.floating):
        x = (np.float32(255) * np.clip(x.astype(np.float32), 0, 1)).astype(np.uint8)
    if x.dtype != np.uint8:
        raise ValueError(f"an image is uint8 or float in [0, 1] (got {x.dtype})")
    if x.ndim >= 3 and x.shape[-1] == 3:
        v = x.astype(np.int32)
        return ((77 * v[..., 0] + 150 * v[..., 1] + 29 * v[..., 2] + 128) >> 8).astype(np.uint8)
    return x


def census(grey) -> np.ndarray:
    """The 62-bit census signature of every pixel of uint8 ``grey`` [H,W] (or a stack [n,H,W]), int64."""
    g = np.asarray(grey)
    if g.dtype != np.uint8 or g.ndim not in (2, 3):
        raise ValueError(f"census takes uint8 grey [H, W] or [n, H, W] (got {g.dtype} {g.shape})")
    H, W = g.shape[-2:]
    ry, rx = CENSUS_H // 2, CENSUS_W // 2
    out = np.zeros(g.shape, np.int64)
    for j in range(-ry, ry + 1):
        ys = np.clip(np.arange(H) + j, 0, H - 1)
        for i in range(-rx, rx + 1):
            if i == 0 and j == 0:
                continue
            xs = np.clip(np.arange(W) + i, 0, W - 1)
            out = (out << 1) | (g[..., ys[:, None], xs[None, :]] < g)
    return out


def popcount64(a) -> np.ndarray:
    """Set bits of every element of an int64 / uint64 array, uint8."""
    b = np.ascontiguousarray(a).view(np.uint8).reshape(*np.shape(a), 8)
    return np.unpackbits(b, axis=-1).sum(-1, dtype=np.uint8)


def cost_volume(census_left, census_right, max_disparity, min_disparity=0) -> np.ndarray:
    """C [H,W,D] uint8 of two census images [H,W]."""
    cl, cr = np.asarray(census_left, np.int64), np.asarray(census_right, np.int64)
    H, W = cl.shape
    D, dmin = int(max_disparity), int(min_disparity)
    C = np.full((H, W, D), COST_OUTSIDE, np.uint8)
    for d in range(D):
        s = dmin + d
        if s < W:
            C[:, s:, d] = popcount64(cl[:, s:] ^ cr[:, :W - s])
    return C


def _step(prev, cost, p1, p2):
    """One step of the path recurrence on rows [..., D]: ``prev`` = L_r(p - r, .), ``cost`` = C(p, .), both int32."""
    m = prev.min(-1, keepdims=True)
    best = np.minimum(prev, m + p2)
    best[..., 1:] = np.minimum(best[..., 1:], prev[..., :-1] + p1)
    best[..., :-1] = np.minimum(best[..., :-1], prev[..., 1:] + p1)
    return cost + best - m


def path_costs(C, direction, p1=7, p2=60) -> np.ndarray:
    """L_r [H,W,D] int32 of one path direction (dy, dx) over the cost volume ``C`` [H,W,D]."""
    dy, dx = direction
    c = np.asarray(C).astype(np.int32)
    H, W, _ = c.shape
    L = np.empty_like(c)
    if dy == 0:
        xs = range(W) if dx > 0 else range(W - 1, -1, -1)
        for k, x in enumerate(xs):
            L[:, x] = c[:, x] if k == 0 else _step(L[:, x - dx], c[:, x], p1, p2)
        return L
    ys = range(H) if dy > 0 else range(H - 1, -1, -1)
    for k, y in enumerate(ys):
        if k == 0:
            L[y] = c[y]
            continue
        src = np.arange(W) - dx          # column of p - r
        inside = (src >= 0) & (src < W)
        L[y] = c[y]
        L[y, inside] = _step(L[y - dy, src[inside]], c[y, inside], p1, p2)
    return L


def aggregate(C, p1=7, p2=60, paths=8) -> np.ndarray:
    """S [H,W,D] uint16 = the sum of the path costs of ``DIRECTIONS[:paths]``; at most paths (max C + P2): 8 (63 + P2) for a census
    cost, 8 (255 + 1024) = 10232 for any byte volume."""
    S = np.zeros(np.shape(C), np.int32)
    for r in DIRECTIONS[:int(paths)]:
        S += path_costs(C, r, p1, p2)
    return S.astype(np.uint16)


def sgm_volume(left, right, max_disparity, min_disparity=0, p1=7, p2=60, paths=8) -> np.ndarray:
    """S of one pair [H,W,D] or of a stack [n,H,W,D], from images of any kind ``to_grey`` takes."""
    D, dmin, p1, p2, paths = check_matcher(max_disparity, min_disparity, p1, p2, paths)[:5]
    gl, gr = to_grey(left), to_grey(right)
    if gl.shape != gr.shape or gl.ndim not in (2, 3):
        raise ValueError(f"a pair is two images of one shape, [H, W(, 3)] or [n, H, W(, 3)] (got {gl.shape} and {gr.shape})")
    if gl.ndim == 3:
        return np.stack([sgm_volume(a, b, D, dmin, p1, p2, paths) for a, b in zip(gl, gr)]) if len(gl) else np.zeros((*gl.shape, D), np.uint16)
    return aggregate(cost_volume(census(gl), census(gr), D, dmin), p1, p2, paths)


def right_argmin(S, min_disparity=0) -> np.ndarray:
    """dR [H,W] int32: the argmin over d (smallest on ties) of S_R[y,x,d] = S[y, x + d + dmin, d] over the columns that exist; -1
    where none does."""
    S = np.asarray(S)
    H, W, D = S.shape
    big = np.iinfo(np.int32).max
    SR = np.full((H, W, D), big, np.int32)
    for d in range(D):
        s = int(min_disparity) + d
        if s < W:
            SR[:, :W - s, d] = S[:, s:, d]
    dR = SR.argmin(-1).astype(np.int32)
    dR[SR.min(-1) == big] = -1
    return dR


def speckle_keep(d0, valid, size, max_diff=1) -> np.ndarray:
    """bool [H,W]: the valid pixels whose segment has at least ``size`` pixels.  Segments join valid 4-neighbours whose ``d0`` differ
    by at most ``max_diff``.  Labels are propagated as the kernel does (the smallest pixel index of the segment wins), to the fixed point."""
    d0, valid = np.asarray(d0).astype(np.int64), np.asarray(valid, bool)
    H, W = valid.shape
    none = H * W
    label = np.where(valid, np.arange(H * W).reshape(H, W), none)
    links = []
    for ax in (0, 1):
        a = [slice(None)] * 2
        b = [slice(None)] * 2
        a[ax], b[ax] = slice(0, -1), slice(1, None)
        a, b = tuple(a), tuple(b)
        links.append((a, b, valid[a] & valid[b] & (np.abs(d0[a] - d0[b]) <= int(max_diff))))
    while True:
        new = label.copy()
        for a, b, ok in links:
            lo = np.where(ok, np.minimum(label[a], label[b]), none)
            new[a] = np.minimum(new[a], lo)
            new[b] = np.minimum(new[b], lo)
        if np.array_equal(new, label):
            break
        label = new
    counts = np.bincount(label.reshape(-1), minlength=none + 1)
    return valid & (counts[label] >= int(size))


def select(S, min_disparity=0, uniqueness=10, lr_max=1, subpixel=True, speckle_size=0, speckle_range=1) -> dict:
    """The disparity of every pixel from S [H,W,D] (module docstring; DESIGN.md 7q has the rules in full): dict(disparity [H,W] fp32,
    0 where not valid; valid bool; d0 int32, -1 where not valid; flags uint8, one bit per failed test)."""
    S = np.asarray(S)
    if S.dtype != np.uint16 or S.ndim != 3:
        raise ValueError(f"select takes S uint16 [H, W, D] (got {S.dtype} {S.shape})")
    H, W, D = S.shape
    dmin = int(min_disparity)
    Si = S.astype(np.int64)
    d0 = Si.argmin(-1)
    s0 = Si.min(-1)
    flags = np.zeros((H, W), np.uint8)
    far = np.abs(np.arange(D)[None, None, :] - d0[..., None]) > 1
    big = np.iinfo(np.int64).max
    s2 = np.where(far, Si, big).min(-1)
    fails = (s2 != big) & (s2 * (100 - int(uniqueness)) < s0 * 100)
    flags[fails] |= FLAG_UNIQUENESS
    dR = right_argmin(S, dmin)
    xr = np.arange(W)[None, :] - dmin - d0
    there = xr >= 0
    dr = dR[np.arange(H)[:, None], np.where(there, xr, 0)]
    ok = there & (dr >= 0) & (np.abs(d0 - dr) <= int(lr_max))
    flags[~ok] |= FLAG_LEFT_RIGHT
    valid = flags == 0
    if int(speckle_size) > 0:
        keep = speckle_keep(d0, valid, speckle_size, speckle_range)
        flags[valid & ~keep] |= FLAG_SPECKLE
        valid = keep
    delta = np.zeros((H, W), np.float64)
    if subpixel and D >= 3:
        inner = (d0 > 0) & (d0 < D - 1)
        dc = np.clip(d0, 1, D - 2)[..., None]
        a, b = np.take_along_axis(Si, dc - 1, -1)[..., 0], np.take_along_axis(Si, dc + 1, -1)[..., 0]
        den = a + b - 2 * s0
        use = inner & (den > 0)
        delta[use] = (a - b)[use].astype(np.float64) / (2 * den[use]).astype(np.float64)
    disparity = np.where(valid, ((dmin + d0).astype(np.float64) + delta).astype(np.float32), np.float32(0)).astype(np.float32)
    return {"disparity": disparity, "valid": valid, "d0": np.where(valid, d0, -1).astype(np.int32), "flags": flags}


def stereo_disparity(left, right, max_disparity, min_disparity=0, p1=7, p2=60, paths=8, uniqueness=10, lr_max=1, subpixel=True,
                     speckle_size=0, speckle_range=1) -> dict:
    """``select`` of ``sgm_volume`` for one pair ([H,W] results) or a stack [n,H,W(,3)] ([n,H,W] results)."""
    D, dmin, p1, p2, paths, uniqueness, lr_max, speckle_size, speckle_range = check_matcher(
        max_disparity, min_disparity, p1, p2, paths, uniqueness, lr_max, speckle_size, speckle_range)
    S = sgm_volume(left, right, D, dmin, p1, p2, paths)
    pick = lambda s: select(s, dmin, uniqueness, lr_max, subpixel, speckle_size, speckle_range)
    if S.ndim == 3:
        return pick(S)
    outs = [pick(s) for s in S]
    empty = {"disparity": np.float32, "valid": bool, "d0": np.int32, "flags": np.uint8}
    return {k: np.stack([o[k] for o in outs]) if outs else np.zeros(S.shape[:3], t) for k, t in empty.items()}


def stereo_errors(disparity, valid, truth, truth_valid=None, thresholds=(0.5, 1, 2, 3)) -> dict:
    """A quick evaluation against ground truth: density (valid pixels among those with truth), the mean absolute error over the pixels
    that are valid and have truth, and the share of those within each threshold (``within``: {threshold: share}).  nan where nothing
    is counted."""
    d, t = np.asarray(disparity, np.float64), np.asarray(truth, np.float64)
    have = np.ones(t.shape, bool) if truth_valid is None else np.asarray(truth_valid, bool)
    both = np.asarray(valid, bool) & have
    err = np.abs(d - t)[both]
    n = int(both.sum())
    nan = float("nan")
    return {"density": n / int(have.sum()) if have.any() else nan, "mean_abs_error": float(err.mean()) if n else nan,
            "within": {float(th): float((err <= th).mean()) if n else nan for th in thresholds}, "count": n}
