"""Helpers of the point-to-surface tests (tests/test_surface_host.py, tests/test_gpu_surface.py): an independently written fp64
point-triangle distance (Ericson's seven regions), triangle soups with queries aimed at every region, meshes whose answers are exact
ties, the sphere probe.  Every coordinate lies in [-1, 1]^3."""
import numpy as np

from endosurf_amd import meshing as M

D2_TOL = 2.0 ** -40          # fp64 error of ~20 operations on magnitudes up to L^2 <= 12 is below 2^-44 L^2; 16 x margin


def _dot(a, b):
    return (a * b).sum(-1)


def ericson_d2(query, vertices, triangles):
    """[Q, T] fp64 squared distances by the closest-point routine of C. Ericson, Real-Time Collision Detection, 5.1.5: the seven Voronoi
    regions of the triangle (three vertices, three edges, the face) told apart by the signs of d1 .. d6 and va, vb, vc.  Valid,
    non-degenerate triangles only."""
    p = np.asarray(query, np.float32).astype(np.float64)[:, None, :]
    v = np.asarray(vertices, np.float32).astype(np.float64)
    tri = np.asarray(triangles, np.int64)
    a, b, c = v[tri[:, 0]][None], v[tri[:, 1]][None], v[tri[:, 2]][None]
    ab, ac = b - a, c - a
    ap, bp, cp = p - a, p - b, p - c
    d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    with np.errstate(divide="ignore", invalid="ignore"):
        on_ab = a + (d1 / (d1 - d3))[..., None] * ab
        on_ac = a + (d2 / (d2 - d6))[..., None] * ac
        on_bc = b + ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[..., None] * (c - b)
        den = 1.0 / (va + vb + vc)
        on_face = a + ab * (vb * den)[..., None] + ac * (vc * den)[..., None]
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
    shape = np.broadcast_shapes(p.shape, a.shape)
    picks = [np.broadcast_to(x, shape) for x in (a, b, on_ab, c, on_ac, on_bc)]
    closest = np.select([k[..., None] for k in conds], picks, on_face)
    d = p - closest
    return _dot(d, d)


def region_queries(v, tri, height):
    """[len(tri), 7, 3]: for each triangle a point ``height`` above (along the normal) the face's centroid, a point outside each edge
    and a point beyond each vertex: one per Voronoi region."""
    a, b, c = (v[tri[:, k]].astype(np.float64) for k in range(3))
    n = np.cross(b - a, c - a)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    g = (a + b + c) / 3.0
    out = [g]
    for p0, p1 in ((a, b), (b, c), (c, a)):
        mid = 0.5 * (p0 + p1)
        out.append(mid + 0.3 * (mid - g))
    for p0 in (a, b, c):
        out.append(p0 + 0.3 * (p0 - g))
    return np.stack(out, 1) + height * n[:, None, :]


def soup(T, Q, seed):
    """T random triangles in [-0.5, 0.5]^3 (indexed: neighbours in the list share vertices) and Q queries in [-1, 1]^3: on vertices, in
    edge and face interiors, above each of the seven regions of some triangles, far outside the triangles' box, and uniform ones."""
    rng = np.random.default_rng(seed)
    V = T + 2
    v = rng.uniform(-0.5, 0.5, (V, 3)).astype(np.float32)
    tri = np.stack([np.arange(T), np.arange(T) + 1, np.arange(T) + 2], 1)
    tri[::3] = tri[::3, ::-1]                                            # both orientations
    tri[T // 2:] = rng.permutation(V)[tri[T // 2:]]                      # half of it without any order in the indices
    a, b, c = (v[tri[:, k]].astype(np.float64) for k in range(3))
    n_reg, n_each = 20, 30
    pick = rng.choice(T, n_reg, replace=False)
    qs = [region_queries(v, tri[pick], h).reshape(-1, 3) for h in (0.2,)]
    k = rng.choice(T, n_each, replace=False)
    qs.append(a[k])                                                       # on vertices
    qs.append(0.5 * (b[k] + c[k]))                                        # edge interiors
    w = rng.dirichlet(np.ones(3), n_each)
    qs.append(w[:, :1] * a[k] + w[:, 1:2] * b[k] + w[:, 2:] * c[k])       # face interiors
    far = rng.uniform(0.9, 1.0, (20, 3)) * rng.choice([-1.0, 1.0], (20, 3))
    qs.append(far)
    have = sum(len(x) for x in qs)
    assert have <= Q
    qs.append(rng.uniform(-1.0, 1.0, (Q - have, 3)))
    return v, tri.astype(np.int64), np.clip(np.concatenate(qs), -1.0, 1.0).astype(np.float32)


# ---- exact cases: dyadic coordinates, every product, sum and quotient of the rule is exact, so an answer is known to the last bit ------
NAN = float("nan")
_SQUARE = [[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]]
_HEX = [[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [-1, 0, 0], [-1, -1, 0], [0, -1, 0]]
_FAN = [[0, 1 + i, 1 + (i + 1) % 6] for i in range(6)]
_FAR = [[-1, -1, -1], [-1, -0.5, -1], [-0.5, -1, -1]]


def exact_cases():
    """name -> (vertices, triangles, queries, expected triangle [Q], expected d2 [Q], expected closest [Q, 3])."""
    out = {}

    def add(name, v, f, q, tri, d2, closest):
        out[name] = (np.asarray(v, np.float32).reshape(-1, 3), np.asarray(f, np.int64).reshape(-1, 3), np.asarray(q, np.float32).reshape(-1, 3),
                     np.asarray(tri, np.int32), np.asarray(d2, np.float64), np.asarray(closest, np.float32).reshape(-1, 3))

    above = [[0.5, 0.5, 1.0], [0.25, 0.25, 0.5]]          # above the diagonal 0-2 of the square: an edge of both triangles
    on = [[0.5, 0.5, 0], [0.25, 0.25, 0]]
    add("shared_edge", _SQUARE, [[0, 1, 2], [0, 2, 3]], above, [0, 0], [1.0, 0.25], on)
    add("shared_edge_swapped", _SQUARE, [[0, 2, 3], [0, 1, 2]], above, [0, 0], [1.0, 0.25], on)
    add("shared_edge_other_orientation", _SQUARE, [[2, 1, 0], [3, 0, 2]], above, [0, 0], [1.0, 0.25], on)
    # a far triangle first, then a closed fan around vertex 0: above (and below) its centre every fan triangle answers with vertex 0
    fan_v = _HEX + _FAR
    add("fan_centre", fan_v, [[7, 8, 9]] + _FAN, [[0, 0, 1.0], [0, 0, -0.5]], [1, 1], [1.0, 0.25], [[0, 0, 0], [0, 0, 0]])
    add("fan_centre_reversed", fan_v, [[7, 8, 9]] + _FAN[::-1], [[0, 0, 1.0]], [1], [1.0], [[0, 0, 0]])
    tri_v = [[0, 0, 0], [1, 0, 0], [0, 1, 0]]
    inside = [[0.25, 0.25, 0.5]]
    add("duplicates", tri_v, [[0, 1, 2], [0, 1, 2], [2, 0, 1], [1, 0, 2]], inside, [0], [0.25], [[0.25, 0.25, 0]])
    add("duplicates_reflected_first", tri_v, [[1, 0, 2], [0, 1, 2]], inside, [0], [0.25], [[0.25, 0.25, 0]])
    # three collinear corners with distinct indices: its three segments
    add("zero_area", [[0, 0, 0], [1, 0, 0], [0.5, 0, 0]], [[0, 1, 2]], [[0.25, 0, 1.0], [-1, 0, 0], [1, 0.5, 0], [0.75, 0, 0]],
        [0, 0, 0, 0], [1.0, 1.0, 0.25, 0.0], [[0.25, 0, 0], [0, 0, 0], [1, 0, 0], [0.75, 0, 0]])
    add("coincident_corners", [[0, 0, 0], [0, 0, 0], [0, 0, 0]], [[0, 1, 2]], [[0, 0, 1.0]], [0], [1.0], [[0, 0, 0]])
    # repeated, out-of-range and NaN-cornered triangles take no part; the one valid triangle (the fourth) answers
    skip_v = tri_v + [[NAN, 0, 0], [0.25, 0.25, 0.25]]
    add("skipped", skip_v, [[0, 0, 1], [0, 1, 5], [0, 1, -1], [0, 1, 2], [0, 1, 3], [2, 2, 2], [4, 4, 1]],
        [[0.25, 0.25, 0.25], [0.25, 0.25, -0.5]], [3, 3], [0.0625, 0.25], [[0.25, 0.25, 0], [0.25, 0.25, 0]])
    add("all_skipped", skip_v, [[0, 0, 1], [0, 1, 5], [0, 1, 3], [-7, 1, 2]], [[0.25, 0.25, 0.25]], [-1], [np.inf], [[NAN] * 3])
    add("nan_queries", tri_v, [[0, 1, 2]], [[NAN, 0, 0], [0.25, 0.25, 0.5], [0, np.inf, 0], [0, 0, -np.inf]], [-1, 0, -1, -1],
        [np.inf, 0.25, np.inf, np.inf], [[NAN] * 3, [0.25, 0.25, 0], [NAN] * 3, [NAN] * 3])
    add("no_triangles", tri_v, np.zeros((0, 3), np.int64), [[0.25, 0.25, 0.5]], [-1], [np.inf], [[NAN] * 3])
    add("no_vertices", np.zeros((0, 3)), [[0, 1, 2]], [[0.25, 0.25, 0.5]], [-1], [np.inf], [[NAN] * 3])
    add("no_queries", tri_v, [[0, 1, 2]], np.zeros((0, 3)), np.zeros(0), np.zeros(0), np.zeros((0, 3)))
    return out


def check_exact(name, got):
    """``got`` = (dist, triangle, closest) as numpy arrays against the case's known answer, to the last bit."""
    _, _, _, tri, d2, closest = exact_cases()[name]
    dist, arg, at = got
    assert dist.dtype == np.float32 and arg.dtype == np.int32 and at.dtype == np.float32, name
    assert dist.shape == tri.shape and arg.shape == tri.shape and at.shape == closest.shape, name
    assert np.array_equal(arg, tri), (name, arg, tri)
    assert np.array_equal(dist, np.sqrt(d2).astype(np.float32)), (name, dist)
    assert np.array_equal(at, closest, equal_nan=True), (name, at)


def sphere_probe():
    """The probe of DESIGN 7f: marching tetrahedra of a radius-0.5 sphere on a 33^3 lattice over [-1, 1]^3 (h = 1 / 16) and 1500 points
    exactly on the sphere (to fp32).  (vertices, triangles, queries, h)."""
    ax = np.linspace(-1, 1, 33)
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    v, f = M.marching_tetrahedra(np.ascontiguousarray(np.sqrt(x * x + y * y + z * z) - 0.5, np.float32), 0.0)
    h = 2.0 / 32
    v = (np.asarray(v, np.float64) * h - 1.0).astype(np.float32)
    q = np.random.default_rng(0).normal(size=(1500, 3))
    q = (0.5 * q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    return v, np.asarray(f, np.int64), q, h


def twin_bounds(q, v, f):
    """What the device is compared with, computed once per mesh: the twin's outputs, the dense matrix of squared distances, each query's
    smallest value and whether its best two distinct values differ by more than 2^-36 (the closest point is then compared)."""
    dist, arg, at, d2 = M.point_to_mesh(q, v, f, return_d2=True)
    best = d2.min(axis=1) if d2.shape[1] else np.full(len(q), np.inf)
    with np.errstate(invalid="ignore"):
        second = np.where(d2 > best[:, None], d2, np.inf).min(axis=1) if d2.shape[1] else best
        clear = np.isfinite(best) & (second - best > 2.0 ** -36)
    return {"dist": dist, "triangle": arg, "closest": at, "d2": d2, "best": best, "clear": clear}
