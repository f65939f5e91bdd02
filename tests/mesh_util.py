"""Helpers of the mesh clean-up tests (tests/test_mesh_host.py, tests/test_gpu_mesh.py): small fields and hand-made meshes, an
independent union-find labelling, an fp64 brute-force nearest neighbour."""
import numpy as np

from endosurf_amd.meshing import marching_tetrahedra
from iso_util import fields


def grid(shape):
    return np.meshgrid(*[np.linspace(-1, 1, n) for n in shape], indexing="ij")


def ball(x, y, z, c, r):
    return np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - r


def field(name, shape=(33, 33, 33)):
    """New analytic fields; the ones of iso_util.fields are passed through."""
    x, y, z = grid(shape)
    if name == "two_disjoint_spheres":          # different sizes, well apart
        u = np.minimum(ball(x, y, z, (-0.45, 0, 0), 0.4), ball(x, y, z, (0.55, 0.1, 0), 0.25))
    elif name == "sphere_and_floaters":          # one body, three floaters of a few cells each
        u = ball(x, y, z, (0, 0, 0), 0.55)
        for c in ((0.8, 0.8, 0.8), (-0.8, 0.75, -0.7), (0.78, -0.8, 0.1)):
            u = np.minimum(u, ball(x, y, z, c, 0.09))
    else:
        return fields(name, shape)
    return np.ascontiguousarray(u, np.float32)


def mt_mesh(name, shape=(33, 33, 33), thr=0.0):
    v, f = marching_tetrahedra(field(name, shape), thr)
    return v.astype(np.float32), f.astype(np.int64)


def fan(n_tris, first=0):
    """A fan of n_tris triangles around vertex ``first`` (n_tris + 2 vertices)."""
    i = np.arange(n_tris)
    return np.stack([np.full(n_tris, first), first + 1 + i, first + 2 + i], 1)


def strip(n, seed=None):
    """2 n triangles between two rows of n + 1 vertices; ``seed`` shuffles the vertex names (a chain with no order in its labels)."""
    i = np.arange(n)
    f = np.concatenate([np.stack([i, i + 1, i + n + 1], 1), np.stack([i + 1, i + n + 2, i + n + 1], 1)])
    if seed is not None:
        f = np.random.default_rng(seed).permutation(2 * n + 2)[f]
    return f


def hand_meshes():
    """name -> (vertices [V,3] float32, triangles [T,3] int64).  Vertex positions are arbitrary but distinct."""
    out = {}

    def add(name, tris, V):
        rng = np.random.default_rng(len(out))
        out[name] = (rng.normal(size=(V, 3)).astype(np.float32), np.asarray(tris, np.int64).reshape(-1, 3))

    add("degenerate", [[0, 1, 2], [2, 2, 3], [3, 4, 3], [5, 5, 5], [4, 5, 6], [6, 7, 8], [1, 2, 0]], 9)
    add("isolated_vertex", [[0, 1, 2], [1, 2, 4]], 6)                                   # 3 and 5 are used by nothing
    add("fans_touching_in_a_vertex", np.concatenate([fan(6, 0), fan(5, 7)]), 14)        # 7 = last vertex of the first fan
    add("nine_and_ten", np.concatenate([fan(9, 0), fan(10, 11)]), 23)                  # the 0.9 rule at its boundary
    add("eight_and_ten", np.concatenate([fan(10, 0), fan(8, 12)]), 22)
    add("big_label_first", np.concatenate([fan(3, 20), fan(7, 0), [[30, 31, 32]]]), 33)
    add("strip", strip(10000), 20002)
    add("strip_shuffled", strip(10000, seed=5), 20002)
    add("only_degenerate", [[0, 0, 1], [2, 2, 2]], 3)
    add("empty", np.zeros((0, 3), np.int64), 4)
    add("nothing", np.zeros((0, 3), np.int64), 0)
    return out


FIELD_CASES = [("two_disjoint_spheres", (33, 33, 33), 0.0), ("sphere_and_floaters", (33, 33, 33), 0.0), ("torus", (30, 33, 28), 0.0),
               ("two_spheres", (33, 33, 33), 0.0), ("ties", (24, 22, 25), 0.5), ("gyroid", (28, 28, 28), 0.3)]


def union_find(tris, V):
    """Labels by the textbook union-find (smaller root wins, so a root is the smallest index of its set)."""
    parent = list(range(V))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for a, b, c in np.asarray(tris).tolist():
        if a == b or b == c or a == c:
            continue
        for p, q in ((a, b), (b, c)):
            rp, rq = find(p), find(q)
            parent[max(rp, rq)] = min(rp, rq)
    return np.array([find(v) for v in range(V)], np.int64)


def expected_components(tris, V):
    """(vertex_label, triangle_label, component_triangles) from union_find."""
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    vl = union_find(tris, V)
    good = (tris[:, 0] != tris[:, 1]) & (tris[:, 1] != tris[:, 2]) & (tris[:, 0] != tris[:, 2])
    tl = np.where(good, vl[tris[:, 0]] if len(tris) else 0, -1)
    ct = np.bincount(tl[good], minlength=V)[:V] if V else np.zeros(0, np.int64)
    return vl, tl, ct


def nearest64(query, points):
    """fp64 brute force: (dist, index of the first minimum, relative gap between the best and the second best distance)."""
    q, p = np.asarray(query, np.float64).reshape(-1, 3), np.asarray(points, np.float64).reshape(-1, 3)
    ok = np.isfinite(p).all(1)
    dist, idx, gap = np.full(len(q), np.inf), np.full(len(q), -1, np.int64), np.full(len(q), np.inf)
    ids = np.nonzero(ok)[0]
    if len(ids) == 0:
        return dist, idx, gap
    rows = max(1, (1 << 22) // len(ids))
    for i0 in range(0, len(q), rows):
        d = np.sqrt(((q[i0:i0 + rows, None, :] - p[None, ids, :]) ** 2).sum(-1))
        d[np.isnan(d)] = np.inf
        k = np.argmin(d, 1)
        best = d[np.arange(len(k)), k]
        dist[i0:i0 + rows] = best
        idx[i0:i0 + rows] = np.where(np.isfinite(best), ids[k], -1)
        if len(ids) > 1:
            d[np.arange(len(k)), k] = np.inf
            with np.errstate(invalid="ignore", divide="ignore"):
                gap[i0:i0 + rows] = (d.min(1) - best) / np.maximum(best, 1e-300)
    return dist, idx, gap
