"""Helpers of the geodesic tests (tests/test_geodesic_host.py, tests/test_gpu_geodesic.py): meshes, the exact cases with their known
answers, an independently written scalar update applied in random order (Gauss-Seidel), a heap Dijkstra on the edge graph, rigid and
scaled tracks.  The sphere probes and their twin results are computed once and shared (``sphere_mesh``, ``twin_sphere``)."""
import functools
import heapq
import math

import numpy as np

from endosurf_amd import geodesic as G
from endosurf_amd import meshing as M

NAN, INF = float("nan"), float("inf")


def ulps(a, b):
    """Distance in fp32 units in the last place between two non-negative fp32 arrays (0 where both are +inf)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def grid_mesh(nx, ny=None, h=0.25, height=None):
    """An nx x ny grid of right triangles in the plane z = 0 (or z = height(x, y)), vertex i * ny + j at (i h, j h); each square is
    cut by the diagonal from (i, j) to (i + 1, j + 1)."""
    ny = nx if ny is None else ny
    gx, gy = np.meshgrid(np.arange(nx) * h, np.arange(ny) * h, indexing="ij")
    z = np.zeros_like(gx) if height is None else height(gx, gy)
    v = np.stack([gx, gy, z], -1).reshape(-1, 3).astype(np.float32)
    i = (np.arange(nx - 1)[:, None] * ny + np.arange(ny - 1)[None]).reshape(-1)
    f = np.concatenate([np.stack([i, i + ny, i + ny + 1], 1), np.stack([i, i + ny + 1, i + 1], 1)])
    return v, f.astype(np.int64)


def bumpy(nx, ny, h=0.0625):
    """A curved height field with dyadic coordinates (z a multiple of 1/64): the mesh of the track tests."""
    return grid_mesh(nx, ny, h, height=lambda x, y: np.round(8.0 * np.sin(3.0 * x) * np.cos(2.0 * y)) / 64.0)


@functools.lru_cache(maxsize=None)
def sphere_mesh(n, method="tetrahedra"):
    """``surface_util.sphere_probe``'s construction at n^3: the radius-0.5 sphere on a lattice over [-1, 1]^3, marching tetrahedra or
    cubes.  (vertices fp32, triangles int64, the index of the top vertex)."""
    ax = np.linspace(-1, 1, n)
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    u = np.ascontiguousarray(np.sqrt(x * x + y * y + z * z) - 0.5, np.float32)
    v, f = (M.marching_tetrahedra if method == "tetrahedra" else M.marching_cubes)(u, 0.0)
    v = (np.asarray(v, np.float64) * (2.0 / (n - 1)) - 1.0).astype(np.float32)
    return v, np.asarray(f, np.int64), int(np.argmax(v[:, 2]))


def great_circle(v, top, radius=0.5):
    """The exact distance on the sphere from vertex ``top`` to every vertex (each projected radially)."""
    d = v.astype(np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return radius * np.arccos(np.clip(d @ d[top], -1.0, 1.0))


@functools.lru_cache(maxsize=None)
def twin_sphere(n, method="tetrahedra"):
    """``mesh_geodesic`` from the top vertex of ``sphere_mesh(n, method)``, computed once."""
    v, f, top = sphere_mesh(n, method)
    return G.mesh_geodesic(v, f, np.array([top]))


def dijkstra(v, f, source):
    """Shortest paths along the edges of the mesh from vertex ``source`` (a binary heap), fp64 [V]."""
    v = np.asarray(v, np.float64)
    adj = [[] for _ in range(len(v))]
    for a, b in {(min(t[i], t[(i + 1) % 3]), max(t[i], t[(i + 1) % 3])) for t in np.asarray(f).tolist() for i in range(3)}:
        w = float(np.linalg.norm(v[a] - v[b]))
        adj[a].append((b, w))
        adj[b].append((a, w))
    dist = np.full(len(v), np.inf)
    dist[source] = 0.0
    heap = [(0.0, source)]
    while heap:
        d, i = heapq.heappop(heap)
        if d > dist[i]:
            continue
        for j, w in adj[i]:
            if d + w < dist[j]:
                dist[j] = d + w
                heapq.heappush(heap, (d + w, j))
    return dist


# ---- the update rule once more, scalar, applied in place in random order ---------------------------------------------------------------
def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def corner_table(v, f):
    """One row per (valid triangle, corner): (c, a, b, l1, l2, ok, q11, q12, q22) as Python numbers."""
    v = np.asarray(v, np.float32).astype(np.float64)
    rows = []
    for k in range(3):
        ic, ia, ib = f[:, k], f[:, (k + 1) % 3], f[:, (k + 2) % 3]
        e1, e2 = v[ia] - v[ic], v[ib] - v[ic]
        g11, g12, g22 = _dot(e1, e1), _dot(e1, e2), _dot(e2, e2)
        det = g11 * g22 - g12 * g12
        ok = det > (2.0 ** -40 * g11) * g22
        with np.errstate(divide="ignore", invalid="ignore"):
            rows += list(zip(ic.tolist(), ia.tolist(), ib.tolist(), np.sqrt(g11).tolist(), np.sqrt(g22).tolist(), ok.tolist(),
                             (g22 / det).tolist(), (-g12 / det).tolist(), (g11 / det).tolist()))
    return rows


def scalar_update(row, ua, ub):
    _, _, _, l1, l2, ok, q11, q12, q22 = row
    edge = min(ua + l1, ub + l2)
    if not ok or ua == INF or ub == INF:
        return edge
    r1, r2 = q11 + q12, q12 + q22
    A = r1 + r2
    B = r1 * ua + r2 * ub
    C = (ua * (q11 * ua + q12 * ub) + ub * (q12 * ua + q22 * ub)) - 1.0
    disc = B * B - A * C
    if not disc >= 0.0:
        return edge
    t = (B + math.sqrt(disc)) / A
    da, db = ua - t, ub - t
    if q11 * da + q12 * db > 0.0 or q12 * da + q22 * db > 0.0:
        return edge
    return min(max(t, ua, ub), edge)


def gauss_seidel(v, f, source, seed, max_passes=10000):
    """The fixed point of the same updates applied one at a time, in place, in an order shuffled anew for every pass.  fp64 [V]."""
    rows = corner_table(v, f)
    rng = np.random.default_rng(seed)
    u = [INF] * len(v)
    u[source] = 0.0
    for _ in range(max_passes):
        changed = False
        for r in rng.permutation(len(rows)).tolist():
            row = rows[r]
            ua, ub = u[row[1]], u[row[2]]
            if ua == INF and ub == INF:
                continue
            cand = scalar_update(row, ua, ub)
            if cand < u[row[0]]:
                u[row[0]] = cand
                changed = True
        if not changed:
            return np.array(u)
    raise AssertionError("the Gauss-Seidel variant did not settle")


# ---- exact cases: dyadic coordinates, every operation of the rule that decides a checked value is exact ----------------------------------
H = 0.25
_TRI = [[0, 0, 0], [0.5, 0, 0], [0, 0.5, 0]]


def exact_cases():
    """name -> (vertices, triangles, sources [S] vertex ids)."""
    gv, gf = grid_mesh(5, h=H)
    far = (np.asarray(_TRI) + [2.0, 2.0, 1.0]).tolist()
    junk = [[0, 0, 1], [0, 1, 27], [0, 1, -1], [3, 3, 3], [0, 1, 26], [1 << 20, 2, 3]]          # repeated, out of range, NaN-cornered (26)
    pad_v = np.concatenate([gv, [[0.5, 0.5, 1.0], [NAN, 0, 0]]]).astype(np.float32)                 # 25: isolated, 26: NaN
    pad_f = np.concatenate([junk[:3], gf[:7], junk[3:], gf[7:]]).astype(np.int64)
    return {
        "grid": (gv, gf, [0]),
        "disjoint": (np.asarray(_TRI + far, np.float32), np.array([[0, 1, 2], [3, 4, 5]]), [0]),
        "padded": (pad_v, pad_f, [0]),
        "source_off_mesh": (pad_v, pad_f, [25]),
        "source_nan_corner": (pad_v, pad_f, [26]),
        "source_out_of_range": (gv, gf, [25]),
        "no_triangles": (gv, np.zeros((0, 3), np.int64), [0]),
        "two_sources": (gv, gf, [0, 12]),
    }


def check_exact(name, solve):
    """``solve(vertices, triangles, sources)`` -> (distance [S,V] fp32 numpy, sweeps) against the case's known answer, to the last bit."""
    v, f, src = exact_cases()[name]
    d, sweeps = solve(v, f, np.asarray(src, np.int64))
    assert d.dtype == np.float32 and d.shape == (len(src), len(v)), name
    assert 1 <= sweeps, name
    if name in ("grid", "padded", "two_sources"):
        g = d[0, :25].reshape(5, 5)
        k = np.arange(5)
        assert np.array_equal(g[:, 0], (k * H).astype(np.float32)) and np.array_equal(g[0, :], (k * H).astype(np.float32)), (name, g)
        diag = np.cumsum([0.0] + [math.sqrt(2 * H * H)] * 4)                 # the diagonal edges, one after the other, added in fp64
        assert np.array_equal(g[k, k], diag.astype(np.float32)), (name, g)
        assert np.array_equal(g, g.T), name                                  # the mesh and the rule are symmetric about the diagonal
    if name == "padded":
        plain, _ = solve(*exact_cases()["grid"][:2], np.asarray([0], np.int64))
        assert np.array_equal(d[:, :25], plain) and np.isinf(d[0, 25:]).all(), name
    if name == "disjoint":
        assert d[0].tolist() == [0.0, 0.5, 0.5, INF, INF, INF], (name, d)
    if name in ("source_off_mesh", "source_nan_corner", "source_out_of_range", "no_triangles"):
        assert np.isinf(d).all() and (d > 0).all(), (name, d)
    if name == "two_sources":
        for s, i in enumerate(src):
            one, _ = solve(v, f, np.asarray([i], np.int64))
            assert np.array_equal(d[s:s + 1], one), (name, s)
        assert d[1, 12] == 0.0 and d[1, 0] == d[0, 12]


# ---- tracks of rigidly moved and scaled copies -------------------------------------------------------------------------------------------
ROT_Z = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])          # quarter turns: exact
ROT_X = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])


def rigid_track(v, f, scaled=False):
    """A ``track_mesh``-like dict of F = 3 frames: the mesh, a rotated and shifted copy (quarter turns, dyadic steps: exact) and
    either a second rigid copy or, with ``scaled``, the mesh scaled by 2 (exact)."""
    v = np.asarray(v, np.float64)
    second = v @ ROT_Z.T + [0.25, -0.5, 0.125]
    third = 2.0 * v if scaled else (v @ ROT_X.T) @ ROT_Z.T + [-0.375, 0.25, 0.5]
    return {"vertices": np.stack([v, second, third]).astype(np.float32), "triangles": f}
