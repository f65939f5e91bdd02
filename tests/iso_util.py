"""Helpers of the iso-surface tests: name mesh vertices by the grid edge they sit on, so that a mesh of the device extractor
(csrc/iso.hip) and one of the host extractor (endosurf_amd/meshing.py marching_tetrahedra) can be compared exactly."""
import numpy as np

from endosurf_amd.meshing import _CORNER, marching_tetrahedra


def host_keys(u, thr):
    """Sorted keys a * N + b (a the inside end, b the outside end, linear grid ids) of every crossing tetrahedron edge: the order of the
    vertices marching_tetrahedra returns (its np.unique over the same keys)."""
    u = np.asarray(u, np.float64)
    N = u.size
    inside = u < thr
    lin = np.arange(N, dtype=np.int64).reshape(u.shape)
    keys = []
    for d in range(1, 8):
        dx, dy, dz = _CORNER[d]
        sl = lambda a, lo: a[dx if lo else 0:a.shape[0] - (0 if lo else dx), dy if lo else 0:a.shape[1] - (0 if lo else dy),
                             dz if lo else 0:a.shape[2] - (0 if lo else dz)]
        ip, iq, p, q = sl(inside, False), sl(inside, True), sl(lin, False), sl(lin, True)
        cross = ip != iq
        a, b = np.where(ip, p, q)[cross], np.where(ip, q, p)[cross]
        keys.append(a * N + b)
    return np.sort(np.concatenate(keys)) if keys else np.zeros(0, np.int64)


def _rows(a):
    a = np.ascontiguousarray(a, np.int64)
    return a.view([("", np.int64)] * 3).reshape(-1)


def canonical(tris):
    """Each triangle rotated (orientation kept) so that its smallest index comes first."""
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    k = np.argmin(tris, axis=1)
    idx = (k[:, None] + np.arange(3)[None]) % 3
    return np.take_along_axis(tris, idx, axis=1)


def compare_with_host(u, thr, verts, tris, ends, area_tol=1e-9):
    """Assert that (verts, tris, ends) -- numpy arrays of a device-scheme mesh -- is marching_tetrahedra(u, thr): the same set of vertices
    (named by their edge), positions within 1 fp32 ulp of the host's fp64 result, the same set of oriented triangles.  Triangles of area
    < area_tol (index units) may differ; returns (V, T, number of such triangles)."""
    u = np.asarray(u)
    N = u.size
    hv, ht = marching_tetrahedra(u, thr)
    hk = host_keys(u, thr)
    assert len(hk) == len(hv), (len(hk), len(hv))
    ends = np.asarray(ends, np.int64).reshape(-1, 2)
    verts = np.asarray(verts).reshape(-1, 3)
    key = ends[:, 0] * N + ends[:, 1]
    assert len(key) == len(hk) and np.array_equal(np.sort(key), hk), "vertex sets differ"
    to_host = np.searchsorted(hk, key)
    assert verts.dtype == np.float32
    want = hv[to_host]
    w32 = want.astype(np.float32)
    ok = (np.abs(verts.astype(np.float64) - want) <= np.spacing(np.abs(w32)).astype(np.float64)) | (np.isnan(verts) & np.isnan(want))
    assert ok.all(), f"{(~ok).sum()} vertex coordinates off by more than 1 ulp"
    got = canonical(to_host[np.asarray(tris, np.int64).reshape(-1, 3)])
    ref = canonical(ht)
    assert len(got) == len(ref), (len(got), len(ref))
    diff = np.setxor1d(_rows(got), _rows(ref))
    if len(diff):
        d = diff.view(np.int64).reshape(-1, 3)
        p0, p1, p2 = hv[d[:, 0]], hv[d[:, 1]], hv[d[:, 2]]
        area = 0.5 * np.linalg.norm(np.cross(p1 - p0, p2 - p0), axis=1)
        assert np.nan_to_num(area, nan=0.0).max() < area_tol, f"{len(d)} triangles differ, largest area {area.max():.3e}"
    return len(hv), len(ht), len(diff)


def edge_use_counts(tris):
    """How many triangles use each undirected edge of an indexed mesh."""
    f = np.asarray(tris, np.int64).reshape(-1, 3)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    _, counts = np.unique(e[:, 0] * (f.max() + 1 if len(f) else 1) + e[:, 1], return_counts=True)
    return counts


def fields(name, shape, seed=0):
    """Analytic / random test fields on a grid of ``shape`` over [-1, 1]^3 (float32)."""
    ax = [np.linspace(-1, 1, n) for n in shape]
    x, y, z = np.meshgrid(*ax, indexing="ij")
    if name == "sphere":
        u = np.sqrt(x * x + y * y + z * z) - 0.6
    elif name == "torus":
        u = np.sqrt((np.sqrt(x * x + y * y) - 0.55) ** 2 + z * z) - 0.25
    elif name == "two_spheres":          # touching at the origin
        u = np.minimum(np.sqrt((x - 0.4) ** 2 + y * y + z * z), np.sqrt((x + 0.4) ** 2 + y * y + z * z)) - 0.4
    elif name == "gyroid":
        k = 2.5 * np.pi
        u = np.sin(k * x) * np.cos(k * y) + np.sin(k * y) * np.cos(k * z) + np.sin(k * z) * np.cos(k * x)
    elif name == "random":               # smooth random field: a few random Fourier modes
        rng = np.random.default_rng(seed)
        u = np.zeros_like(x)
        for _ in range(12):
            f = rng.uniform(-6, 6, 3)
            u += rng.normal() * np.sin(f[0] * x + f[1] * y + f[2] * z + rng.uniform(0, 6.28))
    elif name == "plane_on_grid":        # u == thr exactly on a plane of grid points (thr = 0)
        u = np.broadcast_to((np.arange(shape[0]) - shape[0] // 2).astype(np.float64)[:, None, None], shape).copy()
    elif name == "ties":                 # heavily quantised: many u == thr ties and degenerate triangles
        u = np.round(fields("random", shape, seed).astype(np.float64) * 2) / 2
    else:
        raise KeyError(name)
    return np.ascontiguousarray(u, np.float32)
