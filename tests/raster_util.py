"""Helpers of the rasteriser tests (tests/test_raster_host.py, tests/test_gpu_raster.py): cameras in the convention of data.get_rays, an
independent fp64 brute-force ray caster through get_rays' own rays, small meshes, and the coplanar fill-rule case."""
import numpy as np
import torch

from endosurf_amd import data as D
from endosurf_amd.meshing import marching_tetrahedra
from iso_util import fields


def camera(h, w, focal, eye=(0.0, 0.0, -2.0), rot=None):
    """(K [4,4], pose [4,4]) float64 tensors: principal point in the image centre, camera-to-world pose with rotation ``rot``."""
    K = torch.eye(4, dtype=torch.float64)
    K[0, 0] = K[1, 1] = focal
    K[0, 2], K[1, 2] = (w - 1) / 2.0, (h - 1) / 2.0
    pose = torch.eye(4, dtype=torch.float64)
    if rot is not None:
        pose[:3, :3] = torch.as_tensor(rot, dtype=torch.float64)
    pose[:3, 3] = torch.tensor(eye, dtype=torch.float64)
    return K, pose


def rotation(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx


def ray_cast(vertices, triangles, K, pose, h, w, chunk=1 << 22):
    """fp64 Moller-Trumbore of every pixel's get_rays ray against every triangle: (camera z of the nearest hit [h,w], inf where none;
    its triangle [h,w], -1).  Both faces count; nothing is culled or snapped."""
    rays = D.get_rays(K[None].double(), pose[None].double(), w, h)[0].reshape(-1, 6).numpy()
    o, d = rays[:, :3], rays[:, 3:]
    axis = pose[:3, 2].numpy()                                  # the camera's z axis in the world
    v = np.asarray(vertices, np.float64)
    f = np.asarray(triangles, np.int64).reshape(-1, 3)
    ok = (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    ids = np.nonzero(ok)[0]
    p0, e1, e2 = v[f[ids, 0]], v[f[ids, 1]] - v[f[ids, 0]], v[f[ids, 2]] - v[f[ids, 0]]
    best, arg = np.full(len(o), np.inf), np.full(len(o), -1, np.int64)
    rows = max(1, chunk // max(len(ids), 1))
    with np.errstate(divide="ignore", invalid="ignore"):
        for r0 in range(0, len(o) if len(ids) else 0, rows):
            dd, oo = d[r0:r0 + rows, None, :], o[r0:r0 + rows, None, :]
            pv = np.cross(dd, e2[None])
            det = (e1[None] * pv).sum(-1)
            tv = oo - p0[None]
            u = (tv * pv).sum(-1) / det
            qv = np.cross(tv, e1[None])
            vv = (dd * qv).sum(-1) / det
            t = (e2[None] * qv).sum(-1) / det
            hit = (np.abs(det) > 1e-300) & (u >= 0) & (vv >= 0) & (u + vv <= 1) & (t > 0)
            z = np.where(hit, t * (dd * axis[None, None]).sum(-1), np.inf)
            k = np.argmin(z, 1)
            zz = z[np.arange(len(k)), k]
            best[r0:r0 + rows] = zz
            arg[r0:r0 + rows] = np.where(np.isfinite(zz), ids[k], -1)
    return best.reshape(h, w), arg.reshape(h, w)


def box3(a, fn):
    """fn over the 3 x 3 neighbourhood of every pixel (edge pixels see their own value beyond the border)."""
    p = np.pad(a, 1, mode="edge")
    h, w = a.shape
    return fn(np.stack([p[i:i + h, j:j + w] for i in range(3) for j in range(3)]), 0)


def mt_world(name, n=33):
    """The marching-tetrahedra mesh of iso_util.fields(name) in world coordinates ([-1, 1]^3), float32 vertices."""
    v, f = marching_tetrahedra(fields(name, (n, n, n)), 0.0)
    return (v / (n - 1.0) * 2.0 - 1.0).astype(np.float32), f.astype(np.int64)


def tetrahedron():
    v = np.array([[0.0, -0.6, 0.3], [0.6, 0.5, 0.4], [-0.6, 0.5, 0.2], [0.05, 0.1, -0.6]], np.float32)
    f = np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]], np.int64)
    return v, f


def orient(a, b, c):
    return (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])


def fill_rule_case(seed, n_points=60, x0=2, x1=21, y0=3, y1=17):
    """A rectangle with corners on the pixel centres (x0, y0) .. (x1, y1), triangulated by inserting ``n_points`` random points of the
    1/256 lattice one by one, each strictly inside a triangle, which it splits in three; every third point is a pixel centre.  Integer
    arithmetic throughout.  Returns (xy [V,2] int32 fixed point, triangles [T,3] int64 with random winding, the rectangle in pixels)."""
    rng = np.random.default_rng(seed)
    S = 256
    pts = [(x0 * S, y0 * S), (x1 * S, y0 * S), (x1 * S, y1 * S), (x0 * S, y1 * S)]
    tris = [(0, 1, 2), (0, 2, 3)]
    tries = 0
    while len(pts) < 4 + n_points and tries < 100 * n_points:
        tries += 1
        if tries % 3 == 0:
            q = (int(rng.integers(x0 + 1, x1)) * S, int(rng.integers(y0 + 1, y1)) * S)
        else:
            q = (int(rng.integers(x0 * S + 1, x1 * S)), int(rng.integers(y0 * S + 1, y1 * S)))
        for k, (a, b, c) in enumerate(tris):
            s = [orient(pts[a], pts[b], q), orient(pts[b], pts[c], q), orient(pts[c], pts[a], q)]
            if all(e > 0 for e in s) or all(e < 0 for e in s):
                n = len(pts)
                pts.append(q)
                tris[k:k + 1] = [(a, b, n), (b, c, n), (c, a, n)]
                break
    f = np.array(tris, np.int64)
    flip = rng.random(len(f)) < 0.5
    f[flip] = f[flip][:, [0, 2, 1]]
    return np.array(pts, np.int32), f, (x0, x1, y0, y1)
