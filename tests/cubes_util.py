"""Helpers of the cube-triangulation tests (meshing.marching_cubes, csrc/cubes.hip)."""
import numpy as np

from endosurf_amd.meshing import marching_cubes


def padded(u, value=1.0):
    """``u`` with one layer of outside points around it: the level set closes inside the grid."""
    return np.pad(np.asarray(u), 1, constant_values=value)


def edge_balance(tris):
    """(uses of every undirected edge, uses of every directed edge minus those of its reverse) of an indexed mesh."""
    f = np.asarray(tris, np.int64).reshape(-1, 3)
    a, b = np.concatenate([f[:, 0], f[:, 1], f[:, 2]]), np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    n = int(f.max()) + 1 if len(f) else 1
    _, inv = np.unique(np.minimum(a, b) * n + np.maximum(a, b), return_inverse=True)
    inv = inv.reshape(-1)
    return np.bincount(inv), np.bincount(inv, weights=np.where(a < b, 1.0, -1.0))


def euler_number(verts, tris):
    return len(verts) - len(edge_balance(tris)[0]) + len(tris)


def compare_with_twin(u, thr, verts, tris, ends):
    """Assert that (verts, tris, ends) -- numpy arrays of a device mesh -- is marching_cubes(u, thr): edge_ends and tris equal as arrays,
    order included, positions within 1 fp32 ulp of the twin's fp64 result (the criterion of iso_util.compare_with_host; NaN matches
    NaN).  No area exception: the orientation comes from the table on both sides.  Returns (V, T)."""
    hv, ht, he = marching_cubes(u, thr, return_ends=True)
    verts, tris, ends = np.asarray(verts), np.asarray(tris), np.asarray(ends)
    assert verts.dtype == np.float32 and verts.shape == (len(hv), 3), (verts.dtype, verts.shape, hv.shape)
    assert ends.shape == he.shape and np.array_equal(ends.astype(np.int64), he), "edge_ends differ"
    w32 = hv.astype(np.float32)
    ok = (np.abs(verts.astype(np.float64) - hv) <= np.spacing(np.abs(w32)).astype(np.float64)) | (np.isnan(verts) & np.isnan(hv))
    assert ok.all(), f"{(~ok).sum()} vertex coordinates off by more than 1 ulp"
    assert tris.shape == ht.shape and np.array_equal(tris.astype(np.int64), ht), "triangles differ"
    return len(hv), len(ht)
