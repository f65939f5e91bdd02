"""Depth fusion: what the depth frames alone say the surface is, and which parts of a mesh were ever observed.

A truncated signed distance (TSDF) volume is the classical answer of RGB-D pipelines: every voxel is projected into every depth frame
and averages the truncated difference between the measured depth and its own.  It needs no training, and it is the baseline a learned
surface is compared with.  On a deforming scene plain fusion over time is wrong; the model removes exactly that obstacle: two observed
points are the same tissue when they share x_c = x + D(x, t), so the frames are fused in CANONICAL space, each canonical voxel carried
to the frame's time by ``tracking.to_observed`` before it is projected (``fuse_depth`` with a ``deform_fn``).  The weight volume of the
fusion -- how many frames saw this piece of tissue near the measured depth -- sampled at a mesh's canonical vertices is a per-vertex
coverage map (``sample_volume``; the renderer's ``mesh_coverage``).

numpy; fp64 where stated.  ``integrate``, ``finalize`` and ``sample_volume`` are the specification of the device kernels (csrc/fuse.hip,
DESIGN.md 7p), and the renderer's methods of the same names pass those kernels the same arguments.

What the volume is and is not.  The zero level set is carried exactly by the map: a canonical voxel has s = 0 in a frame exactly when its
observed position lies on the measured surface.  The VALUES are observed-space z-distances along the camera axis (projective, not
Euclidean), so in canonical space the truncation band is stretched by the deformation's Jacobian J: ``trunc`` bounds the band in
observed space only.  Depth is taken at the nearest pixel (no interpolation across depth edges) and every observation weighs 1.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import meshing, tracking

STATE_KEYS = ("tsdf_sum", "weight", "color_sum")
AMBIGUOUS_EPS = 1e-9


def new_state(N, with_color=True):
    """Zeroed state of N voxels: dict(tsdf_sum [N], weight [N], color_sum [N,3] or None), fp32.  The state holds SUMS, not running
    averages: an update is three plain additions, with no multiply for a compiler to fuse, and the same bits come out however the frames
    are split into calls."""
    return {"tsdf_sum": np.zeros(N, np.float32), "weight": np.zeros(N, np.float32),
            "color_sum": np.zeros((N, 3), np.float32) if with_color else None}


def check_trunc(trunc, depth_trunc=math.inf):
    """(trunc, depth_trunc) as Python floats: trunc finite and positive, depth_trunc positive (it may be infinite)."""
    trunc, depth_trunc = float(trunc), float(depth_trunc)
    if not (0.0 < trunc < math.inf):
        raise ValueError(f"trunc must be finite and positive (got {trunc})")
    if not depth_trunc > 0.0:
        raise ValueError(f"depth_trunc must be positive (got {depth_trunc})")
    return trunc, depth_trunc


def _frames(positions, valid, depth, color, mask, cameras):
    pos = np.asarray(positions, np.float32)
    dep = np.asarray(depth, np.float32)
    cam = np.asarray(cameras, np.float64)
    if dep.ndim != 3 or cam.shape != (dep.shape[0], 17):
        raise ValueError(f"depth must be [F, H, W] and cameras [F, 17] (got {dep.shape}, {cam.shape})")
    F = dep.shape[0]
    if pos.ndim not in (2, 3) or pos.shape[-1] != 3 or (pos.ndim == 3 and pos.shape[0] != F):
        raise ValueError(f"positions must be [N, 3] or [{F}, N, 3] (got {pos.shape})")
    N = pos.shape[-2]
    if valid is not None:
        valid = np.asarray(valid) != 0
        if valid.shape != (F, N):
            raise ValueError(f"valid must be [{F}, {N}] (got {valid.shape})")
    if color is not None:
        color = np.asarray(color, np.float32)
        if color.shape != dep.shape + (3,):
            raise ValueError(f"color must be {dep.shape + (3,)} (got {color.shape})")
    if mask is not None:
        mask = np.asarray(mask) != 0
        if mask.shape != dep.shape:
            raise ValueError(f"mask must be {dep.shape} (got {mask.shape})")
    return pos, valid, dep, color, mask, cam, F, N


def _project(p32, cam, H, W):
    """One frame of the rule: (z, u, v, in_image, i, j) of fp32 points [N,3] in fp64, ``meshing.project_vertices``' expressions; the
    pixel indices are 0 where ``in_image`` is false."""
    x = p32.astype(np.float64)
    with np.errstate(all="ignore"):
        d = [x[:, k] - cam[9 + k] for k in range(3)]
        q = [(cam[k] * d[0] + cam[3 + k] * d[1]) + cam[6 + k] * d[2] for k in range(3)]
        z = q[2]
        u = (cam[12] * q[0] + cam[13] * q[1]) / z + cam[14]
        v = cam[15] * q[1] / z + cam[16]
        fj, fi = np.floor(u + 0.5), np.floor(v + 0.5)
        ok = (z > 0) & (fj >= 0) & (fj <= W - 1) & (fi >= 0) & (fi <= H - 1)          # (false for NaN)
    j = np.where(ok, fj, 0.0).astype(np.int64)
    i = np.where(ok, fi, 0.0).astype(np.int64)
    return z, u, v, ok, i, j


def integrate(state, positions, valid, depth, color, mask, cameras, trunc, depth_trunc=math.inf):
    """One block of frames into ``state`` (``new_state``'s dict, updated in place and returned).

    ``positions`` [N,3] (one lattice for all frames) or [F,N,3] (per-frame positions: the warped lattice), read as fp32; ``valid`` None
    or [F,N], a false row is skipped for that frame; ``depth`` [F,H,W] fp32 z-depth (the convention of ``data.depth_points``); ``color``
    [F,H,W,3] fp32 or None (exactly when the state has no ``color_sum``); ``mask`` [F,H,W] or None, 0 = ignore the pixel; ``cameras``
    ``flow.camera_table``'s [F,17].  Per voxel, the frames in index order:

      q = R^T (p - t), z = q_z; skip unless z > 0.
      u = (K00 q_x + K01 q_y) / z + K02, v = K11 q_y / z + K12, in fp64: ``meshing.project_vertices``' expressions.
      j = floor(u + 0.5), i = floor(v + 0.5): the nearest pixel; skip unless 0 <= j <= W - 1 and 0 <= i <= H - 1.
      d = depth[f, i, j]; skip unless d is finite, d > 0, d <= depth_trunc and the mask is non-zero there.
      s = d - z in fp64; skip if s < -trunc (behind the measured surface by more than the band: no evidence).
      tsdf_sum += fp32(min(1, s / trunc)); color_sum += color[f, i, j]; weight += 1 -- three plain fp32 additions.
    """
    trunc, depth_trunc = check_trunc(trunc, depth_trunc)
    pos, valid, dep, color, mask, cam, F, N = _frames(positions, valid, depth, color, mask, cameras)
    if (color is None) != (state.get("color_sum") is None):
        raise ValueError("color and the state's color_sum go together")
    ts, wt, cs = state["tsdf_sum"], state["weight"], state.get("color_sum")
    if ts.shape != (N,) or wt.shape != (N,) or ts.dtype != np.float32 or wt.dtype != np.float32:
        raise ValueError(f"the state must hold fp32 [{N}] sums (got {ts.shape} {ts.dtype}, {wt.shape} {wt.dtype})")
    H, W = dep.shape[1:]
    one = np.float32(1.0)
    for f in range(F):
        z, _, _, ok, i, j = _project(pos[f] if pos.ndim == 3 else pos, cam[f], H, W)
        d = dep[f][i, j]
        with np.errstate(all="ignore"):
            ok = ok & np.isfinite(d) & (d > 0) & (d.astype(np.float64) <= depth_trunc)
            if valid is not None:
                ok = ok & valid[f]
            if mask is not None:
                ok = ok & mask[f][i, j]
            s = d.astype(np.float64) - z
            ok = ok & ~(s < -trunc)
            term = np.minimum(1.0, s / trunc).astype(np.float32)
        ts[ok] = ts[ok] + term[ok]
        wt[ok] = wt[ok] + one
        if cs is not None:
            cs[ok] = cs[ok] + color[f][i, j][ok]
    return state


def ambiguous_rows(positions, valid, depth, cameras, trunc, eps=AMBIGUOUS_EPS):
    """[N] bool: the voxels for which, in any frame, a decision of ``integrate`` hangs on the last bits of an fp64 expression --
    u + 0.5 or v + 0.5 within ``eps`` of an integer, |z| < eps, or |s + trunc| < eps trunc at the pixel the twin reads.  Comparisons of
    another implementation against this twin leave such rows out."""
    pos, valid, dep, _, _, cam, F, N = _frames(positions, valid, depth, None, None, cameras)
    trunc = float(trunc)
    H, W = dep.shape[1:]
    amb = np.zeros(N, bool)
    for f in range(F):
        z, u, v, ok, i, j = _project(pos[f] if pos.ndim == 3 else pos, cam[f], H, W)
        with np.errstate(all="ignore"):
            a = np.abs(z) < eps
            for w in (u + 0.5, v + 0.5):
                a |= np.isfinite(w) & (np.abs(w - np.rint(w)) < eps)
            d = dep[f][i, j].astype(np.float64)
            a |= ok & np.isfinite(d) & (np.abs((d - z) + trunc) < eps * trunc)
        amb |= a if valid is None else (a & valid[f])
    return amb


def finalize(state):
    """dict(tsdf [N] = tsdf_sum / weight where weight > 0, else +1; color [N,3] likewise, else 0 (None without colour); weight [N]),
    fp32 divisions."""
    ts, wt, cs = state["tsdf_sum"], state["weight"], state.get("color_sum")
    seen = wt > 0
    safe = np.where(seen, wt, np.float32(1.0))
    out = {"tsdf": np.where(seen, ts / safe, np.float32(1.0)).astype(np.float32), "weight": wt.copy(), "color": None}
    if cs is not None:
        out["color"] = np.where(seen[:, None], cs / safe[:, None], np.float32(0.0)).astype(np.float32)
    return out


# ---- the lattice -------------------------------------------------------------------------------------------------------------------------
def lattice_axes(bound_min, bound_max, resolution, device="cpu"):
    """The three ``torch.linspace`` axes of the extraction lattice: ``renderer_mesh._Lattice``'s own expressions."""
    from .renderer_mesh import _Lattice
    return _Lattice(bound_min, bound_max, int(resolution), device).axes()


def lattice_points(axes, start=0, stop=None):
    """Rows ``start:stop`` of the lattice's points [R^3, 3], x-major: the LAST axis runs fastest, so neighbouring rows are neighbours
    along z."""
    R = [int(a.shape[0]) for a in axes]
    n = R[0] * R[1] * R[2]
    stop = n if stop is None else min(int(stop), n)
    idx = torch.arange(int(start), stop, device=axes[0].device)
    iz, iy, ix = idx % R[2], (idx // R[2]) % R[1], idx // (R[1] * R[2])
    return torch.stack([axes[0][ix], axes[1][iy], axes[2][iz]], -1)


def _bounds64(bound_min, bound_max):
    lo = torch.as_tensor(bound_min, dtype=torch.float32).cpu().double().reshape(3).numpy()
    hi = torch.as_tensor(bound_max, dtype=torch.float32).cpu().double().reshape(3).numpy()
    return lo, hi


def default_trunc(bound_min, bound_max, resolution):
    """4 x the largest cell side of the lattice, in fp64 on the fp32 bounds."""
    lo, hi = _bounds64(bound_min, bound_max)
    return 4.0 * float(((hi - lo) / (float(resolution) - 1.0)).max())


def check_fuse_args(resolution, voxel_chunk, frame_block, F, *per_frame):
    R, vc, fb = int(resolution), int(voxel_chunk), int(frame_block)
    if R < 2 or vc < 1 or fb < 1:
        raise ValueError(f"resolution must be at least 2 and voxel_chunk, frame_block at least 1 (got {resolution}, {voxel_chunk}, {frame_block})")
    for a in per_frame:
        if a is not None and a.shape[0] != F:
            raise ValueError(f"{F} depth frames take {F} poses, times, colours and masks (got {a.shape[0]})")
    return R, vc, fb


def fuse_depth(deform_fn, depths, colors, masks, intrinsics, poses, times, bound_min, bound_max, resolution, trunc=None,
               depth_trunc=math.inf, max_iters=64, tol=1e-6, voxel_chunk=1 << 18, frame_block=8):
    """The TSDF volume of ``depths`` [F,H,W] (with ``colors`` [F,H,W,3] and ``masks`` [F,H,W], each or None) seen by the cameras
    ``intrinsics`` ([3,3] / [4,4], or one per frame) and ``poses`` [F,4,4] at ``times`` [F], on the resolution^3 lattice of (bound_min,
    bound_max).  With a ``deform_fn`` the lattice is CANONICAL: each chunk of ``voxel_chunk`` voxels is carried to every frame's time of
    a block of ``frame_block`` frames by ``tracking.to_observed`` (in fp64, with ``max_iters`` and ``tol``), rows that did
    not converge are ``valid = False`` for that frame, and the block is integrated; ``deform_fn=None`` fuses in place (a static scene).
    ``trunc=None``: ``default_trunc``.  The chunking changes no bit of the result.

    dict(tsdf [R,R,R], weight [R,R,R], color [R,R,R,3] or None, trunc, bound_min, bound_max (fp64 [3] of the fp32 bounds), space =
    "canonical" or "static")."""
    from . import flow
    dep = np.asarray(depths, np.float32)
    F = dep.shape[0]
    col = None if colors is None else np.asarray(colors, np.float32)
    msk = None if masks is None else np.asarray(masks)
    tt = np.asarray(times, np.float64).reshape(-1)
    R, vc, fb = check_fuse_args(resolution, voxel_chunk, frame_block, F, tt, col, msk)
    table, shared = flow.camera_table(intrinsics, poses)
    if shared or table.shape[0] != F:
        raise ValueError(f"{F} depth frames take poses [{F}, 4, 4] (got {table.shape[0]} camera(s))")
    trunc, depth_trunc = check_trunc(default_trunc(bound_min, bound_max, R) if trunc is None else trunc, depth_trunc)
    axes = lattice_axes(bound_min, bound_max, R)
    N = R * R * R
    state = new_state(N, col is not None)
    for n0 in range(0, N, vc):
        pts = lattice_points(axes, n0, n0 + vc)
        n = pts.shape[0]
        part = {k: (None if state[k] is None else state[k][n0:n0 + n]) for k in STATE_KEYS}
        for f0 in range(0, F, fb):
            sl = slice(f0, min(f0 + fb, F))
            nb = sl.stop - sl.start
            if deform_fn is None:
                pos, valid = pts.numpy(), None
            else:
                tb = torch.as_tensor(tt[sl], dtype=torch.float64)
                ob = tracking.to_observed(deform_fn, pts.double().repeat(nb, 1), tb.repeat_interleave(n), None, max_iters, tol)
                pos = ob["points"].float().reshape(nb, n, 3).numpy()
                valid = ob["converged"].reshape(nb, n).numpy()
            integrate(part, pos, valid, dep[sl], None if col is None else col[sl], None if msk is None else msk[sl], table[sl], trunc,
                      depth_trunc)
    out = finalize(state)
    lo, hi = _bounds64(bound_min, bound_max)
    return {"tsdf": out["tsdf"].reshape(R, R, R), "weight": out["weight"].reshape(R, R, R),
            "color": None if out["color"] is None else out["color"].reshape(R, R, R, 3), "trunc": trunc, "bound_min": lo, "bound_max": hi,
            "space": "static" if deform_fn is None else "canonical"}


# ---- sampling and the mesh ---------------------------------------------------------------------------------------------------------------
def sample_volume(volume, points, bound_min, bound_max):
    """``volume`` [R,R,R] or [R,R,R,C] at world ``points`` [M,3] (read as fp32), trilinear in fp64: (values [M] or [M,C] fp64, inside [M]
    bool).  Per axis g = (p - bound_min) / (bound_max - bound_min) (R - 1) on the fp64 bounds; inside = every g in [0, R - 1] (false for
    a non-finite point); cell i = min(floor(g), R - 2), f = g - i; the two z ends are blended first, then y, then x, each a + f (b - a).
    Rows that are not inside have value 0."""
    vol = np.asarray(volume, np.float32)
    if vol.ndim not in (3, 4) or vol.shape[0] < 2 or vol.shape[:3] != (vol.shape[0],) * 3:
        raise ValueError(f"volume must be [R, R, R] or [R, R, R, C] with R >= 2 (got {vol.shape})")
    R = vol.shape[0]
    v4 = vol.reshape(R, R, R, -1).astype(np.float64)
    p = np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    lo, hi = np.asarray(bound_min, np.float64).reshape(3), np.asarray(bound_max, np.float64).reshape(3)
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi > lo).all()):
        raise ValueError("bounds must be finite with bound_max > bound_min")
    with np.errstate(all="ignore"):
        g = (p - lo) / (hi - lo) * float(R - 1)
        inside = ((g >= 0) & (g <= R - 1)).all(-1)
    g = np.where(inside[:, None], g, 0.0)
    i = np.clip(np.floor(g).astype(np.int64), 0, R - 2)
    f = g - i
    ix, iy, iz = i[:, 0], i[:, 1], i[:, 2]
    fx, fy, fz = f[:, 0:1], f[:, 1:2], f[:, 2:3]
    yb = []
    for dx in (0, 1):
        zb = []
        for dy in (0, 1):
            a, e = v4[ix + dx, iy + dy, iz], v4[ix + dx, iy + dy, iz + 1]
            zb.append(a + fz * (e - a))
        yb.append(zb[0] + fy * (zb[1] - zb[0]))
    val = np.where(inside[:, None], yb[0] + fx * (yb[1] - yb[0]), 0.0)
    return (val[:, 0] if vol.ndim == 3 else val), inside


ISO = {"tetrahedra": meshing.marching_tetrahedra, "cubes": meshing.marching_cubes}


def mesh_filter(edge_ends, triangles, weight_flat, min_weight):
    """(keep_vertex [V] bool, triangles kept and renumbered [T',3]): a vertex is kept when both grid ends of its edge have weight >=
    ``min_weight``, a triangle when all three of its vertices are; kept vertices keep their order."""
    keep = (weight_flat[edge_ends[:, 0]] >= min_weight) & (weight_flat[edge_ends[:, 1]] >= min_weight)
    tri = triangles[keep[triangles].all(-1)] if triangles.shape[0] else triangles
    new = np.cumsum(keep) - 1
    return keep, new[tri]


def fused_mesh(volume, min_weight=1.0, iso="tetrahedra"):
    """The zero level set of a fused ``volume`` (``fuse_depth``'s dict) as a mesh of the observed part only.  ``iso``: "tetrahedra"
    (``meshing.marching_tetrahedra``) or "cubes".  Never-observed voxels have tsdf +1, so the extractor also finds a false sheet
    between observed negative voxels and never-observed ones; it is dropped here, without any NaN convention in the extractor: a vertex
    is kept when BOTH grid ends of its edge have weight >= ``min_weight``, a triangle when all three vertices are kept, and the result
    is compacted.  dict(vertices [V,3] fp64 world (canonical for a canonical volume), triangles [T,3] int64, colors [V,3] or None,
    weight [V] -- colours and weight are the two ends' values interpolated as the vertex is --, edge_ends [V,2])."""
    if iso not in ISO:
        raise ValueError(f"iso must be one of {sorted(ISO)} (got {iso!r})")
    tsdf = np.asarray(volume["tsdf"], np.float32)
    R = tsdf.shape[0]
    wflat = np.asarray(volume["weight"], np.float32).reshape(-1)
    verts, tris, ends = ISO[iso](tsdf, 0.0, return_ends=True)
    keep, tris = mesh_filter(ends, tris, wflat, float(min_weight))
    verts, ends = verts[keep], ends[keep]
    u = tsdf.reshape(-1).astype(np.float64)
    ua, ub = u[ends[:, 0]], u[ends[:, 1]]
    w = ((0.0 - ua) / (ub - ua))[:, None]
    lerp = lambda a: a[ends[:, 0]] + w * (a[ends[:, 1]] - a[ends[:, 0]])
    lo, hi = np.asarray(volume["bound_min"], np.float64), np.asarray(volume["bound_max"], np.float64)
    color = volume.get("color")
    return {"vertices": verts / (R - 1.0) * (hi - lo)[None] + lo[None], "triangles": tris,
            "colors": None if color is None else lerp(np.asarray(color, np.float64).reshape(-1, 3)),
            "weight": lerp(wflat.astype(np.float64)[:, None])[:, 0], "edge_ends": ends}
