"""Geodesic distance on triangle meshes and along surface tracks: a first-order eikonal solver (the triangle update of Kimmel and
Sethian with an edge fallback, double-buffered Jacobi sweeps).  numpy only; this module is the specification and the fp64 host twin of
csrc/geodesic.hip (``Engine.geodesic``).  All arithmetic is fp64 on the inputs rounded to fp32;
x.y = (x0 y0 + x1 y1) + x2 y2."""
from __future__ import annotations

import numpy as np

from . import meshing

DET_REL = 2.0 ** -40          # a corner whose Gram determinant is not above DET_REL g11 g22 is a sliver: its edges only


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def corner_geometry(c, a, b):
    """What ``corner_update`` needs of the corner ``c`` of the triangle (c, a, b) and does not depend on the values: a dict of
    l1 = sqrt(g11), l2 = sqrt(g22), ok (det > 2^-40 g11 g22) and, where ok, q11, q12, q22, r1, r2, A (below)."""
    e1, e2 = a - c, b - c
    g11, g12, g22 = _dot(e1, e1), _dot(e1, e2), _dot(e2, e2)
    det = g11 * g22 - g12 * g12
    ok = det > (DET_REL * g11) * g22
    with np.errstate(divide="ignore", invalid="ignore"):
        q11, q12, q22 = g22 / det, -g12 / det, g11 / det
        r1, r2 = q11 + q12, q12 + q22
        A = r1 + r2
    return {"l1": np.sqrt(g11), "l2": np.sqrt(g22), "ok": ok, "q11": q11, "q12": q12, "q22": q22, "r1": r1, "r2": r2, "A": A}


def corner_values(geo, ua, ub):
    """``corner_update`` from ``corner_geometry``'s dict (broadcast against the values)."""
    with np.errstate(invalid="ignore", over="ignore"):
        edge = np.minimum(ua + geo["l1"], ub + geo["l2"])
        ok = geo["ok"] & np.isfinite(ua) & np.isfinite(ub)
        B = geo["r1"] * ua + geo["r2"] * ub
        s1 = geo["q11"] * ua + geo["q12"] * ub
        s2 = geo["q12"] * ua + geo["q22"] * ub
        C = (ua * s1 + ub * s2) - 1.0
        disc = B * B - geo["A"] * C
        ok = ok & (disc >= 0.0)
        t = (B + np.sqrt(np.where(ok, disc, 0.0))) / geo["A"]
        da, db = ua - t, ub - t
        w1 = geo["q11"] * da + geo["q12"] * db
        w2 = geo["q12"] * da + geo["q22"] * db
        ok = ok & (w1 <= 0.0) & (w2 <= 0.0)
        t = np.maximum(np.maximum(t, ua), ub)
    return np.where(ok, np.minimum(t, edge), edge)


def corner_update(c, a, b, ua, ub):
    """The candidate value at the corner ``c`` [...,3] of a valid triangle whose other corners ``a``, ``b`` hold ``ua``, ``ub`` (>= 0 or
    +inf).  Every line is one rounding per operation, in this order (csrc/geodesic.hip follows it line by line):

        e1 = a - c, e2 = b - c;  g11 = e1.e1, g12 = e1.e2, g22 = e2.e2;  det = g11 g22 - g12 g12
        edge = min(ua + sqrt(g11), ub + sqrt(g22))                        (an infinite u contributes +inf)
        the triangle candidate exists iff det > (2^-40 g11) g22, ua and ub are finite, and disc >= 0 below:
        q11 = g22 / det, q12 = -g12 / det, q22 = g11 / det                (Q = G^-1)
        r1 = q11 + q12, r2 = q12 + q22, A = r1 + r2                        (1'Q1)
        B = r1 ua + r2 ub                                                  (1'Qu)
        s1 = q11 ua + q12 ub, s2 = q12 ua + q22 ub, C = (ua s1 + ub s2) - 1 (u'Qu - 1)
        disc = B B - A C;  t = (B + sqrt(disc)) / A                        (the larger root of A t^2 - 2 B t + C = 0)
        da = ua - t, db = ub - t;  w1 = q11 da + q12 db, w2 = q12 da + q22 db
        t is accepted iff w1 <= 0 and w2 <= 0 (upwind: the gradient E w points into the triangle), as max(max(t, ua), ub)
        the candidate is min(t, edge) if t is accepted, else edge."""
    return corner_values(corner_geometry(c, a, b), ua, ub)


CORNERS = ((0, 1, 2), (1, 2, 0), (2, 0, 1))          # (c, a, b) of a triangle's three corner updates


class _Frame:
    """One frame's valid triangles with the geometry of their corners, and the sweep over any number of fields."""

    def __init__(self, v32, triangles):
        _, _, tri, ids = meshing._surface_inputs(np.zeros((0, 3), np.float32), v32, triangles)
        self.V, self.ids = len(v32), ids
        self.tri = tri[ids]
        self.v = np.asarray(v32, np.float32).astype(np.float64)
        p = [self.v[self.tri[:, k]] for k in range(3)]
        self.geo = [corner_geometry(p[c], p[a], p[b]) for c, a, b in CORNERS]
        target = np.concatenate([self.tri[:, c] for c, _, _ in CORNERS])
        self.order = np.argsort(target, kind="stable")
        ids_sorted = target[self.order]
        self.starts = np.nonzero(np.r_[True, ids_sorted[1:] != ids_sorted[:-1]])[0] if len(target) else np.zeros(0, np.int64)
        self.touched = ids_sorted[self.starts] if len(target) else np.zeros(0, np.int64)          # the vertices on a valid triangle

    def sweep(self, cur):
        """next [S,V] of cur [S,V]: next[c] = min(cur[c], every corner update of every valid triangle, computed from cur)."""
        nxt = cur.copy()
        if len(self.tri) == 0:
            return nxt
        cand = np.concatenate([corner_values(self.geo[k], cur[:, self.tri[:, a]], cur[:, self.tri[:, b]])
                               for k, (c, a, b) in enumerate(CORNERS)], axis=1)
        best = np.minimum.reduceat(cand[:, self.order], self.starts, axis=1)
        nxt[:, self.touched] = np.minimum(cur[:, self.touched], best)
        return nxt

    def solve(self, cur):
        """(the fixed point of ``sweep`` from cur, the number of sweeps: the first that changes nothing is the last)."""
        sweeps = 0
        while True:
            nxt = self.sweep(cur)
            sweeps += 1
            if np.array_equal(nxt, cur):
                return nxt, sweeps
            if sweeps > self.V + 1:
                raise RuntimeError(f"geodesic sweeps did not reach their fixed point in {sweeps} sweeps ({self.V} vertices)")
            cur = nxt


def project(points, v_ref32, triangles):
    """(triangle [N] int64, -1 for none; weights [N,3] fp64) of ``points`` [N,3] on the mesh of the reference frame: the triangle and
    closest point p' of ``meshing.point_to_mesh``, and p''s barycentric weights in that triangle (v0, v1, v2):
    e1 = v1 - v0, e2 = v2 - v0, d = p' - v0; d11 = e1.e1, d12 = e1.e2, d22 = e2.e2, b1 = d.e1, b2 = d.e2; den = d11 d22 - d12 d12;
    w1 = (d22 b1 - d12 b2) / den, w2 = (d11 b2 - d12 b1) / den, w0 = (1 - w1) - w2; a triangle with den <= 0 (no area) gives (1, 0, 0)."""
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    _, t, closest = meshing.point_to_mesh(pts, v_ref32, triangles)
    t = t.astype(np.int64)
    w = np.zeros((len(pts), 3))
    hit = t >= 0
    if hit.any():
        tri = np.asarray(triangles).reshape(-1, 3).astype(np.int64)[t[hit]]
        v = np.asarray(v_ref32, np.float32).astype(np.float64)
        v0, v1, v2 = v[tri[:, 0]], v[tri[:, 1]], v[tri[:, 2]]
        e1, e2, d = v1 - v0, v2 - v0, closest[hit].astype(np.float64) - v0
        d11, d12, d22, b1, b2 = _dot(e1, e1), _dot(e1, e2), _dot(e2, e2), _dot(d, e1), _dot(d, e2)
        den = d11 * d22 - d12 * d12
        flat = ~(den > 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            w1 = np.where(flat, 0.0, (d22 * b1 - d12 * b2) / den)
            w2 = np.where(flat, 0.0, (d11 * b2 - d12 * b1) / den)
        w[hit] = np.stack([(1.0 - w1) - w2, w1, w2], 1)
    return t, w


def carry(tri_ids, weights, v32, triangles):
    """The material points (triangle, weights) in the frame ``v32`` [V,3]: (w0 v0 + w1 v1) + w2 v2 per component, fp64 [N,3]; NaN rows
    where there is no triangle."""
    out = np.full((len(tri_ids), 3), np.nan)
    hit = tri_ids >= 0
    if hit.any():
        tri = np.asarray(triangles).reshape(-1, 3).astype(np.int64)[tri_ids[hit]]
        v = np.asarray(v32, np.float32).astype(np.float64)
        w = weights[hit]
        out[hit] = (w[:, 0:1] * v[tri[:, 0]] + w[:, 1:2] * v[tri[:, 1]]) + w[:, 2:3] * v[tri[:, 2]]
    return out


def _length(d):
    return np.sqrt(_dot(d, d))


def mesh_geodesic(vertices, triangles, sources, *, targets=None, reference=0):
    """Geodesic distance fields on a triangle mesh, and their read-out at points.  ``vertices`` [V,3] or [F,V,3] (F frames of one
    topology, e.g. ``track_mesh``'s), ``triangles`` [T,3] integers, ``sources`` an integer array [S] of vertex ids or a float array
    [S,3] of points, ``targets`` [Q,3] points or None.  Returns dict(distance [F,S,V] fp32 ([S,V] for a single mesh; +inf = not
    reachable), sweeps, and with targets target_distance [F,S,Q] fp32 ([S,Q])).

    * Validity.  A triangle takes part in a frame iff its indices are distinct, lie in [0, V), and its corners are finite there
      (the rule of ``meshing.point_to_mesh``).
    * Update.  ``corner_update`` (its docstring is the operation order).  A triangle's three updates are (c, a, b) = (v0, v1, v2),
      (v1, v2, v0), (v2, v0, v1).
    * Sweep.  next[c] = min(cur[c], every corner update of every valid triangle, computed from cur): Jacobi, so the result does not
      depend on any order.  The fields start at +inf except the seeds and the sweeps stop after the first that changes nothing;
      ``sweeps`` counts them (that last one included; the largest count over the frames).  V sweeps suffice: an accepted update is
      never below its inputs, so each sweep makes final at least the smallest value that is not yet final; V + 1 sweeps raise.
    * Seeds.  A seed (vertex, value) takes effect iff the vertex is a corner of a triangle valid in that frame and the value is
      finite.  A vertex-id source seeds that vertex with 0.  A source point is projected onto the ``reference`` frame (``project``:
      ``point_to_mesh``'s triangle and closest point p', p''s barycentric weights), the material point is carried to every frame
      (``carry``), and in each frame the triangle's three corners are seeded with their straight distances to the carried p'.
      A source on no triangle (a bad vertex id, a non-finite point, no valid triangle) leaves its whole field +inf; it is not an error.
    * Read-out.  Targets are projected and carried like source points.  target_distance[f, s, q] = the smallest of
      corner_update(q'; a, b, u[a], u[b]) over the corner pairs (v0, v1), (v1, v2), (v2, v0) of the target's triangle and, when
      source s is a point in the same triangle, the straight |p' - q'|; +inf for a target on no triangle (or an invalid one in f)."""
    v = np.asarray(vertices, np.float32)
    single = v.ndim == 2
    if single:
        v = v[None]
    if v.ndim != 3 or v.shape[2] != 3:
        raise ValueError(f"vertices must be [V, 3] or [F, V, 3] (got {v.shape})")
    F, V = v.shape[:2]
    if not -F <= int(reference) < F:
        raise ValueError(f"reference frame {reference} of {F}")
    ref = int(reference) % F
    tri = np.asarray(triangles)
    tri = np.zeros((0, 3), np.int64) if tri.size == 0 else tri
    src = np.asarray(sources)
    by_id = np.issubdtype(src.dtype, np.integer)
    if by_id:
        src = src.reshape(-1).astype(np.int64)
    else:
        if src.ndim != 2 or src.shape[1] != 3:
            raise ValueError(f"sources must be an integer [S] array of vertex ids or a float [S, 3] array of points (got {src.shape})")
        s_tri, s_w = project(src, v[ref], tri)
    S = len(src)
    if S < 1:
        raise ValueError("at least one source")
    if targets is not None:
        q_tri, q_w = project(np.asarray(targets, np.float32).reshape(-1, 3), v[ref], tri)
        target_distance = np.full((F, S, len(q_tri)), np.inf, np.float32)
    distance = np.full((F, S, V), np.inf, np.float32)
    tri64 = tri.astype(np.int64).reshape(-1, 3)
    sweeps = 0
    for f in range(F):
        frame = _Frame(v[f], tri)
        on_mesh = np.zeros(V, bool)
        on_mesh[frame.touched] = True
        cur = np.full((S, V), np.inf)
        if by_id:
            for s, i in enumerate(src):
                if 0 <= i < V and on_mesh[i]:
                    cur[s, i] = 0.0
        else:
            p = carry(s_tri, s_w, v[f], tri)
            for s in np.nonzero(s_tri >= 0)[0]:
                corners = tri64[s_tri[s]]
                val = _length(frame.v[corners] - p[s])
                for i, d in zip(corners, val):
                    if on_mesh[i] and np.isfinite(d):
                        cur[s, i] = min(cur[s, i], d)
        u, n = frame.solve(cur)
        sweeps = max(sweeps, n)
        distance[f] = u.astype(np.float32)
        if targets is not None and len(q_tri):
            valid = np.zeros(len(tri64), bool)
            valid[frame.ids] = True
            q = carry(q_tri, q_w, v[f], tri)
            rows = np.nonzero((q_tri >= 0) & np.isfinite(q).all(1) & valid[np.maximum(q_tri, 0)])[0]
            if len(rows):
                corners = tri64[q_tri[rows]]                                  # [R,3]
                pc = frame.v[corners]                                         # [R,3,3]
                best = np.full((S, len(rows)), np.inf)
                for a, b in ((0, 1), (1, 2), (2, 0)):
                    geo = corner_geometry(q[rows], pc[:, a], pc[:, b])
                    best = np.minimum(best, corner_values(geo, u[:, corners[:, a]], u[:, corners[:, b]]))
                if not by_id:
                    same = (s_tri[:, None] == q_tri[rows][None]) & (s_tri[:, None] >= 0)
                    with np.errstate(invalid="ignore"):
                        straight = _length(p[:, None, :] - q[rows][None])
                    best = np.where(same & np.isfinite(straight), np.minimum(best, straight), best)
                target_distance[f][:, rows] = best.astype(np.float32)
    out = {"distance": distance[0] if single else distance, "sweeps": sweeps}
    if targets is not None:
        out["target_distance"] = target_distance[0] if single else target_distance
    return out


def track_geodesic(track, points_a, points_b, reference=0, mesh_fn=mesh_geodesic):
    """[F, S] lengths along the tissue between the paired landmarks ``points_a[s]`` and ``points_b[s]`` ([S,3] each, given in frame
    ``reference``) over the frames of the dict ``track_mesh`` returns: S fields from ``points_a`` read out at ``points_b``, the
    diagonal of ``mesh_geodesic``'s target_distance.  ``mesh_fn``: that function, or one with its signature (the renderer passes its
    device path)."""
    if len(points_a) != len(points_b):
        raise ValueError(f"track_geodesic pairs its landmarks: {len(points_a)} and {len(points_b)} points")
    td = mesh_fn(track["vertices"], track["triangles"], points_a, targets=points_b, reference=reference)["target_distance"]
    if td.ndim == 2:
        td = td[None]
    i = list(range(td.shape[1]))
    return td[:, i, i]
