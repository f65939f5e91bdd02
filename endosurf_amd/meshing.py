"""Iso-surface extraction for ``extract_observation_geometry``.

The reference delegates to PyMCubes (``mcubes.marching_cubes``, src/renderer/utils.py:130, requirements.txt:8 — an
un-vendored third-party dependency; parity unpinned).  When ``mcubes`` is importable it is used, otherwise this module's
marching-tetrahedra extractor (vectorised numpy, host side: it runs once per frame on a field that was sampled on the GPU and
copied back in a single transfer) produces a watertight mesh of the same level set in the same index-space coordinates.
The triangulation differs from PyMCubes' (6 tetrahedra per cell instead of the cube table)."""
from __future__ import annotations

import numpy as np

# the 6 tetrahedra of a cube around its main diagonal (corner index = 4*dx + 2*dy + dz); they tile space consistently
_TETS = np.array([[0, 1, 3, 7], [0, 3, 2, 7], [0, 2, 6, 7], [0, 6, 4, 7], [0, 4, 5, 7], [0, 5, 1, 7]], np.int64)
_CORNER = np.array([[(c >> 2) & 1, (c >> 1) & 1, c & 1] for c in range(8)], np.int64)


def _tet_edges_for_case():
    """For each of the 16 inside/outside patterns of a tetrahedron: up to 2 triangles given as edges (a, b) between local
    vertices (a inside, b outside), or -1."""
    table = np.full((16, 2, 3, 2), -1, np.int64)
    for case in range(16):
        ins = [i for i in range(4) if (case >> i) & 1]
        out = [i for i in range(4) if not (case >> i) & 1]
        if len(ins) == 1:
            a = ins[0]
            table[case, 0] = [(a, out[0]), (a, out[1]), (a, out[2])]
        elif len(ins) == 3:
            b = out[0]
            table[case, 0] = [(ins[0], b), (ins[1], b), (ins[2], b)]
        elif len(ins) == 2:
            a0, a1 = ins
            b0, b1 = out
            table[case, 0] = [(a0, b0), (a0, b1), (a1, b1)]
            table[case, 1] = [(a0, b0), (a1, b1), (a1, b0)]
    return table


_TABLE = _tet_edges_for_case()


def marching_tetrahedra(u: np.ndarray, threshold: float = 0.0):
    """(vertices [V,3] float in index coordinates, triangles [T,3] int) of the level set u == threshold.
    'inside' = u < threshold; triangles are oriented with normals pointing to increasing u."""
    u = np.asarray(u, np.float64)
    nx, ny, nz = u.shape
    if min(nx, ny, nz) < 2:
        return np.zeros((0, 3), np.float64), np.zeros((0, 3), np.int64)
    inside = u < threshold
    # cells that the level set crosses
    blk = [inside[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz] for dx, dy, dz in _CORNER]
    cnt = np.sum(blk, axis=0)
    ci, cj, ck = np.nonzero((cnt > 0) & (cnt < 8))
    if ci.size == 0:
        return np.zeros((0, 3), np.float64), np.zeros((0, 3), np.int64)
    base = np.stack([ci, cj, ck], -1)                                     # [C,3]
    corner_idx = base[:, None, :] + _CORNER[None]                         # [C,8,3]
    lin = (corner_idx[..., 0] * ny + corner_idx[..., 1]) * nz + corner_idx[..., 2]     # [C,8] linear grid ids
    tet_lin = lin[:, _TETS]                                               # [C,6,4]
    tet_in = inside.reshape(-1)[tet_lin]
    case = (tet_in * np.array([1, 2, 4, 8])).sum(-1)                      # [C,6]
    tri = _TABLE[case]                                                    # [C,6,2,3,2] local vertex pairs
    ok = tri[..., 0, 0] >= 0                                              # [C,6,2]
    tl = np.broadcast_to(tet_lin[:, :, None, None, :], tri.shape[:4] + (4,))
    a = np.take_along_axis(tl, np.maximum(tri[..., 0:1], 0), -1)[..., 0][ok]     # [T,3] grid id of the inside end
    b = np.take_along_axis(tl, np.maximum(tri[..., 1:2], 0), -1)[..., 0][ok]     # [T,3] outside end
    # unique vertices per grid edge
    key = a.astype(np.int64) * (nx * ny * nz) + b
    uniq, inv = np.unique(key.reshape(-1), return_inverse=True)
    ea, eb = uniq // (nx * ny * nz), uniq % (nx * ny * nz)
    ua, ub = u.reshape(-1)[ea], u.reshape(-1)[eb]
    w = (threshold - ua) / (ub - ua)
    pa = np.stack(np.unravel_index(ea, u.shape), -1).astype(np.float64)
    pb = np.stack(np.unravel_index(eb, u.shape), -1).astype(np.float64)
    verts = pa + w[:, None] * (pb - pa)
    tris = inv.reshape(-1, 3).astype(np.int64)
    # orientation: normal along the field gradient (from the inside end towards the outside end of an edge)
    p0, p1, p2 = verts[tris[:, 0]], verts[tris[:, 1]], verts[tris[:, 2]]
    n = np.cross(p1 - p0, p2 - p0)
    ia = np.stack(np.unravel_index(a[:, 0], u.shape), -1).astype(np.float64)
    ib = np.stack(np.unravel_index(b[:, 0], u.shape), -1).astype(np.float64)
    flip = np.einsum("ij,ij->i", n, ib - ia) < 0
    tris[flip] = tris[flip][:, [0, 2, 1]]
    keep = (tris[:, 0] != tris[:, 1]) & (tris[:, 1] != tris[:, 2]) & (tris[:, 0] != tris[:, 2])
    return verts, tris[keep]


def iso_surface(u: np.ndarray, threshold: float = 0.0):
    """mcubes.marching_cubes(u, threshold) when PyMCubes is installed (the reference's extractor), else marching tetrahedra."""
    try:
        import mcubes  # type: ignore
        if hasattr(mcubes, "marching_cubes"):
            return mcubes.marching_cubes(np.asarray(u), threshold)
    except ImportError:
        pass
    return marching_tetrahedra(u, threshold)


# ---- narrow-band field (host twin of csrc/band.hip / Engine.band_field) ---------------------------------------------------------------
def band_margin(ends, shape, block, lipschitz):
    """``lipschitz`` times the world-space diagonal of a full block of ``block`` cells on a lattice of ``shape`` points whose axes run
    from ends[a][0] to ends[a][1] (fp64 arithmetic: Engine.band_field and band_field pass the same number to the seed rule)."""
    import math
    return float(lipschitz) * math.sqrt(sum((block * (float(hi) - float(lo)) / (n - 1)) ** 2 for (lo, hi), n in zip(ends, shape)))


def band_field(sample, axes, threshold=0.0, block=8, lipschitz=1.0, max_fraction=0.5, return_blocks=False):
    """A field on the lattice ``axes`` (three 1-D coordinate arrays) whose marching_tetrahedra mesh is the dense field's, built from
    evaluations of ``sample(x[M,3]) -> [M]`` near the level set only (numpy twin of ``Engine.band_field``, same block sets, same values).

    Blocks of ``block`` cells per axis.  A block is a SEED when the 'inside' flags (u < threshold, NaN outside) of its 8 corners differ,
    a corner is NaN, or no corner is farther than ``lipschitz`` * (world diagonal of a block) from the level; seeds are evaluated on all
    their points, and a block next to an evaluated one is activated as well when a value on the shared face has the other sign than its
    corners, until no face does.  Inactive blocks are filled with their corner value farthest from the level.  If the seeds are more
    than ``max_fraction`` of the blocks the lattice is evaluated densely instead (``fallback``).

    The mesh of the result contains, complete and with the dense mesh's coordinates, every vertex-connected component of the dense mesh
    that crosses a seed block; it is the dense mesh when |grad u| <= lipschitz holds in the blocks that were culled.  With a smaller
    ``lipschitz`` a closed component that fits between the block corners can be lost.

    Returns (field [nx,ny,nz] float32, stats[, block_round [nbx,nby,nbz] int32: 0 = never evaluated, 1 = seed, r = activated by the
    (r-1)-th growth round])."""
    axes = [np.asarray(a, np.float32).reshape(-1) for a in axes]
    shape = tuple(len(a) for a in axes)
    B = int(block)
    if len(axes) != 3 or min(shape) < 2:
        raise ValueError("band_field needs three axes of at least 2 points")
    if not 2 <= B <= 32:
        raise ValueError("block must be in 2..32")
    thr = float(threshold)
    nb = tuple(-(-(n - 1) // B) for n in shape)
    NB, N = nb[0] * nb[1] * nb[2], shape[0] * shape[1] * shape[2]

    def evaluate(ix, iy, iz):
        x = np.stack([axes[0][ix], axes[1][iy], axes[2][iz]], -1).reshape(-1, 3)
        return np.asarray(sample(x), np.float32).reshape(-1)

    cidx = [np.minimum(np.arange(b + 1) * B, n - 1) for b, n in zip(nb, shape)]
    ci, cj, ck = np.meshgrid(*cidx, indexing="ij")
    uc = evaluate(ci, cj, ck).reshape(ci.shape)
    corner = np.stack([uc[dx:dx + nb[0], dy:dy + nb[1], dz:dz + nb[2]] for dx, dy, dz in _CORNER])          # [8, nbx, nby, nbz]
    c64 = corner.astype(np.float64)
    cin = c64 < thr
    nan = np.isnan(c64)
    dev = np.where(nan, -1.0, np.abs(c64 - thr))
    far_c = np.argmax(dev, axis=0)                                          # the first corner with the largest |u - thr|
    far = np.take_along_axis(dev, far_c[None], 0)[0] > band_margin([(a[0], a[-1]) for a in axes], shape, B, lipschitz)
    fill = np.take_along_axis(corner, far_c[None], 0)[0]
    seed = (cin.any(0) != cin.all(0)) | nan.any(0) | ~far
    rnd = seed.astype(np.int32)
    stats = {"dense_points": N, "evaluated_points": int(uc.size), "blocks": NB, "seed_blocks": int(seed.sum()), "active_blocks": int(seed.sum()),
             "rounds": 0, "fallback": False}
    if stats["seed_blocks"] > float(max_fraction) * NB:
        gi, gj, gk = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
        field = evaluate(gi, gj, gk).reshape(shape)
        stats.update(evaluated_points=stats["evaluated_points"] + N, active_blocks=NB, fallback=True)
        return (field, stats, rnd) if return_blocks else (field, stats)
    bof = [np.minimum(np.arange(n) // B, b - 1) for n, b in zip(shape, nb)]
    field = np.ascontiguousarray(fill[np.ix_(*bof)], np.float32)

    def span(b, axis):          # the closed index range of block coordinate b
        return slice(b * B, min((b + 1) * B, shape[axis] - 1) + 1)

    r = 1
    while True:
        new = np.argwhere(rnd == r)
        if len(new) == 0:
            break
        idx = [np.meshgrid(*[np.arange(span(b[a], a).start, span(b[a], a).stop) for a in range(3)], indexing="ij") for b in new]
        vals = evaluate(*[np.concatenate([g[a].reshape(-1) for g in idx]) for a in range(3)])
        stats["evaluated_points"] += int(vals.size)
        o = 0
        for b, g in zip(new, idx):
            field[span(b[0], 0), span(b[1], 1), span(b[2], 2)] = vals[o:o + g[0].size].reshape(g[0].shape)
            o += g[0].size
        for b in new:
            for axis in range(3):
                for side in (-1, 1):
                    q = b.copy()
                    q[axis] += side
                    if not 0 <= q[axis] < nb[axis] or rnd[tuple(q)] != 0:
                        continue
                    sl = [span(b[a], a) for a in range(3)]
                    plane = max(b[axis], q[axis]) * B
                    sl[axis] = slice(plane, plane + 1)
                    if ((field[tuple(sl)].astype(np.float64) < thr) != (float(fill[tuple(q)]) < thr)).any():
                        rnd[tuple(q)] = r + 1
        r += 1
    stats.update(active_blocks=int((rnd > 0).sum()), rounds=int(rnd.max()) - 1 if rnd.max() > 0 else 0)
    return (field, stats, rnd) if return_blocks else (field, stats)


# ---- connected components, the largest-component filter, nearest neighbour (host twins of csrc/mesh.hip; contract: DESIGN.md 7b) -------
def _as_triangles(triangles, n_vertices):
    tri = np.asarray(triangles)
    if tri.size == 0:
        tri = np.zeros((0, 3), np.int64)
    if tri.ndim != 2 or tri.shape[1] != 3 or not np.issubdtype(tri.dtype, np.integer):
        raise ValueError(f"triangles must be an integer [T, 3] array (got {tri.dtype} {tri.shape})")
    V = int(n_vertices)
    if V < 0 or V >= 1 << 31 or len(tri) >= 1 << 31:
        raise ValueError("vertex / triangle counts must be in [0, 2^31)")
    tri = tri.astype(np.int64)
    if len(tri) and (tri.min() < 0 or tri.max() >= V):
        raise ValueError(f"triangle indices outside [0, {V})")
    return tri, V


def mesh_components(triangles, n_vertices):
    """Connected components of an indexed triangle mesh (numpy twin of ``Engine.mesh_components``).

    A triangle with a repeated index is degenerate: it joins nothing and counts for nothing.  Two other triangles are connected when
    they share a vertex index (Open3D's ``cluster_connected_triangles`` asks for a shared edge: the two differ only where two sheets
    touch in a single vertex, which this rule merges).  The label of a component is its smallest vertex index.
    Returns (vertex_label [V] int32: a vertex of no non-degenerate triangle is its own label, triangle_label [T] int32: -1 for a
    degenerate triangle, component_triangles [V] int32: the triangle count at the label's index, 0 elsewhere)."""
    return _components(*_as_triangles(triangles, n_vertices))[:3]


def _components(tri, V):
    """mesh_components of checked arguments, and the number of hooking rounds it took (the last one, which finds nothing, included)."""
    good = (tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])
    t = tri[good]
    parent = np.arange(V, dtype=np.int64)
    rounds = 0
    while len(t):          # min-label hooking of the roots, then pointer jumping until flat: O(log V) rounds
        rounds += 1
        r = parent[t]
        m = r.min(axis=1)
        if (r == m[:, None]).all():
            break
        np.minimum.at(parent, r.reshape(-1), np.repeat(m, 3))
        while True:
            nxt = parent[parent]
            if np.array_equal(nxt, parent):
                break
            parent = nxt
    tlabel = np.full(len(tri), -1, np.int64)
    tlabel[good] = parent[t[:, 0]]
    counts = np.bincount(tlabel[good], minlength=V)[:V] if V else np.zeros(0, np.int64)
    return parent.astype(np.int32), tlabel.astype(np.int32), counts.astype(np.int32), rounds


def keep_components(vertices, triangles, keep_ratio=0.9, compact=True):
    """The triangles of the largest components (numpy twin of ``Engine.keep_components``): triangle i stays iff it is not degenerate
    and NOT ``component_triangles[label_i] < keep_ratio * max(component_triangles)`` (fp64, the comparison of the reference's
    trainer_endosurf.py:444 with keep_ratio = 0.9).  Kept triangles and vertices keep their input order; duplicate triangles are not
    removed.  ``compact=True`` drops the vertices no kept triangle uses and renumbers; ``compact=False`` keeps every vertex (what the
    reference does, which never calls ``remove_unreferenced_vertices``).
    Returns (vertices [V', 3], triangles [T', 3] int32, vertex_map [V'] int64: the old index of each new vertex, stats)."""
    verts = np.asarray(vertices)
    if verts.ndim != 2 or verts.shape[1] != 3:
        raise ValueError(f"vertices must be [V, 3] (got {verts.shape})")
    ratio = float(keep_ratio)
    if not 0.0 <= ratio <= 1.0:
        raise ValueError("keep_ratio must be in [0, 1]")
    tri, V = _as_triangles(triangles, len(verts))
    _, tlabel, counts, rounds = _components(tri, V)
    biggest = int(counts.max()) if V else 0
    good = tlabel >= 0
    keep = good.copy()
    keep[good] = ~(counts[tlabel[good]] < ratio * biggest)
    used = np.ones(V, bool)
    if compact:
        used = np.zeros(V, bool)
        used[tri[keep].reshape(-1)] = True
    vmap = np.nonzero(used)[0].astype(np.int64)
    new_id = np.cumsum(used) - 1
    stats = {"components": int((counts > 0).sum()), "max_triangles": biggest, "kept_triangles": int(keep.sum()),
             "degenerate": int((~good).sum()), "rounds": rounds}
    return verts[vmap], new_id[tri[keep]].astype(np.int32).reshape(-1, 3), vmap, stats


def nearest(query, points, chunk=1 << 22):
    """Exact nearest neighbour (numpy twin of ``Engine.nearest``, chunked brute force): for each query row the row of ``points`` with
    the smallest fp32 squared distance (dx dx + dy dy) + dz dz, the smallest index among equal ones; dist = its square root.  Non-finite
    rows of ``points`` (and points whose squared distance overflows) are never an answer; a query without an answer gets inf and -1.
    Returns (dist [Q] float32, index [Q] int32)."""
    q = np.ascontiguousarray(np.asarray(query, np.float32).reshape(-1, 3))
    p = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 3))
    Q, P = len(q), len(p)
    if P >= 1 << 31 or Q >= 1 << 31:
        raise ValueError("point / query counts must be below 2^31")
    best = np.full(Q, np.inf, np.float32)
    arg = np.full(Q, -1, np.int64)
    ids = np.nonzero(np.isfinite(p).all(axis=1))[0]
    pf = p[ids]
    rows = max(1, int(chunk) // max(len(pf), 1))
    with np.errstate(over="ignore", invalid="ignore"):
        for q0 in range(0, Q if len(pf) else 0, rows):
            d = q[q0:q0 + rows, None, :] - pf[None, :, :]
            d *= d
            d2 = (d[..., 0] + d[..., 1]) + d[..., 2]
            d2[~np.isfinite(d2)] = np.inf          # (a non-finite query row, an overflow)
            k = np.argmin(d2, axis=1)               # the first minimum: pf is in index order
            v = d2[np.arange(len(k)), k]
            hit = np.isfinite(v)
            best[q0:q0 + rows] = np.where(hit, v, np.inf)
            arg[q0:q0 + rows] = np.where(hit, ids[k], -1)
    return np.sqrt(best), arg.astype(np.int32)
