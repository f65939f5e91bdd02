"""Iso-surface extraction for ``extract_observation_geometry``.

The reference delegates to PyMCubes (``mcubes.marching_cubes``, src/renderer/utils.py:130, requirements.txt:8 — an
un-vendored third-party dependency; parity unpinned).  When ``mcubes`` is importable it is used, otherwise this module's
marching-tetrahedra extractor (vectorised numpy, host side: it runs once per frame on a field that was sampled on the GPU and
copied back in a single transfer) produces a watertight mesh of the same level set in the same index-space coordinates.
The triangulation differs from PyMCubes' (6 tetrahedra per cell instead of the cube table).  ``marching_cubes`` is a second extractor with
a cube table of this project's own (not PyMCubes'): the numpy twin of the device path's ``method="cubes"``, never chosen by default."""
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


def marching_tetrahedra(u: np.ndarray, threshold: float = 0.0, return_ends: bool = False):
    """(vertices [V,3] float in index coordinates, triangles [T,3] int[, edge_ends [V,2] int64 = the linear grid ids of each vertex's
    inside and outside end]) of the level set u == threshold.
    'inside' = u < threshold; triangles are oriented with normals pointing to increasing u."""
    u = np.asarray(u, np.float64)
    nx, ny, nz = u.shape
    empty = (np.zeros((0, 3), np.float64), np.zeros((0, 3), np.int64)) + ((np.zeros((0, 2), np.int64),) if return_ends else ())
    if min(nx, ny, nz) < 2:
        return empty
    inside = u < threshold
    # cells that the level set crosses
    blk = [inside[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz] for dx, dy, dz in _CORNER]
    cnt = np.sum(blk, axis=0)
    ci, cj, ck = np.nonzero((cnt > 0) & (cnt < 8))
    if ci.size == 0:
        return empty
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
    return (verts, tris[keep], np.stack([ea, eb], -1).astype(np.int64)) if return_ends else (verts, tris[keep])


# ---- cube triangulation (numpy twin of csrc/cubes.hip; the rule is this project's own: DESIGN.md 7a "Cube triangulation") ---------------
# the 12 cube edges as (owner corner, direction code 4 dx + 2 dy + dz of the axis): edge id = position in this list
CUBE_EDGES = tuple((oc, d) for oc in range(8) for d in (1, 2, 4) if not oc & d)
# the 6 cube faces: their 4 corners in cyclic order
CUBE_FACES = tuple(tuple(side * a + o for o in (0, b, b + c, c)) for a, b, c in ((4, 2, 1), (2, 4, 1), (1, 4, 2)) for side in (0, 1))
_EDGE_ID = {frozenset((oc, oc | d)): i for i, (oc, d) in enumerate(CUBE_EDGES)}
_cubes_cache = {}


def cube_edges_share_face(e1, e2):
    """Do the cube edges with ids ``e1`` and ``e2`` lie on one cube face?"""
    ends = {CUBE_EDGES[e1][0], sum(CUBE_EDGES[e1]), CUBE_EDGES[e2][0], sum(CUBE_EDGES[e2])}
    return any(ends <= set(face) for face in CUBE_FACES)


def cube_case_loops(case):
    """The closed loops of crossing edges (edge ids) of one of the 256 cell cases (bit c = corner c inside), each starting at its
    smallest edge id and oriented so that its normal points from the inside corners to the outside ones.

    On every face the crossing edges are joined by segments: two crossing edges by one segment; four (diagonal corners inside) by
    cutting off each inside corner, i.e. joining the two edges that meet at it.  The rule reads the face's four flags only, so the two
    cells that share a face draw the same segments."""
    ins = [(case >> c) & 1 for c in range(8)]
    nbr = {}
    for face in CUBE_FACES:
        fe = [_EDGE_ID[frozenset((face[i], face[(i + 1) % 4]))] for i in range(4)]          # edge i joins corners i and i + 1
        cr = [i for i in range(4) if ins[face[i]] != ins[face[(i + 1) % 4]]]
        segs = [(fe[cr[0]], fe[cr[1]])] if len(cr) == 2 else [(fe[(i - 1) % 4], fe[i]) for i in range(4) if ins[face[i]]] if len(cr) == 4 else []
        for a, b in segs:
            nbr.setdefault(a, []).append(b)
            nbr.setdefault(b, []).append(a)
    assert all(len(v) == 2 and v[0] != v[1] for v in nbr.values()), case
    corner = _CORNER.astype(np.float64)
    loops, todo = [], set(nbr)
    while todo:
        start = min(todo)
        loop, prev, cur = [start], start, nbr[start][0]
        while cur != start:
            loop.append(cur)
            prev, cur = cur, nbr[cur][0] if nbr[cur][0] != prev else nbr[cur][1]
        todo -= set(loop)
        assert 3 <= len(loop) <= 7, (case, loop)
        mid = np.array([0.5 * (corner[CUBE_EDGES[e][0]] + corner[sum(CUBE_EDGES[e])]) for e in loop])
        newell = np.cross(mid, np.roll(mid, -1, axis=0)).sum(axis=0)
        out_minus_in = sum((corner[sum(CUBE_EDGES[e])] - corner[CUBE_EDGES[e][0]]) * (1.0 if ins[CUBE_EDGES[e][0]] else -1.0) for e in loop)
        s = float(newell @ out_minus_in)
        assert s != 0.0, (case, loop)
        loops.append(loop if s > 0 else [loop[0]] + loop[:0:-1])
    return loops


def cube_fan(loop):
    """The fan that triangulates ``loop``: its apex is the first loop position whose fan has no diagonal joining two edges of one
    cube face (such a diagonal coincides with a segment the neighbouring cell may draw: a mesh edge used four times)."""
    n = len(loop)
    for k in range(n):
        r = loop[k:] + loop[:k]
        if not any(cube_edges_share_face(r[0], r[i]) for i in range(2, n - 1)):
            return [(r[0], r[i], r[i + 1]) for i in range(1, n - 1)]
    raise AssertionError(f"no fan without a face diagonal for loop {loop}")


def cubes_table():
    """table [256, 5, 3] int64: corner j of triangle k of a cell case as a cube edge id (index into CUBE_EDGES), -1 where there is
    none.  Loops in ascending order of their first edge, triangles in fan order, normals from inside to outside."""
    if "table" not in _cubes_cache:
        table = np.full((256, 5, 3), -1, np.int64)
        for case in range(256):
            tris = [t for loop in cube_case_loops(case) for t in cube_fan(loop)]
            assert len(tris) <= 5, case
            table[case, :len(tris)] = np.array(tris, np.int64).reshape(-1, 3)
        _cubes_cache["table"] = table
    return _cubes_cache["table"]


def marching_cubes(u: np.ndarray, threshold: float = 0.0, return_ends: bool = False):
    """(vertices [V,3] float64 in index coordinates, triangles [T,3] int64[, edge_ends [V,2] int64]) of the level set u == threshold
    by this project's cube triangulation (``cubes_table``): numpy twin of ``Engine.iso_surface(method="cubes")`` and its specification.

    Conventions are ``marching_tetrahedra``'s: 'inside' = u < threshold (NaN and u == threshold are outside), a vertex sits on an axis
    edge of the grid and is named by (inside end, outside end) as linear grid ids, its position is the same fp64 expression (a cube
    vertex equals the tetrahedra vertex on that edge bit for bit), normals point to increasing u -- by the table, not by a cross
    product.  Vertices are ordered by (linear id of the smaller end, direction code 4 dx + 2 dy + dz: z, then y, then x), triangles
    by (cell linear id, position in the table row).  Degenerate positions (a vertex on a grid point) are kept."""
    u = np.asarray(u, np.float64)
    empty = (np.zeros((0, 3), np.float64), np.zeros((0, 3), np.int64)) + ((np.zeros((0, 2), np.int64),) if return_ends else ())
    if u.ndim != 3 or min(u.shape) < 2:
        return empty
    nx, ny, nz = u.shape
    inside = u < threshold
    stride = np.array([1, nz, ny * nz], np.int64)                          # of the axes in slot order: z, y, x
    cross = np.zeros((nx, ny, nz, 3), bool)                                # slot (p, k): the edge from p along axis k crosses the level
    cross[:, :, :-1, 0] = inside[:, :, :-1] != inside[:, :, 1:]
    cross[:, :-1, :, 1] = inside[:, :-1, :] != inside[:, 1:, :]
    cross[:-1, :, :, 2] = inside[:-1, :, :] != inside[1:, :, :]
    flat = cross.reshape(-1)
    slots = np.nonzero(flat)[0]
    if slots.size == 0:
        return empty
    vid = np.cumsum(flat) - 1                                              # vertex id of a slot
    p, k = slots // 3, slots % 3
    q = p + stride[k]
    pin = inside.reshape(-1)[p]
    ea, eb = np.where(pin, p, q), np.where(pin, q, p)
    ua, ub = u.reshape(-1)[ea], u.reshape(-1)[eb]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        w = (threshold - ua) / (ub - ua)
        pa = np.stack(np.unravel_index(ea, u.shape), -1).astype(np.float64)
        pb = np.stack(np.unravel_index(eb, u.shape), -1).astype(np.float64)
        verts = pa + w[:, None] * (pb - pa)
    # triangles: the table row of every cell, its edge ids turned into slots of the cell's corner points
    case = np.zeros((nx - 1, ny - 1, nz - 1), np.int64)
    for c, (dx, dy, dz) in enumerate(_CORNER):
        case |= inside[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].astype(np.int64) << c
    ci, cj, ck = np.nonzero((case > 0) & (case < 255))
    rows = cubes_table()[case[ci, cj, ck]]                                 # [C,5,3] edge ids
    owner = np.array([(oc >> 2) * stride[2] + ((oc >> 1) & 1) * stride[1] + (oc & 1) for oc, _ in CUBE_EDGES], np.int64)
    rank = np.array([{1: 0, 2: 1, 4: 2}[d] for _, d in CUBE_EDGES], np.int64)
    cell = ((ci * ny + cj) * nz + ck)[:, None, None]
    e = np.maximum(rows, 0)
    tris = vid[(cell + owner[e]) * 3 + rank[e]][rows[..., 0] >= 0].astype(np.int64).reshape(-1, 3)
    return (verts, tris, np.stack([ea, eb], -1).astype(np.int64)) if return_ends else (verts, tris)


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


# ---- point-cloud clean-up queries (host twins of csrc/cloud.hip; contract: DESIGN.md 7g) -----------------------------------------------
def _cloud_rows(a):
    a = np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1, 3))
    if len(a) >= 1 << 31:
        raise ValueError("point / query counts must be below 2^31")
    return a


def _d2_rows(q, pf):
    """fp32 (dx dx + dy dy) + dz dz of every row of ``q`` against every row of ``pf``: [len(q), len(pf)]."""
    d = q[:, None, :] - pf[None, :, :]
    d *= d
    return (d[..., 0] + d[..., 1]) + d[..., 2]


def self_nearest(points, chunk=1 << 22):
    """For each row of ``points`` its nearest OTHER row (numpy twin of ``Engine.self_nearest``, chunked brute force; what Open3D's
    compute_nearest_neighbor_distance measures): for a finite row i the lexicographic minimum of (d2, j) over the finite rows j != i, d2
    the fp32 squared distance of ``nearest``; dist = its square root.  A duplicate of the point gives 0.  A non-finite row, a row
    without another finite row and a row whose every d2 overflows get inf and -1.  Returns (dist [P] float32, index [P] int32)."""
    p = _cloud_rows(points)
    best = np.full(len(p), np.inf, np.float32)
    arg = np.full(len(p), -1, np.int64)
    ids = np.nonzero(np.isfinite(p).all(axis=1))[0]
    pf = p[ids]
    rows = max(1, int(chunk) // max(len(pf), 1))
    with np.errstate(over="ignore", invalid="ignore"):
        for q0 in range(0, len(pf) if len(pf) > 1 else 0, rows):
            d2 = _d2_rows(pf[q0:q0 + rows], pf)
            m = np.arange(len(d2))
            d2[m, q0 + m] = np.inf                   # the row itself
            d2[~np.isfinite(d2)] = np.inf          # (an overflow)
            k = np.argmin(d2, axis=1)               # the first minimum: pf is in index order
            v = d2[m, k]
            hit = np.isfinite(v)
            best[ids[q0:q0 + rows]] = np.where(hit, v, np.inf)
            arg[ids[q0:q0 + rows]] = np.where(hit, ids[k], -1)
    return np.sqrt(best), arg.astype(np.int32)


def radius_count(query, points, radius=None, cap=0, radius_sq=None, chunk=1 << 22):
    """How many rows of ``points`` lie within a radius of each ``query`` row (numpy twin of ``Engine.radius_count``, chunked brute
    force): count[q] = the number of finite rows p with fp32 d2(q, p) <= r2, d2 the squared distance of ``nearest`` and
    r2 = float32(radius) x float32(radius) in fp32 (only the square of ``radius`` matters), or ``radius_sq`` itself.  A query that is a
    row of ``points`` counts itself.  A non-finite query row gives 0; r2 NaN or negative gives 0 everywhere; r2 = inf gives the number of
    finite rows.  ``cap`` > 0 gives min(count, cap).  Returns count [Q] int32."""
    q, p = _cloud_rows(query), _cloud_rows(points)
    if (radius is None) == (radius_sq is None):
        raise ValueError("radius_count takes either radius or radius_sq")
    if int(cap) < 0:
        raise ValueError(f"cap must be >= 0 (got {cap!r})")
    with np.errstate(over="ignore", invalid="ignore"):
        r2 = np.float32(radius_sq) if radius is None else np.float32(radius) * np.float32(radius)
        count = np.zeros(len(q), np.int64)
        if not r2 >= 0:
            return count.astype(np.int32)
        pf = p[np.isfinite(p).all(axis=1)]
        qids = np.nonzero(np.isfinite(q).all(axis=1))[0]
        rows = max(1, int(chunk) // max(len(pf), 1))
        for q0 in range(0, len(qids) if len(pf) else 0, rows):
            sel = qids[q0:q0 + rows]
            count[sel] = (_d2_rows(q[sel], pf) <= r2).sum(axis=1)          # (an overflowed d2 is inf: within r2 = inf only)
    return (np.minimum(count, int(cap)) if int(cap) > 0 else count).astype(np.int32)


def radius_outlier_mask(points, nb_points, radius):
    """bool [P]: the rows of ``points`` that a radius-outlier filter keeps (numpy twin of ``Engine.radius_outlier_mask``): a row is
    kept iff more than ``nb_points`` rows lie within ``radius`` of it, itself included, i.e.
    ``radius_count(points, points, radius, cap=nb_points + 1) > nb_points``; a non-finite row is never kept.  This is Open3D's
    ``remove_radius_outlier(nb_points, radius)`` as remembered (its search returns the point itself, and it keeps a point with more
    than ``nb_points`` results); the rule is NOT pinned against Open3D, which this project does not have at hand."""
    nb = int(nb_points)
    if nb < 0:
        raise ValueError(f"nb_points must be >= 0 (got {nb_points!r})")
    return radius_count(points, points, radius, cap=nb + 1) > nb


# ---- point-to-surface distance (host twin of csrc/surface.hip; contract: DESIGN.md 7f) ------------------------------------------------
def _dot3(a, b):          # vectors are tuples of three component arrays: no [..., 3] temporaries
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross3(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _sub3(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _where3(c, a, b):
    return tuple(np.where(c, x, y) for x, y in zip(a, b))


def _surface_inputs(points, vertices, triangles):
    """(queries [Q,3] fp32, vertices [V,3] fp32, triangles [T,3] int64, the indices of the triangles that take part)."""
    q = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 3))
    v = np.ascontiguousarray(np.asarray(vertices, np.float32).reshape(-1, 3))
    tri = np.asarray(triangles)
    if tri.size == 0:
        tri = np.zeros((0, 3), np.int64)
    if tri.ndim != 2 or tri.shape[1] != 3 or not np.issubdtype(tri.dtype, np.integer):
        raise ValueError(f"triangles must be an integer [T, 3] array (got {tri.dtype} {tri.shape})")
    if len(q) >= 1 << 31 or len(v) >= 1 << 31 or len(tri) >= 1 << 31:
        raise ValueError("query / vertex / triangle counts must be below 2^31")
    tri = tri.astype(np.int64)
    ok = ((tri >= 0) & (tri < len(v))).all(axis=1) & (tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])
    ids = np.nonzero(ok)[0]
    ids = ids[np.isfinite(v[tri[ids]]).all(axis=(1, 2))] if len(ids) else ids
    return q, v, tri, ids


def _point_triangles(q, v, tri):
    """(d2 [R,K] fp64, closest [R,K,3] fp64) of finite queries ``q`` [R,3] fp32 against the K triangles ``tri`` (all of them take part):
    the per-triangle rule of ``point_to_mesh``."""
    q = tuple(q[:, k].astype(np.float64)[:, None] for k in range(3))
    i0, i1, i2 = (tri[:, k][None] for k in range(3))
    v0, v1, v2 = (tuple(v[tri[:, j], k].astype(np.float64)[None] for k in range(3)) for j in range(3))
    n = _cross3(_sub3(v1, v0), _sub3(v2, v0))
    n2 = _dot3(n, n)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = _dot3(_sub3(q, v0), n) / n2
        p = tuple(q[k] - s * n[k] for k in range(3))
        inside = (n2 > 0) & (_dot3(_cross3(_sub3(v1, v0), _sub3(p, v0)), n) > 0) & (_dot3(_cross3(_sub3(v2, v1), _sub3(p, v1)), n) > 0) \
            & (_dot3(_cross3(_sub3(v0, v2), _sub3(p, v2)), n) > 0)
        d = _sub3(q, p)
        best = np.where(inside, _dot3(d, d), np.inf)
    at = _where3(inside, p, (np.nan, np.nan, np.nan))
    for ia, ib, pa, pb in ((i0, i1, v0, v1), (i1, i2, v1, v2), (i2, i0, v2, v0)):
        swap = ia > ib
        a, b = _where3(swap, pb, pa), _where3(swap, pa, pb)          # from the smaller vertex index to the larger
        e = _sub3(b, a)
        l2 = _dot3(e, e)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(l2 > 0, _dot3(_sub3(q, a), e) / l2, 0.0)
        c = tuple(np.where(t <= 0, a[k], np.where(t >= 1, b[k], a[k] + t * e[k])) for k in range(3))
        d = _sub3(q, c)
        d2 = _dot3(d, d)
        upd = d2 < best                                                  # strict: on a tie the face, then the earlier edge
        best = np.where(upd, d2, best)
        at = _where3(upd, c, at)
    return best, np.stack(at, -1)


def point_to_mesh(points, vertices, triangles, chunk=1 << 17, return_d2=False):
    """Exact distance from each row of ``points`` [Q,3] to the triangle mesh (``vertices`` [V,3], ``triangles`` [T,3] integers): numpy
    twin of ``Engine.point_to_mesh`` and its specification (chunked brute force).  Returns (dist [Q] float32, triangle [Q] int32,
    closest [Q,3] float32).  All arithmetic is fp64 on the inputs rounded to fp32; x.y = (x0 y0 + x1 y1) + x2 y2.

    * A triangle takes part iff its three indices are distinct, all lie in [0, V), and its three corners are finite.  Any other is
      skipped: never dereferenced, never an answer.
    * Edge.  The closest point of a segment is computed with the segment oriented from its smaller vertex index a to its larger b:
      l2 = |b - a|^2, t = ((q - a).(b - a)) / l2 if l2 > 0 else 0; t <= 0 gives a itself, t >= 1 gives b itself, otherwise
      c = a + t (b - a); d2 = |q - c|^2.  Two triangles that share an edge or a vertex therefore compute bit-identical values for it:
      a tie between them is an exact tie.
    * Face.  n = (v1 - v0) x (v2 - v0), n2 = n.n.  Only if n2 > 0: s = ((q - v0).n) / n2, p = q - s n; p counts iff the three side
      values ((vb - va) x (p - va)).n, for (va, vb) = (v0, v1), (v1, v2), (v2, v0), are all strictly positive (the border belongs to
      the edges); d2 = |q - p|^2.  A zero-area triangle with distinct indices is therefore its three segments.
    * Per triangle: the smallest d2 among the face, if it counts, and the three edges; on a tie the face wins, then the edges in the
      order v0v1, v1v2, v2v0.
    * Per query: the lexicographic minimum of (d2, triangle index) over the triangles that take part: the result does not depend on
      any order of evaluation.
    * dist = float32(sqrt(d2)), closest = that triangle's closest point rounded to float32.  A non-finite query row, T == 0 or no
      triangle that takes part gives inf / -1 / nan; Q == 0 gives empty arrays.

    ``chunk``: query-triangle pairs evaluated at a time (a few hundred bytes of temporaries each).  ``return_d2=True`` appends the dense
    matrix the minimum is taken over, d2 [Q,T] fp64 (inf for a triangle that takes no part and for a non-finite query row): for small
    inputs (tests, probes)."""
    q, v, tri, ids = _surface_inputs(points, vertices, triangles)
    Q = len(q)
    dist = np.full(Q, np.inf, np.float32)
    arg = np.full(Q, -1, np.int32)
    closest = np.full((Q, 3), np.nan, np.float32)
    dense = np.full((Q, len(tri)), np.inf) if return_d2 else None
    rows = np.nonzero(np.isfinite(q).all(axis=1))[0]
    if len(ids) == 0 or len(rows) == 0:
        return (dist, arg, closest, dense) if return_d2 else (dist, arg, closest)
    tk = tri[ids]
    step = max(1, int(chunk) // len(ids))
    for r0 in range(0, len(rows), step):
        r = rows[r0:r0 + step]
        d2, at = _point_triangles(q[r], v, tk)
        k = np.argmin(d2, axis=1)                    # the first minimum: ``ids`` ascends
        j = np.arange(len(r))
        dist[r] = np.sqrt(d2[j, k]).astype(np.float32)
        arg[r] = ids[k]
        closest[r] = at[j, k].astype(np.float32)
        if return_d2:
            dense[np.ix_(r, ids)] = d2
    return (dist, arg, closest, dense) if return_d2 else (dist, arg, closest)


# ---- mesh rasteriser (host twins of csrc/raster.hip; contract: DESIGN.md 7c) ---------------------------------------------------------
RAST_SUBPIXEL = 256                  # fixed-point units per pixel
RAST_GUARD = 1 << 22                 # |fixed-point coordinate| <= this: every edge function fits in int64 with room to spare
RAST_MAX_SIZE = 8192                 # largest image side
RAST_MAX_ATTRS = 8
RAST_CULL = {"none": 0, "back": 1, "front": 2}
RAST_REASONS = ("invalid", "near_rejected", "zero_area", "culled", "offscreen")          # count[t] = -1 .. -4, and 0 tiles


def camera_params(intrinsics, pose):
    """The 17 fp64 numbers both rasterisers read: R [9] (row-major rotation of the camera-to-world ``pose``), t [3], K00, K01, K02,
    K11, K12 of the upper-triangular ``intrinsics`` ([3,3] or [4,4]).  Raises for non-finite entries, K00 or K11 not positive, a last
    intrinsics row other than (0, 0, 1), or a pose whose rotation is not orthonormal with determinant +1 (to 1e-3)."""
    K = np.asarray(intrinsics.detach().cpu() if hasattr(intrinsics, "detach") else intrinsics, np.float64)
    P = np.asarray(pose.detach().cpu() if hasattr(pose, "detach") else pose, np.float64)
    if K.shape not in ((3, 3), (4, 4)) or P.shape != (4, 4):
        raise ValueError(f"intrinsics must be [3,3] or [4,4] and pose [4,4] (got {K.shape}, {P.shape})")
    cam = np.concatenate([P[:3, :3].reshape(-1), P[:3, 3], [K[0, 0], K[0, 1], K[0, 2], K[1, 1], K[1, 2]]])
    if not np.isfinite(cam).all():
        raise ValueError("camera parameters must be finite")
    if not (K[0, 0] > 0 and K[1, 1] > 0) or K[1, 0] != 0 or tuple(K[2, :3]) != (0.0, 0.0, 1.0):
        raise ValueError("intrinsics must be upper triangular with positive focal lengths and a last row (0, 0, 1)")
    R = P[:3, :3]
    if np.abs(R.T @ R - np.eye(3)).max() > 1e-3 or np.linalg.det(R) < 0:
        raise ValueError("pose must be rigid (camera to world: an orthonormal rotation of determinant +1 and a translation)")
    return cam


def project_vertices(vertices, intrinsics, pose):
    """Stage A of the rasteriser (numpy twin of ``Engine.project_vertices``): world vertices [V,3] through the pinhole camera of
    ``data.get_rays`` -- x_cam = R^T (x - t), u = (K00 x + K01 y) / z + K02, v = K11 y / z + K12 in fp64, pixel (row i, column j)
    being the image point (u, v) = (j, i).  Returns (xy [V,2] int32 = rint(256 u), rint(256 v) clamped to +-2^22 (NaN -> 0),
    zc [V] float32 = the camera z, NaN for a vertex with a non-finite coordinate)."""
    cam = camera_params(intrinsics, pose)
    x = np.asarray(vertices, np.float32).reshape(-1, 3).astype(np.float64)
    R, t = cam[:9].reshape(3, 3), cam[9:12]
    with np.errstate(all="ignore"):
        d = x - t[None]
        c = [(R[0, i] * d[:, 0] + R[1, i] * d[:, 1]) + R[2, i] * d[:, 2] for i in range(3)]
        u = (cam[12] * c[0] + cam[13] * c[1]) / c[2] + cam[14]
        v = cam[15] * c[1] / c[2] + cam[16]
        q = np.stack([u, v], -1) * float(RAST_SUBPIXEL)
        q = np.where(np.isnan(q), 0.0, np.clip(q, -float(RAST_GUARD), float(RAST_GUARD)))
        ok = np.isfinite(x).all(axis=1) & np.isfinite(c[2])
        zc = np.where(ok, c[2], np.nan).astype(np.float32)
    return np.rint(q).astype(np.int32), zc


def _rast_setup(xy, zc, tri, H, W, near, cull):
    """Per triangle: reason (0 = drawn, 1 + index into RAST_REASONS otherwise), pixel box [T,4] = jmin, jmax, imin, imax, and the
    number of 8 x 8 tiles the box touches."""
    V, T = len(zc), len(tri)
    reason = np.zeros(T, np.int64)
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    bad = (tri < 0).any(1) | (tri >= V).any(1) | (a == b) | (b == c) | (a == c)
    s = np.where(bad[:, None], 0, tri)
    if V == 0:          # (every triangle is invalid: one row to index)
        xy, zc = np.zeros((1, 2), np.int32), np.zeros(1, np.float32)
    p = xy[s].astype(np.int64)                                                  # [T,3,2]
    z = zc[s].astype(np.float64)
    with np.errstate(invalid="ignore"):
        behind = ~(z > near).all(1)
    area = (p[:, 1, 0] - p[:, 0, 0]) * (p[:, 2, 1] - p[:, 0, 1]) - (p[:, 1, 1] - p[:, 0, 1]) * (p[:, 2, 0] - p[:, 0, 0])
    culled = ((cull == 1) & (area > 0)) | ((cull == 2) & (area < 0))          # the front of a triangle has a NEGATIVE screen area (y down)
    S = RAST_SUBPIXEL
    jmin = np.clip(-((-p[..., 0].min(1)) // S), 0, None)
    jmax = np.clip(p[..., 0].max(1) // S, None, W - 1)
    imin = np.clip(-((-p[..., 1].min(1)) // S), 0, None)
    imax = np.clip(p[..., 1].max(1) // S, None, H - 1)
    off = (jmin > jmax) | (imin > imax)
    for code, m in ((5, off), (4, culled), (3, area == 0), (2, behind), (1, bad)):          # the first test that fires names the reason
        reason[m] = code
    tiles = np.where(reason == 0, ((jmax >> 3) - (jmin >> 3) + 1) * ((imax >> 3) - (imin >> 3) + 1), 0)
    return reason, np.stack([jmin, jmax, imin, imax], 1), tiles, p, z, area


def rasterize_projected(xy, zc, triangles, height, width, attributes=None, near=1e-6, cull="none", runner_up=False, chunk=1 << 22):
    """Stage B of the rasteriser, the specification of csrc/raster.hip: a pure function of the snapped vertices.

    A triangle is rejected when an index repeats or lies outside [0, V) (``invalid``), a corner has ``zc`` not > ``near`` (no clipping:
    the whole triangle goes, ``near_rejected``), its doubled fixed-point area A = (p1 - p0) x (p2 - p0) is 0 (``zero_area``), or by
    ``cull`` (``culled``: "back" drops A > 0, "front" A < 0 -- with the image's y axis pointing down, the side the normal
    (v1 - v0) x (v2 - v0) points to is seen with A < 0); ``offscreen`` counts drawn triangles whose box holds no pixel centre.
    Coverage of the pixel centre P = (256 j, 256 i): with s = sign(A) and, for the edge from a to b opposite corner k,
    E_k = (bx - ax)(Py - ay) - (by - ay)(Px - ax), the pixel is covered iff for every k  s E_k > 0, or E_k == 0 and the edge d = s (b - a)
    is a left edge (dy < 0) or a top edge (dy == 0, dx > 0).  That is the sign of s E_k at P + (eps, eps^2): a centre on a shared edge,
    or on a vertex of a closed fan, belongs to exactly one triangle.
    Depth (fp64 from the exact integers, no multiply feeds an add): l_k = E_k / A, w_k = l_k / zc_k, z = 1 / ((w_0 + w_1) + w_2),
    b_k = w_k z.  The visible triangle has the smallest (bits of float32(z), index) pair.

    Returns a dict: ``depth`` [H,W] float32 (+inf: nothing), ``triangle`` [H,W] int32 (-1), ``bary`` [H,W,3] float32 (0),
    ``attributes`` [H,W,C] float32 = (b_0 a_0 + b_1 a_1) + b_2 a_2 in fp32 (0; C = 0 without attributes), ``stats``; with ``runner_up``
    also ``second_depth`` [H,W] float32 (+inf), the depth of the second smallest pair."""
    H, W = int(height), int(width)
    if not (1 <= H <= RAST_MAX_SIZE and 1 <= W <= RAST_MAX_SIZE):
        raise ValueError(f"height and width must be in 1..{RAST_MAX_SIZE}")
    if cull not in RAST_CULL:
        raise ValueError(f"cull must be one of {sorted(RAST_CULL)}")
    near = float(near)
    if not (near >= 0.0 and np.isfinite(near)):
        raise ValueError("near must be finite and >= 0")
    xy = np.asarray(xy, np.int32).reshape(-1, 2)
    zc = np.asarray(zc, np.float32).reshape(-1)
    tri = np.asarray(triangles)
    tri = (np.zeros((0, 3), np.int64) if tri.size == 0 else tri.astype(np.int64)).reshape(-1, 3)
    V, T = len(zc), len(tri)
    if len(xy) != V or V >= 1 << 31 or T >= 1 << 31:
        raise ValueError("xy [V,2] and zc [V] must agree, and V, T must be below 2^31")
    att = None
    if attributes is not None:
        att = np.asarray(attributes, np.float32)
        if att.ndim != 2 or att.shape[0] != V or not 1 <= att.shape[1] <= RAST_MAX_ATTRS:
            raise ValueError(f"attributes must be [V, 1..{RAST_MAX_ATTRS}]")
    C = 0 if att is None else att.shape[1]
    reason, box, tiles, p, z, area = _rast_setup(xy, zc, tri, H, W, near, RAST_CULL[cull])
    stats = {name: int((reason == i + 1).sum()) for i, name in enumerate(RAST_REASONS)}
    stats.update(triangles=T, work_items=int(tiles.sum()))
    if stats["work_items"] >= 1 << 31:
        raise ValueError("2^31 work items or more")
    EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
    ids = np.nonzero(reason == 0)[0]
    nj, ni = box[ids, 1] - box[ids, 0] + 1, box[ids, 3] - box[ids, 2] + 1
    cand = nj * ni
    pix_all, key_all = [np.zeros(0, np.int64)], [np.zeros(0, np.uint64)]
    start = 0
    while start < len(ids):          # runs of triangles with at most ``chunk`` box pixels together
        csum = np.cumsum(cand[start:])
        stop = start + max(1, int(np.searchsorted(csum, chunk, side="right")))
        sel, n = ids[start:stop], cand[start:stop]
        which = np.repeat(np.arange(len(sel)), n)
        local = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)
        t = sel[which]
        j = box[t, 0] + local % nj[start:stop][which]
        i = box[t, 2] + local // nj[start:stop][which]
        Px, Py = j * RAST_SUBPIXEL, i * RAST_SUBPIXEL
        q, s = p[t], np.sign(area[t])
        E, inside = [], np.ones(len(t), bool)
        for k in range(3):
            a, b = q[:, (k + 1) % 3], q[:, (k + 2) % 3]
            dx, dy = b[:, 0] - a[:, 0], b[:, 1] - a[:, 1]
            e = dx * (Py - a[:, 1]) - dy * (Px - a[:, 0])
            E.append(e)
            owns = (s * dy < 0) | ((dy == 0) & (s * dx > 0))
            inside &= (s * e > 0) | ((e == 0) & owns)
        t, i, j = t[inside], i[inside], j[inside]
        A = area[t].astype(np.float64)
        w = [(E[k][inside].astype(np.float64) / A) / z[t, k] for k in range(3)]
        depth = (1.0 / ((w[0] + w[1]) + w[2])).astype(np.float32)
        key_all.append((depth.view(np.uint32).astype(np.uint64) << np.uint64(32)) | t.astype(np.uint64))
        pix_all.append(i * W + j)
        start = stop
    pix, key = np.concatenate(pix_all), np.concatenate(key_all)
    order = np.lexsort((key, pix))
    pix, key = pix[order], key[order]
    first = np.ones(len(pix), bool)
    first[1:] = pix[1:] != pix[:-1]
    zbuf = np.full(H * W, EMPTY, np.uint64)
    zbuf[pix[first]] = key[first]
    hit = zbuf != EMPTY
    tid = np.where(hit, zbuf & np.uint64(0xFFFFFFFF), 0).astype(np.int64)
    out_depth = np.where(hit, (zbuf >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(np.inf)).astype(np.float32)
    bary = np.zeros((H * W, 3), np.float32)
    attr = np.zeros((H * W, C), np.float32)
    hp = np.nonzero(hit)[0]
    if len(hp):          # the winner's weights again, as the resolve kernel recomputes them
        t = tid[hp]
        Px, Py = (hp % W) * RAST_SUBPIXEL, (hp // W) * RAST_SUBPIXEL
        q, A = p[t], area[t].astype(np.float64)
        w = []
        for k in range(3):
            a, b = q[:, (k + 1) % 3], q[:, (k + 2) % 3]
            e = (b[:, 0] - a[:, 0]) * (Py - a[:, 1]) - (b[:, 1] - a[:, 1]) * (Px - a[:, 0])
            w.append((e.astype(np.float64) / A) / z[t, k])
        zz = 1.0 / ((w[0] + w[1]) + w[2])
        b32 = np.stack([w[k] * zz for k in range(3)], -1).astype(np.float32)
        bary[hp] = b32
        if C:
            a3 = att[tri[t]]                                                     # [n,3,C]
            attr[hp] = (b32[:, 0:1] * a3[:, 0] + b32[:, 1:2] * a3[:, 1]) + b32[:, 2:3] * a3[:, 2]
    stats["covered_pixels"] = int(hit.sum())
    out = {"depth": out_depth.reshape(H, W), "triangle": np.where(hit, tid, -1).astype(np.int32).reshape(H, W), "bary": bary.reshape(H, W, 3),
           "attributes": attr.reshape(H, W, C), "stats": stats}
    if runner_up:
        second = np.zeros(len(pix), bool)
        second[1:] = first[:-1] & ~first[1:]
        sd = np.full(H * W, np.inf, np.float32)
        sd[pix[second]] = (key[second] >> np.uint64(32)).astype(np.uint32).view(np.float32)
        out["second_depth"] = sd.reshape(H, W)
    return out


def rasterize(vertices, triangles, intrinsics, pose, height, width, attributes=None, near=1e-6, cull="none", runner_up=False):
    """A triangle mesh as depth / triangle-id / barycentric / interpolated-attribute images of a pinhole camera (numpy twin of
    ``Engine.rasterize``): ``project_vertices`` then ``rasterize_projected``, whose docstrings are the contract.  One sample per pixel,
    at the point ``data.get_rays`` casts the pixel's ray through; depth is the camera z (``data.depth_points``' convention)."""
    xy, zc = project_vertices(vertices, intrinsics, pose)
    return rasterize_projected(xy, zc, triangles, height, width, attributes, near, cull, runner_up)


def vertex_normals(vertices, triangles):
    """Area-weighted vertex normals of an indexed mesh (unit length; 0 for a vertex of no triangle with an area)."""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    f = np.asarray(triangles, np.int64).reshape(-1, 3)
    n = np.zeros_like(v)
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    for k in range(3):
        np.add.at(n, f[:, k], fn)
    return (n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-30)).astype(np.float32)


# ---- mesh export: clean-up and vertex clustering (host twins of csrc/mesh.hip es_mesh_clean_* and csrc/export.hip) ------
def _clean_keep(tri):
    """(keep [T] bool, degenerate [T] bool) of checked int64 triangles: the rule of ``mesh_clean``."""
    good = (tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])
    keep = np.zeros(len(tri), bool)
    ids = np.nonzero(good)[0]
    if len(ids):
        _, first = np.unique(np.sort(tri[ids], axis=1), axis=0, return_index=True)          # the first occurrence of each corner set
        keep[ids[first]] = True
    return keep, ~good


def mesh_clean(vertices, triangles, compact=False):
    """The mesh without its degenerate and duplicate triangles (numpy twin of ``Engine.mesh_clean``; what Open3D's
    ``remove_degenerate_triangles`` and ``remove_duplicated_triangles`` do together).

    A triangle with a repeated index is degenerate and goes.  Two triangles are duplicates when they name the same three vertices, in
    any rotation and either orientation; of a set of duplicates the one with the smallest triangle index stays.  Surviving triangles
    keep their input order and their own orientation.  ``compact=True`` also drops the vertices no surviving triangle uses and
    renumbers; ``compact=False`` keeps every vertex.  Indices are compared as integers: nothing is folded for V, T < 2^31.
    Returns (vertices [V', 3], triangles [T', 3] int32, vertex_map [V'] int64: the old index of each new vertex (the convention of
    ``keep_components``), stats: degenerate, duplicates, kept_triangles)."""
    verts = np.asarray(vertices)
    if verts.ndim != 2 or verts.shape[1] != 3:
        raise ValueError(f"vertices must be [V, 3] (got {verts.shape})")
    tri, V = _as_triangles(triangles, len(verts))
    keep, degenerate = _clean_keep(tri)
    used = np.ones(V, bool)
    if compact:
        used = np.zeros(V, bool)
        used[tri[keep].reshape(-1)] = True
    vmap = np.nonzero(used)[0].astype(np.int64)
    new_id = np.cumsum(used) - 1
    n_deg, n_keep = int(degenerate.sum()), int(keep.sum())
    stats = {"degenerate": n_deg, "duplicates": len(tri) - n_deg - n_keep, "kept_triangles": n_keep}
    return verts[vmap], new_id[tri[keep]].astype(np.int32).reshape(-1, 3), vmap, stats


CLUSTER_MAX_ATTRS = 8
CLUSTER_HALF = 1 << 20               # cell coordinates lie in [-2^20, 2^20): three of them pack into one 63-bit key


def cluster_vertices(vertices, triangles, cell, origin=(0.0, 0.0, 0.0), attributes=None):
    """Vertex clustering (numpy twin of ``Engine.cluster_vertices``; the averaging variant of Open3D's ``simplify_vertex_clustering``).

    The cell of a vertex is floor((float64(v) - origin) / cell) per axis (v the fp32 coordinate; one subtraction and one division in
    fp64).  Every cell coordinate must lie in [-2^20, 2^20) -- ValueError otherwise, as for a vertex that is not finite.  Each occupied
    cell becomes one vertex; cells are numbered by ascending (ix, iy, iz), ix most significant.  Its position is the fp64 sum of its
    members' positions, added in ascending old index, divided by their number and rounded to fp32; ``attributes`` [V, C], 1 <= C <= 8
    (colours, normals) are averaged the same way.  The triangles are renumbered and then cleaned by the rule of ``mesh_clean`` (a
    triangle with two corners in one cell, and duplicates, go; order kept; every new vertex stays, used or not).
    Returns (vertices [V', 3] float32, triangles [T', 3] int32, attributes [V', C] float32 or None, vertex_cluster [V] int32: the new
    vertex of each old one, stats: cells, largest_cell, degenerate, duplicates, kept_triangles)."""
    verts = np.ascontiguousarray(np.asarray(vertices, np.float32))
    if verts.ndim != 2 or verts.shape[1] != 3:
        raise ValueError(f"vertices must be [V, 3] (got {verts.shape})")
    tri, V = _as_triangles(triangles, len(verts))
    cell = float(cell)
    org = np.asarray(origin, np.float64).reshape(-1)
    if not (cell > 0.0 and np.isfinite(cell)) or org.shape != (3,) or not np.isfinite(org).all():
        raise ValueError("cell must be finite and positive, origin three finite numbers")
    att = None
    if attributes is not None:
        att = np.asarray(attributes, np.float32)
        if att.ndim != 2 or att.shape[0] != V or not 1 <= att.shape[1] <= CLUSTER_MAX_ATTRS:
            raise ValueError(f"attributes must be [V, 1..{CLUSTER_MAX_ATTRS}]")
    with np.errstate(invalid="ignore", over="ignore"):
        idx = np.floor((verts.astype(np.float64) - org[None]) / cell)
    if not ((idx >= -CLUSTER_HALF) & (idx < CLUSTER_HALF)).all():          # (NaN fails both)
        raise ValueError("a vertex's cell coordinate lies outside [-2^20, 2^20) (or the vertex is not finite): use a larger cell")
    q = idx.astype(np.int64) + CLUSTER_HALF
    key = (q[:, 0] << 42) | (q[:, 1] << 21) | q[:, 2]
    order = np.argsort(key, kind="stable")                                   # by (cell, old index)
    cells, cluster_sorted, counts = np.unique(key[order], return_inverse=True, return_counts=True)
    cluster_sorted = cluster_sorted.reshape(-1)
    n = len(cells)

    def mean(x):          # np.add.at adds one row after the other, in the order given: ascending old index within a cell
        acc = np.zeros((n, x.shape[1]), np.float64)
        np.add.at(acc, cluster_sorted, x[order].astype(np.float64))
        return (acc / counts[:, None].astype(np.float64)).astype(np.float32)

    vertex_cluster = np.zeros(V, np.int64)
    vertex_cluster[order] = cluster_sorted
    keep, degenerate = _clean_keep(vertex_cluster[tri].reshape(-1, 3))
    n_deg, n_keep = int(degenerate.sum()), int(keep.sum())
    stats = {"cells": n, "largest_cell": int(counts.max()) if n else 0, "degenerate": n_deg, "duplicates": len(tri) - n_deg - n_keep,
             "kept_triangles": n_keep}
    return (mean(verts), vertex_cluster[tri[keep]].astype(np.int32).reshape(-1, 3), None if att is None else mean(att),
            vertex_cluster.astype(np.int32), stats)
