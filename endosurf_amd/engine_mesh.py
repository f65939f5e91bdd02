"""The geometry methods of ``engine.Engine`` (a mixin): iso-surface, narrow band, components, distances, mesh export, rasteriser."""
from __future__ import annotations

import ctypes as C

import torch

from ._device import f32
from ._lib import EndoSurfHipError, check, ptr
from .meshing import RAST_CULL, RAST_MAX_ATTRS, RAST_MAX_SIZE, RAST_REASONS, band_margin, camera_params


class MeshMixin:
    def _scratch_bytes(self, fn_name, *dims):
        """What ``es_*_scratch_bytes`` answers for ``dims``; its -1 (sizes the library refuses) raises with the library's message."""
        nbytes = int(getattr(self.lib, fn_name)(*dims))
        if nbytes < 0:
            check(1, fn_name)
        return nbytes

    def _scratch(self, fn_name, *dims):
        return self.empty(self._scratch_bytes(fn_name, *dims), dtype=torch.uint8)

    def _tri_arg(self, tris, what):
        """``tris`` as the library reads it: int32 [T, 3], contiguous, on this device."""
        if not torch.is_tensor(tris) or tris.dim() != 2 or tris.shape[1] != 3 or tris.device != self.device \
                or tris.dtype not in (torch.int32, torch.int64):
            got = f"{tris.dtype} {tuple(tris.shape)} on {tris.device}" if torch.is_tensor(tris) else type(tris).__name__
            raise EndoSurfHipError(f"{what} takes [T, 3] int32 / int64 triangles on {self.device} (got {got})")
        return tris.detach().to(torch.int32).contiguous()

    def _rows3_arg(self, t, what, rows):
        """``t`` ([N, 3] on this device; ``rows`` names it in the message) as the library reads it: fp32, contiguous."""
        if t.dim() != 2 or t.shape[1] != 3 or t.device != self.device:
            raise EndoSurfHipError(f"{what} takes {rows} on {self.device} (got {tuple(t.shape)} on {t.device})")
        return f32(t)

    def _attrs_arg(self, attributes, V, what):
        """Per-vertex ``attributes`` ([V, 1..RAST_MAX_ATTRS] on this device, or None) as the library reads them, and their width (0)."""
        if attributes is None:
            return None, 0
        if attributes.dim() != 2 or attributes.shape[0] != V or not 1 <= attributes.shape[1] <= RAST_MAX_ATTRS or attributes.device != self.device:
            raise EndoSurfHipError(f"{what} takes [V, 1..{RAST_MAX_ATTRS}] attributes on {self.device} (got {tuple(attributes.shape)})")
        return f32(attributes), int(attributes.shape[1])

    # ---- iso-surface extraction (csrc/iso.hip, csrc/cubes.hip) ----------------------------------------
    ISO_METHODS = {"tetrahedra": "es_iso", "cubes": "es_cubes"}          # method -> the prefix of its three library calls

    def iso_surface(self, field: torch.Tensor, threshold: float = 0.0, method: str = "tetrahedra"):
        """The level set ``field == threshold`` of a device field [nx, ny, nz] as a welded, oriented triangle mesh, triangulated like
        ``meshing.marching_tetrahedra``: (verts [V,3] fp32 in index coordinates, tris [T,3] int32, edge_ends [V,2] int32 = linear grid
        ids of each vertex's inside and outside end), all on the device.  The two counts are the only thing read back to the host.
        ``method="cubes"`` triangulates like ``meshing.marching_cubes`` instead (csrc/cubes.hip: this project's cube table): the
        vertices on the grid's axis edges only, bit for bit those the default method puts there, about a third of the vertices and
        triangles."""
        if method not in self.ISO_METHODS:
            raise EndoSurfHipError(f"iso_surface: method must be one of {sorted(self.ISO_METHODS)} (got {method!r})")
        if field.dim() != 3 or field.device != self.device:
            raise EndoSurfHipError(f"iso_surface takes a [nx, ny, nz] field on {self.device} (got {tuple(field.shape)} on {field.device})")
        fn = {k: f"{self.ISO_METHODS[method]}_{k}" for k in ("scratch_bytes", "count", "emit")}
        u = f32(field)
        nx, ny, nz = (int(s) for s in u.shape)
        scratch, totals = self._scratch(fn["scratch_bytes"], nx, ny, nz), self.empty(2, dtype=torch.int64)
        check(getattr(self.lib, fn["count"])(ptr(u), nx, ny, nz, float(threshold), ptr(scratch), ptr(totals), self.st()), fn["count"])
        V, T = (int(v) for v in totals.tolist())
        if max(V, T) >= 1 << 31:
            raise EndoSurfHipError(f"iso_surface: {V} vertices / {T} triangles do not fit int32 indices")
        verts, ends, tris = self.empty(V, 3), self.empty(V, 2, dtype=torch.int32), self.empty(T, 3, dtype=torch.int32)
        check(getattr(self.lib, fn["emit"])(ptr(u), nx, ny, nz, float(threshold), ptr(scratch), V, T, ptr(verts), ptr(ends), ptr(tris), self.st()),
              fn["emit"])
        return verts, tris, ends

    # ---- narrow-band field (csrc/band.hip) ---------------------------------------------------------------
    def band_field(self, sample, axes, threshold: float = 0.0, block: int = 8, lipschitz: float = 1.0, max_fraction: float = 0.5,
                   net_chunk: int = 1 << 22):
        """A device field [nx, ny, nz] on the lattice ``axes`` (three 1-D fp32 device tensors) whose ``iso_surface`` is the one of the
        densely sampled field, built from ``sample(x[M,3]) -> [M]`` (any device callable) evaluated near the level set only: the scheme,
        its exactness contract and its limit are those of ``meshing.band_field``, the numpy twin of this method (same block sets, same
        values; the kernels are csrc/band.hip).  ``sample`` sees at most ``net_chunk`` points per call and must give a point the same
        value whatever batch it arrives in.  The host reads two integers per round (the seeds, then each growth round).
        Returns (field, stats, block_round [nbx, nby, nbz] int32: 0 = never evaluated, 1 = seed, r = activated by growth round r - 1);
        ``stats``: dense_points, evaluated_points (coarse lattice and duplicated face points included), blocks, seed_blocks,
        active_blocks, rounds, fallback."""
        if len(axes) != 3 or any(a.dim() != 1 or a.device != self.device for a in axes):
            raise EndoSurfHipError(f"band_field takes three 1-D axes on {self.device}")
        ax = [f32(a) for a in axes]
        nx, ny, nz = (int(a.shape[0]) for a in ax)
        B, thr, chunk = int(block), float(threshold), max(1, int(net_chunk))
        scratch = self._scratch("es_band_scratch_bytes", nx, ny, nz, B)
        nb = [-(-(n - 1) // B) for n in (nx, ny, nz)]
        NB, N, Nc = nb[0] * nb[1] * nb[2], nx * ny * nz, (nb[0] + 1) * (nb[1] + 1) * (nb[2] + 1)
        ends = torch.stack([torch.stack([a[0], a[-1]]) for a in ax]).tolist()          # (one small read: the world size of a block)
        margin = band_margin(ends, (nx, ny, nz), B, lipschitz)
        totals = self.empty(2, dtype=torch.int64)
        axp, st = [ptr(a) for a in ax], self.st()

        def lattice(stride, total, out):          # sample the (coarse) lattice in runs of ``chunk`` points
            for p0 in range(0, total, chunk):
                c = min(chunk, total - p0)
                x = self.empty(c, 3)
                check(self.lib.es_band_lattice_points(*axp, nx, ny, nz, stride, p0, c, ptr(x), st), "es_band_lattice_points")
                out[p0:p0 + c] = sample(x).reshape(-1)

        coarse = self.empty(Nc)
        lattice(B, Nc, coarse)
        check(self.lib.es_band_seed(ptr(coarse), nx, ny, nz, B, thr, margin, ptr(scratch), ptr(totals), st), "es_band_seed")
        n_list, n_pts = (int(v) for v in totals.tolist())
        stats = {"dense_points": N, "evaluated_points": Nc, "blocks": NB, "seed_blocks": n_list, "active_blocks": n_list, "rounds": 0, "fallback": False}
        field = self.empty(N)
        block_round = scratch[:4 * NB].view(torch.int32).view(*nb)
        if n_list > float(max_fraction) * NB:          # the band cannot win: sample the lattice itself
            lattice(1, N, field)
            stats.update(evaluated_points=Nc + N, active_blocks=NB, fallback=True)
            return field.view(nx, ny, nz), stats, block_round.clone()
        check(self.lib.es_band_fill(nx, ny, nz, B, ptr(scratch), ptr(field), st), "es_band_fill")
        r = 1
        while n_list:
            for m0 in range(0, n_pts, chunk):
                c = min(chunk, n_pts - m0)
                x = self.empty(c, 3)
                check(self.lib.es_band_points(*axp, nx, ny, nz, B, ptr(scratch), n_list, m0, c, ptr(x), st), "es_band_points")
                vals = f32(sample(x).reshape(-1))
                check(self.lib.es_band_scatter(ptr(vals), nx, ny, nz, B, ptr(scratch), n_list, m0, c, ptr(field), st), "es_band_scatter")
            stats["evaluated_points"] += n_pts
            check(self.lib.es_band_grow(ptr(field), nx, ny, nz, B, thr, r, ptr(scratch), ptr(totals), st), "es_band_grow")
            n_list, n_pts = (int(v) for v in totals.tolist())
            stats["active_blocks"] += n_list
            stats["rounds"] += 1 if n_list else 0
            r += 1
        return field.view(nx, ny, nz), stats, block_round.clone()

    def iso_surface_band(self, sample, axes, threshold: float = 0.0, block: int = 8, lipschitz: float = 1.0, max_fraction: float = 0.5,
                         net_chunk: int = 1 << 22, method: str = "tetrahedra"):
        """``iso_surface`` of the field ``sample`` takes on the lattice ``axes``, sampled near the level set only (``band_field``):
        (verts, tris, edge_ends, stats).  The mesh holds, complete and bit-identical, every vertex-connected component of the dense
        lattice's mesh that crosses a seed block: all of it when |grad u| <= ``lipschitz`` holds in the blocks that were culled.  With
        a smaller ``lipschitz`` (0 = sign changes of the block corners only) a closed component smaller than a block that no block
        corner sees can be lost.  ``method`` is ``iso_surface``'s: the band field guarantees the inside flags of every grid point a
        crossing tetrahedron edge touches, and the cube triangulation's axis edges are among those."""
        if method not in self.ISO_METHODS:
            raise EndoSurfHipError(f"iso_surface_band: method must be one of {sorted(self.ISO_METHODS)} (got {method!r})")
        field, stats, _ = self.band_field(sample, axes, threshold, block, lipschitz, max_fraction, net_chunk)
        verts, tris, ends = self.iso_surface(field, threshold, method)
        return verts, tris, ends, stats

    # ---- connected components, largest-component filter, nearest neighbour (csrc/mesh.hip) ----------------------------
    def _mesh_args(self, tris, n_verts, what):
        """``tris`` as the library reads it (int32 [T, 3], contiguous, on this device) and V, checked: one read-back of the index range."""
        t32 = self._tri_arg(tris, what)
        V, T = int(n_verts), int(t32.shape[0])
        if V < 0 or V >= 1 << 31 or T >= 1 << 31:
            raise EndoSurfHipError(f"{what}: {V} vertices / {T} triangles do not fit int32 indices")
        if T:
            lo, hi = (int(v) for v in torch.stack([tris.min(), tris.max()]).tolist())
            if lo < 0 or hi >= V:
                raise EndoSurfHipError(f"{what}: triangle indices {lo}..{hi} outside [0, {V})")
        return t32, V, T

    def _mesh_components(self, t32, V, T, scratch):
        st = self.st()
        changed, totals = self.empty(1, dtype=torch.int32), self.empty(3, dtype=torch.int64)
        vlabel, tlabel, counts = (self.empty(n, dtype=torch.int32) for n in (V, T, V))
        check(self.lib.es_mesh_cc_begin(ptr(t32), V, T, ptr(scratch), st), "es_mesh_cc_begin")
        rounds = 0
        while True:          # the fixed point is reached in O(log V) rounds on meshes; V rounds always suffice (each joins two trees)
            check(self.lib.es_mesh_cc_round(ptr(t32), V, T, ptr(scratch), ptr(changed), st), "es_mesh_cc_round")
            rounds += 1
            if not int(changed.item()):
                break
            if rounds > V + 1:
                raise EndoSurfHipError(f"mesh_components did not reach its fixed point in {rounds} rounds")
        check(self.lib.es_mesh_cc_finish(ptr(t32), V, T, ptr(scratch), ptr(vlabel), ptr(tlabel), ptr(counts), ptr(totals), st), "es_mesh_cc_finish")
        ncomp, biggest, degenerate = (int(v) for v in totals.tolist())
        stats = {"components": ncomp, "max_triangles": biggest, "kept_triangles": T - degenerate, "degenerate": degenerate, "rounds": rounds}
        return vlabel, tlabel, counts, stats

    def _mesh_keep_emit(self, v32, t32, V, T, scratch, totals, st):
        """The tail of ``keep_components`` and ``_mesh_clean``: (verts, tris, vertex_map, the counts read from ``totals``: V', T' first)."""
        counts = [int(v) for v in totals.tolist()]
        V2, T2 = counts[:2]
        verts_out, tris_out, vmap = self.empty(V2, 3), self.empty(T2, 3, dtype=torch.int32), self.empty(V2, dtype=torch.int64)
        check(self.lib.es_mesh_keep_emit(ptr(v32), ptr(t32), V, T, ptr(scratch), V2, T2, ptr(verts_out), ptr(tris_out), ptr(vmap), st), "es_mesh_keep_emit")
        return verts_out, tris_out, vmap, counts

    def mesh_components(self, tris: torch.Tensor, n_verts: int):
        """Connected components of a device mesh, by the rule of ``meshing.mesh_components`` (its numpy twin): vertex connectivity,
        degenerate triangles join nothing, label = the smallest vertex index of the component.  (vertex_label [V], triangle_label [T]
        (-1 = degenerate), component_triangles [V], stats), int32 device tensors; ``stats``: components (with a triangle),
        max_triangles, kept_triangles (= the non-degenerate ones here), degenerate, rounds.  The host reads one integer per round."""
        t32, V, T = self._mesh_args(tris, n_verts, "mesh_components")
        return self._mesh_components(t32, V, T, self._scratch("es_mesh_scratch_bytes", V, T))

    def keep_components(self, verts: torch.Tensor, tris: torch.Tensor, keep_ratio: float = 0.9, compact: bool = True):
        """The mesh without the triangles of small components (``meshing.keep_components`` is the numpy twin and the specification):
        a triangle stays iff it is not degenerate and its component has at least ``keep_ratio`` x the triangles of the largest one.
        (verts [V', 3], tris [T', 3] int32, vertex_map [V'] int64, stats); order is kept, ``vertex_map`` is the old index of each new
        vertex (``attr.index_select(0, vertex_map)`` moves per-vertex attributes along).  ``compact=False`` drops triangles only."""
        v32 = self._rows3_arg(verts, "keep_components", "[V, 3] vertices")
        ratio = float(keep_ratio)
        if not 0.0 <= ratio <= 1.0:
            raise EndoSurfHipError(f"keep_components: keep_ratio must be in [0, 1] (got {keep_ratio!r})")
        t32, V, T = self._mesh_args(tris, v32.shape[0], "keep_components")
        scratch, totals, st = self._scratch("es_mesh_scratch_bytes", V, T), self.empty(2, dtype=torch.int64), self.st()
        _, tlabel, counts, stats = self._mesh_components(t32, V, T, scratch)
        check(self.lib.es_mesh_keep_count(ptr(t32), V, T, ptr(tlabel), ptr(counts), ratio, stats["max_triangles"], int(bool(compact)),
                                          ptr(scratch), ptr(totals), st), "es_mesh_keep_count")
        verts_out, tris_out, vmap, kept = self._mesh_keep_emit(v32, t32, V, T, scratch, totals, st)
        stats["kept_triangles"] = kept[1]
        return verts_out, tris_out, vmap, stats

    def nearest(self, query: torch.Tensor, points: torch.Tensor):
        """Exact nearest neighbour of each ``query`` row among the rows of ``points`` ([Q, 3], [P, 3] on this device): (dist [Q] fp32,
        index [Q] int32) by the rule of ``meshing.nearest`` (the numpy twin): fp32 squared distance, ties to the smallest index,
        non-finite rows never an answer, inf / -1 where there is none; bit-identical from call to call.  No read-back."""
        q, p = self._rows3_arg(query, "nearest", "[N, 3] query"), self._rows3_arg(points, "nearest", "[N, 3] points")
        Q, P = int(q.shape[0]), int(p.shape[0])
        scratch, st = self._scratch("es_nn_scratch_bytes", P), self.st()
        dist, index = self.empty(Q), self.empty(Q, dtype=torch.int32)
        check(self.lib.es_nn_build(ptr(p), P, ptr(scratch), st), "es_nn_build")
        check(self.lib.es_nn_query(ptr(q), Q, P, ptr(scratch), ptr(dist), ptr(index), st), "es_nn_query")
        return dist, index

    # ---- point-cloud clean-up queries (csrc/cloud.hip; contract: DESIGN.md 7g) ---------------------------------------------------
    def _nn_grid(self, p32):
        """The scratch ``es_nn_build`` leaves for the rows of ``p32``."""
        scratch = self._scratch("es_nn_scratch_bytes", int(p32.shape[0]))
        check(self.lib.es_nn_build(ptr(p32), int(p32.shape[0]), ptr(scratch), self.st()), "es_nn_build")
        return scratch

    def self_nearest(self, points: torch.Tensor):
        """For each row of ``points`` [P, 3] its nearest other row: (dist [P] fp32, index [P] int32) by the rule of
        ``meshing.self_nearest`` (the numpy twin and the specification): the smallest (fp32 squared distance, index) over the finite
        rows j != i, so a duplicate of the point gives 0; inf / -1 for a non-finite row and for a row without another finite row.
        Bit-identical from call to call; no read-back."""
        p = self._rows3_arg(points, "self_nearest", "[N, 3] points")
        P = int(p.shape[0])
        dist, index = self.empty(P), self.empty(P, dtype=torch.int32)
        check(self.lib.es_cloud_self_nearest(ptr(p), P, ptr(self._nn_grid(p)), ptr(dist), ptr(index), self.st()), "es_cloud_self_nearest")
        return dist, index

    def radius_count(self, query: torch.Tensor, points: torch.Tensor, radius=None, cap: int = 0, radius_sq=None):
        """count [Q] int32 = the number of finite rows of ``points`` [P, 3] whose fp32 squared distance to the ``query`` row is <= r2, by
        the rule of ``meshing.radius_count`` (the numpy twin and the specification).  ``radius`` is a Python float or a 0-dim tensor on
        this device (no read-back either way) and is squared in fp32; ``radius_sq`` gives r2 itself instead.  A query that is a row of
        ``points`` counts itself; a non-finite query row, or r2 NaN or negative, gives 0; ``cap`` > 0 gives min(count, cap) and stops
        reading there.  Bit-identical from call to call."""
        q, p = self._rows3_arg(query, "radius_count", "[N, 3] query"), self._rows3_arg(points, "radius_count", "[N, 3] points")
        if (radius is None) == (radius_sq is None):
            raise EndoSurfHipError("radius_count takes either radius or radius_sq")
        cap = int(cap)
        if cap < 0:
            raise EndoSurfHipError(f"radius_count: cap must be >= 0 (got {cap})")
        r = torch.as_tensor(radius if radius_sq is None else radius_sq).to(self.device).float().reshape(-1)
        if r.numel() != 1:
            raise EndoSurfHipError(f"radius_count takes one radius (got {r.numel()} values)")
        r2 = (r * r if radius_sq is None else r).contiguous()
        Q, P = int(q.shape[0]), int(p.shape[0])
        count = self.empty(Q, dtype=torch.int32)
        check(self.lib.es_cloud_radius_count(ptr(q), Q, P, ptr(self._nn_grid(p)), ptr(r2), cap, ptr(count), self.st()), "es_cloud_radius_count")
        return count

    def radius_outlier_mask(self, points: torch.Tensor, nb_points: int, radius):
        """bool [P]: the rows of ``points`` with more than ``nb_points`` rows within ``radius``, themselves included
        (``meshing.radius_outlier_mask`` is the numpy twin and the specification); False for a non-finite row.  No read-back."""
        nb = int(nb_points)
        if nb < 0:
            raise EndoSurfHipError(f"radius_outlier_mask: nb_points must be >= 0 (got {nb_points!r})")
        return self.radius_count(points, points, radius, cap=nb + 1) > nb

    # ---- point-to-surface distance (csrc/surface.hip; contract: DESIGN.md 7f) ------------------------------------------------
    def point_to_mesh(self, points: torch.Tensor, vertices: torch.Tensor, triangles: torch.Tensor, return_work: bool = False):
        """Exact distance from each row of ``points`` [Q, 3] to the triangle mesh ``vertices`` [V, 3] / ``triangles`` [T, 3] (int32 or
        int64), all on this device: (dist [Q] fp32, triangle [Q] int32, closest [Q, 3] fp32) by the rule of ``meshing.point_to_mesh``
        (the numpy twin and the specification), evaluated in fp64.  A triangle with a repeated or out-of-range index or a non-finite
        corner is skipped, not an error; inf / -1 / nan where there is no answer (a non-finite query row, no triangle that takes
        part).  Bit-identical from call to call; no read-back.  ``return_work=True`` appends work [Q, 2] int32: the cell shells a
        query read and the triangles it measured."""
        q = self._rows3_arg(points, "point_to_mesh", "[N, 3] points")
        v = self._rows3_arg(vertices, "point_to_mesh", "[N, 3] vertices")
        Q, V, t = int(q.shape[0]), int(v.shape[0]), triangles
        if torch.is_tensor(t) and t.dtype == torch.int64:          # an index beyond int32 must stay out of range, not wrap into it
            t = torch.where((t < 0) | (t >= V), torch.full_like(t, -1), t)
        t32 = self._tri_arg(t, "point_to_mesh")          # (not _mesh_args: no read-back, and a bad index is skipped, not an error)
        T = int(t32.shape[0])
        scratch, st = self._scratch("es_surf_scratch_bytes", V, T), self.st()
        dist, tri, closest = self.empty(Q), self.empty(Q, dtype=torch.int32), self.empty(Q, 3)
        work = self.empty(Q, 2, dtype=torch.int32) if return_work else None
        check(self.lib.es_surf_build(ptr(v), ptr(t32), V, T, ptr(scratch), st), "es_surf_build")
        check(self.lib.es_surf_query(ptr(q), Q, ptr(v), ptr(t32), V, T, ptr(scratch), ptr(dist), ptr(tri), ptr(closest), ptr(work), st), "es_surf_query")
        return (dist, tri, closest, work) if return_work else (dist, tri, closest)

    # ---- mesh export: clean-up, normals, clustering, PLY body (csrc/mesh.hip, csrc/export.hip; contract: DESIGN.md 7e) ------
    def _mesh_clean(self, v32, t32, V, T, compact):
        """``mesh_clean`` of checked arguments.  The two stable sorts order the triangles by (sorted corners, triangle index)."""
        st, scratch = self.st(), self._scratch("es_mesh_scratch_bytes", V, T)
        key_hi, key_lo = self.empty(T, dtype=torch.int32), self.empty(T, dtype=torch.int64)
        check(self.lib.es_mesh_clean_keys(ptr(t32), V, T, ptr(key_hi), ptr(key_lo), st), "es_mesh_clean_keys")
        by_lo = torch.sort(key_lo, stable=True).indices
        order = by_lo[torch.sort(key_hi[by_lo], stable=True).indices].contiguous()
        totals = self.empty(3, dtype=torch.int64)
        check(self.lib.es_mesh_clean_count(ptr(t32), V, T, ptr(order), int(bool(compact)), ptr(scratch), ptr(totals), st), "es_mesh_clean_count")
        verts_out, tris_out, vmap, (_, T2, degenerate) = self._mesh_keep_emit(v32, t32, V, T, scratch, totals, st)
        return verts_out, tris_out, vmap, {"degenerate": degenerate, "duplicates": T - degenerate - T2, "kept_triangles": T2}

    def mesh_clean(self, vertices: torch.Tensor, triangles: torch.Tensor, compact: bool = False):
        """The mesh without its degenerate and duplicate triangles (``meshing.mesh_clean`` is the numpy twin and the specification; what
        Open3D's remove_degenerate_triangles + remove_duplicated_triangles do): a triangle with a repeated index goes, and of the
        triangles with the same three vertex indices, in any rotation or orientation, the one with the smallest triangle index stays.
        Survivors keep their order and their own orientation.  (verts [V', 3], tris [T', 3] int32, vertex_map [V'] int64, stats):
        ``compact=True`` also drops the vertices no surviving triangle uses and renumbers, ``vertex_map`` being the old index of each
        new vertex as in ``keep_components``; ``stats``: degenerate, duplicates, kept_triangles.  One read-back (three counts)."""
        v32 = self._rows3_arg(vertices, "mesh_clean", "[V, 3] vertices")
        t32, V, T = self._mesh_args(triangles, v32.shape[0], "mesh_clean")
        return self._mesh_clean(v32, t32, V, T, compact)

    def vertex_normals(self, vertices: torch.Tensor, triangles: torch.Tensor):
        """Area-weighted vertex normals [V, 3] fp32 of a device mesh, bit for bit those of ``meshing.vertex_normals`` (the numpy twin
        and the specification) for fp32 vertices: per vertex the fp64 sum of the un-normalised fp64 face cross products of its
        triangles, added in the twin's order (corner 0 of every triangle in triangle order, then corner 1, then corner 2), normalised;
        0 for a vertex of no triangle with an area.  No float atomics, no read-back."""
        v32 = self._rows3_arg(vertices, "vertex_normals", "[V, 3] vertices")
        t32, V, T = self._mesh_args(triangles, v32.shape[0], "vertex_normals")
        st, scratch = self.st(), self._scratch("es_vn_scratch_bytes", V)
        corner_vertex, normals = self.empty(3 * T, dtype=torch.int32), self.empty(V, 3)
        check(self.lib.es_vn_count(ptr(t32), V, T, ptr(corner_vertex), ptr(scratch), st), "es_vn_count")
        order = torch.sort(corner_vertex, stable=True).indices
        check(self.lib.es_vn_gather(ptr(v32), ptr(t32), V, T, ptr(order), ptr(scratch), ptr(normals), st), "es_vn_gather")
        return normals

    def cluster_vertices(self, vertices: torch.Tensor, triangles: torch.Tensor, cell: float, origin=(0.0, 0.0, 0.0), attributes=None):
        """Vertex clustering (``meshing.cluster_vertices`` is the numpy twin and the specification; the averaging variant of Open3D's
        simplify_vertex_clustering): the vertices of one cell floor((float64(v) - origin) / cell) become one vertex, their fp64 mean in
        ascending index rounded to fp32, numbered by ascending (ix, iy, iz); ``attributes`` [V, C <= 8] are averaged likewise; the
        triangles are renumbered and cleaned (``mesh_clean``: collapsed and duplicate triangles go, order kept).  Cell coordinates must
        lie in [-2^20, 2^20).  Returns (verts [V', 3], tris [T', 3] int32, attributes [V', C] or None, vertex_cluster [V] int32,
        stats: cells, largest_cell, degenerate, duplicates, kept_triangles).  Two read-backs (the cell counts, the clean-up's)."""
        v32 = self._rows3_arg(vertices, "cluster_vertices", "[V, 3] vertices")
        t32, V, T = self._mesh_args(triangles, v32.shape[0], "cluster_vertices")
        org = [float(o) for o in origin]
        if len(org) != 3:
            raise EndoSurfHipError(f"cluster_vertices: origin must have three entries (got {origin!r})")
        att, Cn = self._attrs_arg(attributes, V, "cluster_vertices")
        st, scratch = self.st(), self._scratch("es_cluster_scratch_bytes", V)
        key = self.empty(V, dtype=torch.int64)
        check(self.lib.es_cluster_keys(ptr(v32), V, float(cell), *org, ptr(key), st), "es_cluster_keys")
        sorted_key, order = torch.sort(key, stable=True)
        totals = self.empty(3, dtype=torch.int64)
        check(self.lib.es_cluster_count(ptr(sorted_key), V, ptr(scratch), ptr(totals), st), "es_cluster_count")
        cells, bad, largest = (int(v) for v in totals.tolist())
        verts_out, cluster, att_out = self.empty(cells, 3), self.empty(V, dtype=torch.int32), self.empty(cells, Cn) if Cn else None
        check(self.lib.es_cluster_emit(ptr(v32), ptr(att), Cn, V, ptr(order), ptr(scratch), cells, bad, ptr(verts_out), ptr(att_out), ptr(cluster), st),
              "es_cluster_emit")
        remapped = self.empty(T, 3, dtype=torch.int32)
        check(self.lib.es_cluster_remap(ptr(t32), V, T, ptr(cluster), ptr(remapped), st), "es_cluster_remap")
        _, tris_out, _, cstats = self._mesh_clean(verts_out, remapped, cells, T, False)
        return verts_out, tris_out, att_out, cluster, dict(cells=cells, largest_cell=largest, **cstats)

    def ply_pack(self, vertices: torch.Tensor, triangles=None, colors=None, normals=None):
        """The body of a ``binary_little_endian 1.0`` PLY file as a uint8 device tensor (``data.ply_body`` is the numpy twin, and
        ``data.ply_header`` the text in front of it): per vertex ``float x y z``, then ``float nx ny nz`` with ``normals`` [V, 3], then
        ``uchar red green blue`` with ``colors`` [V, 3] -- floats quantised by the rule of ``data.to8b``, trunc(255 clip(c, 0, 1)) in
        fp32: below 0 gives 0, above 1 gives 255, NaN 0 --; then per triangle ``uchar 3`` and three ``int`` indices (13 bytes).
        ``triangles=None`` packs a point cloud.  No read-back."""
        v32 = self._rows3_arg(vertices, "ply_pack", "[V, 3] vertices")
        V = int(v32.shape[0])
        t32 = None if triangles is None else self._tri_arg(triangles, "ply_pack")
        T = 0 if t32 is None else int(t32.shape[0])
        rows = {name: None if a is None else self._rows3_arg(a, "ply_pack", f"[V, 3] {name}") for name, a in (("normals", normals), ("colors", colors))}
        for name, r in rows.items():
            if r is not None and r.shape[0] != V:
                raise EndoSurfHipError(f"ply_pack: {name} has {r.shape[0]} rows for {V} vertices")
        out = self.empty(self._scratch_bytes("es_ply_body_bytes", V, T, int(normals is not None), int(colors is not None)), dtype=torch.uint8)
        check(self.lib.es_ply_pack(ptr(v32), ptr(rows["normals"]), ptr(rows["colors"]), ptr(t32), V, T, ptr(out), self.st()), "es_ply_pack")
        return out

    # ---- mesh rasteriser (csrc/raster.hip) ------------------------------------------------------------------------------
    def project_vertices(self, vertices: torch.Tensor, intrinsics, pose):
        """Stage A of the rasteriser (``meshing.project_vertices`` is the numpy twin and the specification): world vertices [V, 3]
        through the pinhole camera ``intrinsics`` ([3,3] or [4,4]) at the camera-to-world ``pose`` [4,4] of ``data.get_rays``, in fp64:
        (xy [V, 2] int32 in 1/256-pixel fixed point, zc [V] fp32 camera depth, NaN for a non-finite vertex), on the device."""
        v32 = self._rows3_arg(vertices, "project_vertices", "[V, 3] vertices")
        cam = (C.c_double * 17)(*camera_params(intrinsics, pose).tolist())
        V = int(v32.shape[0])
        xy, zc = self.empty(V, 2, dtype=torch.int32), self.empty(V)
        check(self.lib.es_rast_project(ptr(v32), V, cam, ptr(xy), ptr(zc), self.st()), "es_rast_project")
        return xy, zc

    def rasterize_projected(self, xy: torch.Tensor, zc: torch.Tensor, triangles: torch.Tensor, height: int, width: int, attributes=None,
                            near: float = 1e-6, cull: str = "none"):
        """Stage B of the rasteriser on the output of ``project_vertices`` (``meshing.rasterize_projected`` is the numpy twin and the
        specification): the dict of ``rasterize``.  The host reads the number of work items back between counting and filling, and
        the counts of ``stats`` at the end."""
        H, W = int(height), int(width)
        if not (1 <= H <= RAST_MAX_SIZE and 1 <= W <= RAST_MAX_SIZE):
            raise EndoSurfHipError(f"rasterize: height and width must be in 1..{RAST_MAX_SIZE} (got {height!r}, {width!r})")
        if cull not in RAST_CULL:
            raise EndoSurfHipError(f"rasterize: cull must be one of {sorted(RAST_CULL)} (got {cull!r})")
        if xy.dim() != 2 or xy.shape[1] != 2 or xy.dtype != torch.int32 or zc.dim() != 1 or zc.shape[0] != xy.shape[0] \
                or xy.device != self.device or zc.device != self.device:
            raise EndoSurfHipError(f"rasterize takes xy [V, 2] int32 and zc [V] on {self.device}")
        t32 = self._tri_arg(triangles, "rasterize")
        V, T = int(zc.shape[0]), int(t32.shape[0])
        att, Cn = self._attrs_arg(attributes, V, "rasterize")
        out = {"depth": None, "triangle": None, "bary": None, "attributes": None,
               "stats": dict({name: 0 for name in RAST_REASONS}, triangles=T, work_items=0, covered_pixels=0)}
        if V == 0 or T == 0:          # nothing to draw: no launch
            out.update(depth=torch.full((H, W), float("inf"), device=self.device), triangle=torch.full((H, W), -1, dtype=torch.int32, device=self.device),
                       bary=torch.zeros(H, W, 3, device=self.device), attributes=torch.zeros(H, W, Cn, device=self.device))
            out["stats"]["invalid"] = T
            return out
        xy32, zc32 = xy.contiguous(), f32(zc)
        scratch, totals, st = self._scratch("es_rast_scratch_bytes", V, T, H, W), self.empty(8, dtype=torch.int64), self.st()
        view = (H, W, float(near), RAST_CULL[cull], ptr(scratch))
        check(self.lib.es_rast_count(ptr(t32), V, T, ptr(xy32), ptr(zc32), *view, ptr(totals), st), "es_rast_count")
        n_work = int(totals[0].item())
        check(self.lib.es_rast_fill(ptr(t32), V, T, ptr(xy32), ptr(zc32), *view, n_work, st), "es_rast_fill")
        depth, tri, bary, attr = self.empty(H, W), self.empty(H, W, dtype=torch.int32), self.empty(H, W, 3), self.empty(H, W, Cn)
        check(self.lib.es_rast_resolve(ptr(t32), V, T, ptr(xy32), ptr(zc32), ptr(att), Cn, *view[:4], ptr(scratch), ptr(depth), ptr(tri), ptr(bary),
                                       ptr(attr) if Cn else None, ptr(totals), st), "es_rast_resolve")
        tt = totals.tolist()
        out["stats"].update({name: int(tt[1 + i]) for i, name in enumerate(RAST_REASONS)}, work_items=int(tt[0]), covered_pixels=int(tt[6]))
        out.update(depth=depth, triangle=tri, bary=bary, attributes=attr)
        return out

    def rasterize(self, vertices: torch.Tensor, triangles: torch.Tensor, intrinsics, pose, height: int, width: int, attributes=None,
                  near: float = 1e-6, cull: str = "none"):
        """A device mesh as images of a pinhole camera, without a display: ``depth`` [H, W] fp32 (camera z, the convention of
        ``data.depth_points``; +inf where nothing is hit), ``triangle`` [H, W] int32 (-1), ``bary`` [H, W, 3] (perspective-correct
        weights of the triangle's corners; 0), ``attributes`` [H, W, C] (the per-vertex ``attributes`` [V, C <= 8] interpolated with
        them; 0) and ``stats`` (triangles, rejected ones by reason -- invalid, near_rejected, zero_area, culled, offscreen --,
        work_items, covered_pixels).  Pixel (row i, column j) is sampled where ``data.get_rays`` casts its ray; one sample per pixel.
        A triangle with a corner not farther than ``near`` along the camera axis is dropped whole (no clipping); ``cull`` = "none",
        "back" or "front" (the front is the side the normal (v1 - v0) x (v2 - v0) points to: the outside of ``iso_surface``'s meshes).
        ``meshing.rasterize`` is the numpy twin; the rules of coverage and depth are in ``meshing.rasterize_projected``.  Equal depths
        go to the smaller triangle index, so the images are bit-identical from call to call."""
        xy, zc = self.project_vertices(vertices, intrinsics, pose)
        return self.rasterize_projected(xy, zc, triangles, height, width, attributes, near, cull)
