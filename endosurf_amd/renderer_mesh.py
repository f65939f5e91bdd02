"""The offline geometry methods of ``renderer.EndoSurfRenderer`` (a mixin): fields, meshes, their export, errors and pictures."""
from __future__ import annotations

import torch

from ._device import _on_device, f32
from .data import cal_geometric_error, cal_rmse, depth_points, write_ply
from .meshing import camera_params, iso_surface


class _Lattice:
    """The extraction lattice of (bound_min, bound_max, resolution) on ``device``: the bounds as fp32 [1,3] tensors ``bmin`` / ``bmax``
    and, each computed when asked for, the ``torch.linspace`` axes, the index -> world map and half a cell."""
    def __init__(self, bound_min, bound_max, resolution, device):
        self.lo, self.hi = (torch.as_tensor(b, dtype=torch.float32).cpu() for b in (bound_min, bound_max))
        self.resolution, self.device = resolution, device
        self.bmin, self.bmax = self.lo.to(device).reshape(1, 3), self.hi.to(device).reshape(1, 3)
    def axes(self):          # (the ends are the Python floats of the fp32 bounds)
        return [torch.linspace(float(self.lo[i]), float(self.hi[i]), int(self.resolution), device=self.device) for i in range(3)]
    def to_world(self, verts):          # index-space vertices [V,3], in their own precision (fp32 on the device)
        return verts / (self.resolution - 1.0) * (self.bmax - self.bmin) + self.bmin
    def half_cell(self):
        return 0.5 * (self.bmax - self.bmin) / (self.resolution - 1.0)


class RendererMeshMixin:
    def _field_on_device(self, bound_min, bound_max, resolution, t, net_chunk=1 << 22):
        """The SDF on a resolution^3 linspace grid at time ``t`` as a DEVICE tensor [R,R,R] (x-major): the grid coordinates are generated
        on the device and sampled by the fused query kernel in launches of ``net_chunk`` points."""
        R, ax = int(resolution), _Lattice(bound_min, bound_max, resolution, self.device).axes()
        tt = torch.as_tensor(t, dtype=torch.float32, device=self.device).reshape(-1)[:1]
        u = torch.empty(R * R * R, device=self.device)
        per_x = max(1, int(net_chunk) // (R * R))
        for i in range(0, R, per_x):
            xx, yy, zz = torch.meshgrid(ax[0][i:i + per_x], ax[1], ax[2], indexing="ij")
            pts = torch.stack([xx.reshape(-1), yy.reshape(-1), zz.reshape(-1)], -1)
            u[i * R * R:(i + per_x) * R * R] = self.sdf_observed(pts, tt).reshape(-1)
        return u.reshape(R, R, R)

    @_on_device
    def extract_fields(self, bound_min, bound_max, resolution, t, net_chunk=1 << 22):
        """SDF on a resolution^3 linspace grid at time ``t`` (reference extract_fields, utils.py:139-157, with the query of
        extract_observation_geometry): the grid coordinates are generated on the device, sampled by the fused query kernel in
        launches of ``net_chunk`` points and returned with ONE device-to-host copy as numpy [R,R,R] (x-major like the reference)."""
        return self._field_on_device(bound_min, bound_max, resolution, t, net_chunk).cpu().numpy()

    def _mesh_on_device(self, t, bound_min, bound_max, resolution, threshold, net_chunk, band=None, counts=None, method="tetrahedra"):
        """(vertices [V,3] in world coordinates, triangles [T,3] int32) as device tensors: field, iso-surface and the index -> world map
        all on the GPU (the field never leaves it; the host reads the two counts).  ``band``: True or a dict of block / lipschitz /
        max_fraction samples near the surface only, and ``Engine.band_field``'s counts go to ``counts["stats"]`` if ``counts`` is a dict.
        ``method``: ``Engine.iso_surface``'s triangulation, "tetrahedra" or "cubes"."""
        if method not in self.engine.ISO_METHODS:          # (before the field is sampled)
            raise ValueError(f"method must be one of {sorted(self.engine.ISO_METHODS)} (got {method!r})")
        if band is None or band is False:
            u = self._field_on_device(bound_min, bound_max, resolution, t, net_chunk)
        else:
            u, stats = self._band_field_on_device(bound_min, bound_max, resolution, t, threshold, net_chunk, {} if band is True else dict(band))
            if counts is not None:
                counts["stats"] = stats
        verts, tris, _ = self.engine.iso_surface(u, threshold, method)
        return _Lattice(bound_min, bound_max, resolution, self.device).to_world(verts), tris

    @staticmethod
    def _components_arg(components):
        """The ``components`` keyword as Engine.keep_components' arguments, or None: 0.9 / True (= 0.9) / dict(keep_ratio, compact)."""
        if components is None or components is False:
            return None
        components = 0.9 if components is True else components
        if isinstance(components, dict):
            unknown = set(components) - {"keep_ratio", "compact"}
            if unknown:
                raise TypeError(f"components takes keep_ratio and compact (got {sorted(unknown)})")
            return dict(keep_ratio=float(components.get("keep_ratio", 0.9)), compact=bool(components.get("compact", True)))
        return dict(keep_ratio=float(components), compact=True)

    def _band_field_on_device(self, bound_min, bound_max, resolution, t, threshold, net_chunk, band):
        """``_field_on_device`` with the SDF queried near the level set only (``Engine.band_field``): the same linspace axes, hence the
        same coordinates, and always the 64-point-tile query, whose per-point result does not depend on the batch -- the kernel the
        dense path runs for every launch above 16 384 points, so a band value is the dense value bit for bit.  (With
        ``engine.split_precision`` on, launches of ``engine.x3_query_min`` points or more go to the split-precision query as they do in
        ``query_sdf``; the bit-identity statement is made for the default fp32 path only.)"""
        unknown = set(band) - {"block", "lipschitz", "max_fraction"}
        if unknown:
            raise TypeError(f"band takes block, lipschitz and max_fraction (got {sorted(unknown)})")
        ax = _Lattice(bound_min, bound_max, resolution, self.device).axes()
        tt = torch.as_tensor(t, dtype=torch.float32, device=self.device).reshape(-1)[:1]
        weff, packed = self._weights()
        weff = weff.detach()

        def sample(x):
            with torch.no_grad():
                return self.engine.query_sdf(self.engine.points(x=x, t=tt), weff, packed, self.use_deform, tile_points=64)

        u, stats, _ = self.engine.band_field(sample, ax, threshold, net_chunk=net_chunk, **band)
        return u, stats

    @_on_device
    def extract_observation_geometry(self, t, bound_min, bound_max, resolution, threshold=0.0, net_chunk=1 << 22, cpu=True, on_device=False,
                                     band=None, components=None, method="tetrahedra"):
        """(vertices, triangles) of the observed-space surface at time t (reference endosurf.py:490-500 + extract_geometry,
        utils.py:128-136).  Field sampling runs on the GPU.  By default the field is copied to the host and the iso-surface extractor
        is PyMCubes when installed (as in the reference), otherwise endosurf_amd.meshing.marching_tetrahedra (different triangulation
        of the same level set).  ``on_device=True`` extracts on the GPU as well (``Engine.iso_surface``: marching_tetrahedra's
        triangulation, fp32 vertices, int32 triangles) and returns numpy arrays when ``cpu`` else device tensors.  With ``on_device``,
        ``band=True`` or ``band=dict(block=8, lipschitz=1.0, max_fraction=0.5)`` queries the SDF near the surface only (see
        ``extract_observation_mesh``); the default ``None`` samples every grid point.  With ``on_device``, ``components=0.9`` (or True,
        or dict(keep_ratio=0.9, compact=True)) keeps the largest connected components only (``Engine.keep_components``; see
        ``extract_observation_mesh``); the default ``None`` keeps every triangle.  With ``on_device``, ``method="cubes"`` triangulates
        with this project's cube table (``meshing.marching_cubes``, csrc/cubes.hip: a third of the vertices and triangles; not
        PyMCubes' table) instead of the default "tetrahedra"."""
        comp = self._components_arg(components)
        if method != "tetrahedra" and not on_device:
            raise ValueError("method needs on_device=True (the host path is meshing.iso_surface: PyMCubes, else marching tetrahedra)")
        if band is not None and band is not False and not on_device:
            raise ValueError("band needs on_device=True (the narrow-band field is assembled on the GPU)")
        if comp is not None and not on_device:
            raise ValueError("components needs on_device=True (the component filter runs on the GPU)")
        if on_device:
            vertices, triangles = self._mesh_on_device(t, bound_min, bound_max, resolution, threshold, net_chunk, band, method=method)
            if comp is not None:
                vertices, triangles, _, _ = self.engine.keep_components(vertices, triangles, **comp)
            return (vertices.cpu().numpy(), triangles.cpu().numpy()) if cpu else (vertices, triangles)
        u = self.extract_fields(bound_min, bound_max, resolution, t, net_chunk)
        vertices, triangles = iso_surface(u, threshold)
        b_max = torch.as_tensor(bound_max, dtype=torch.float32).cpu().numpy()
        b_min = torch.as_tensor(bound_min, dtype=torch.float32).cpu().numpy()
        vertices = vertices / (resolution - 1.0) * (b_max - b_min)[None, :] + b_min[None, :]
        return vertices, triangles

    @_on_device
    def extract_observation_mesh(self, t, bound_min, bound_max, resolution, threshold=0.0, net_chunk=1 << 22, view_point=None, refine_steps=0,
                                 band=None, components=None, clean=False, simplify=None, method="tetrahedra"):
        """The observed-space surface at time t as a coloured mesh, device tensors only (what the reference's demo assembles from
        extract_observation_geometry + renderonpts, trainer_endosurf.py:403-460): ``vertices`` [V,3] world coordinates, ``triangles``
        [T,3] int32, ``normals`` [V,3] the analytic observed-space SDF gradient at the vertices normalised as renderonpts does, ``sdf``
        [V] the SDF at the vertices, and with a ``view_point`` [3] ``colors`` [V,3] = renderonpts(vertices, normalize(vertices -
        view_point), t).  ``refine_steps`` Newton steps v -= (sdf - threshold) g / |g|^2, each clamped to half a grid cell, pull the
        vertices onto the level set before the attributes are taken (linear interpolation leaves an O(h^2) residual).  ``net_chunk``
        bounds the grid points per query launch; the vertices are evaluated min(net_chunk, 131072) at a time (a point evaluation keeps
        ~10 KB of workspace per point, a query none).

        ``band=True`` or ``band=dict(block=8, lipschitz=1.0, max_fraction=0.5)`` queries the SDF only in blocks of ``block`` grid cells
        near the surface (``Engine.band_field``, csrc/band.hip) instead of at all resolution^3 points, and adds ``stats`` (a dict of
        counts: dense_points, evaluated_points, blocks, seed_blocks, active_blocks, rounds, fallback) to the result.  A block is
        examined when its corners change sign or none of them is farther than ``lipschitz`` * (block diagonal) from the level -- the
        SDF is trained towards |grad| = 1 --, and blocks next to an examined one are added as long as the surface is seen to cross their
        shared face.  Every connected piece of the dense mesh that passes through an examined block comes out complete and
        bit-identical, in the dense vertex and triangle order: the whole mesh when |grad sdf| <= lipschitz holds in the culled blocks.
        What a too small ``lipschitz`` can lose is a closed floater smaller than a block that no block corner sees.  Bit-identity is
        stated for the default fp32 query; with ``engine.split_precision`` the band follows ``query_sdf``'s choice of kernel per launch.
        The default ``None`` is the dense path.

        ``components=0.9``, ``True`` (= 0.9) or ``dict(keep_ratio=0.9, compact=True)`` removes, right after the iso-surface and before
        refinement, normals and colours (so the point evaluations run on the kept vertices only), every triangle whose connected
        component has fewer than ``keep_ratio`` x the triangles of the largest one -- the reference demo's floater filter
        (trainer_endosurf.py:440-445), by ``Engine.keep_components`` (csrc/mesh.hip): components by shared vertices, degenerate
        triangles dropped, order kept; ``compact=False`` keeps the orphaned vertices as the reference does.  Adds ``components`` (a dict
        of counts: components, max_triangles, kept_triangles, degenerate, rounds) to the result.  The filter removes exactly what a
        too small band ``lipschitz`` can lose, so band and dense agree behind it.  The default ``None`` keeps every triangle.

        ``clean=True`` removes, after the component filter, every triangle with a repeated index and every duplicate of an earlier
        triangle (``Engine.mesh_clean``; unreferenced vertices go as well) and adds ``clean`` (a dict of counts: degenerate, duplicates,
        kept_triangles).  ``simplify=c`` (a cell size in scene units, cells counted from the origin) or ``simplify="grid"`` (one cell of
        the extraction lattice, counted from ``bound_min``) then merges the vertices of each cell into their mean
        (``Engine.cluster_vertices``, which cleans behind itself) before refinement, normals and colours, which are therefore evaluated
        at the clustered vertices, not averaged; it adds ``simplify`` (cells, largest_cell, degenerate, duplicates, kept_triangles).
        Both are off by default, and the mesh is then bit for bit what it was without these keywords.

        ``method="cubes"`` extracts with this project's cube triangulation (``Engine.iso_surface(method="cubes")``,
        ``meshing.marching_cubes``) instead of the default "tetrahedra": the vertices on the lattice's axis edges only, about a third
        of the vertices and triangles, so every later step -- filter, clean-up, clustering, refinement, normals, colours, export --
        handles a third of the elements.  The result then carries ``method``.  Band and dense agree as they do by default."""
        comp = self._components_arg(components)
        counts = {}          # the dicts of counts the result carries, by its key
        vertices, triangles = self._mesh_on_device(t, bound_min, bound_max, resolution, threshold, net_chunk, band, counts, method)
        if method != "tetrahedra":
            counts["method"] = method
        if comp is not None:
            vertices, triangles, _, counts["components"] = self.engine.keep_components(vertices, triangles, **comp)
        if clean:
            vertices, triangles, _, counts["clean"] = self.engine.mesh_clean(vertices, triangles, compact=True)
        if simplify is not None and simplify is not False:
            cell, origin = self._simplify_arg(simplify, bound_min, bound_max, resolution)
            vertices, triangles, _, _, counts["simplify"] = self.engine.cluster_vertices(vertices, triangles, cell, origin)
        tt = torch.as_tensor(t, dtype=torch.float32, device=self.device).reshape(-1)[:1]
        chunk = max(1, min(int(net_chunk), 1 << 17))

        def sdf_grad(v):
            with torch.no_grad():
                out = [self._point_eval(v[i:i + chunk], tt) for i in range(0, v.shape[0], chunk)]
            return torch.cat([o[0] for o in out], 0).reshape(-1, 1), torch.cat([o[1] for o in out], 0)

        out = {"vertices": vertices, "triangles": triangles, **counts}
        if vertices.shape[0] == 0:
            out.update(normals=vertices.clone(), sdf=vertices.new_zeros(0))
            if view_point is not None:
                out["colors"] = vertices.clone()
            return out
        half_cell = _Lattice(bound_min, bound_max, resolution, self.device).half_cell()
        for _ in range(int(refine_steps)):
            s, g = sdf_grad(vertices)
            step = (s - threshold) * g / (g * g).sum(-1, keepdim=True).clamp_min(1e-20)
            vertices = vertices - torch.maximum(torch.minimum(step, half_cell), -half_cell)
        out["vertices"] = vertices
        if view_point is None:
            s, g = sdf_grad(vertices)
            out["normals"] = g / (torch.linalg.norm(g, ord=2, dim=-1, keepdim=True) + 1e-10)
        else:
            vp = torch.as_tensor(view_point, dtype=torch.float32).to(self.device).reshape(1, 3)
            dirs = vertices - vp
            dirs = dirs / torch.linalg.norm(dirs, ord=2, dim=-1, keepdim=True)
            out["colors"], out["normals"] = self.renderonpts(vertices, dirs, tt, net_chunk=chunk, cpu=False)
            s, _ = sdf_grad(vertices)
        out["sdf"] = s.reshape(-1)
        return out

    @staticmethod
    def _simplify_arg(simplify, bound_min, bound_max, resolution):
        """The ``simplify`` keyword as (cell, origin) of Engine.cluster_vertices: a cell size in scene units counted from the origin, or
        "grid": the largest spacing of the extraction lattice, counted from ``bound_min``."""
        if isinstance(simplify, str):
            if simplify != "grid":
                raise ValueError(f'simplify takes a cell size or "grid" (got {simplify!r})')
            bmin = torch.as_tensor(bound_min, dtype=torch.float32).cpu().double().reshape(3)
            bmax = torch.as_tensor(bound_max, dtype=torch.float32).cpu().double().reshape(3)
            return float(((bmax - bmin) / (float(resolution) - 1.0)).max()), tuple(float(b) for b in bmin)
        cell = float(simplify)
        if not cell > 0.0:
            raise ValueError(f"simplify: the cell size must be positive (got {simplify!r})")
        return cell, (0.0, 0.0, 0.0)

    @_on_device
    def export_observation_mesh(self, prefix, t, bound_min, bound_max, resolution, threshold=0.0, view_point=None, components=0.9, simplify=None,
                                method="tetrahedra", **extract_kwargs):
        """The three mesh files of the reference's demo for one frame (trainer_endosurf.py:435-466), without Open3D:
        ``prefix + "_geometry.ply"`` (vertices and triangles), ``prefix + "_color.ply"`` (plus the ``renderonpts`` colours clipped to
        [0, 1]; white without a ``view_point``, as there is no direction to render from) and ``prefix + "_normal.ply"`` (plus the
        paint (-n 0.5 + 0.5).clip(0, 1) of the normals ``Engine.vertex_normals`` computes from the triangles, the demo's
        compute_vertex_normals).  The mesh is that of ``extract_observation_mesh`` with the component filter (``components``, 0.9 as in
        the demo; None for none), always cleaned of degenerate and duplicate triangles, clustered when ``simplify`` is given, and
        triangulated by ``method`` ("tetrahedra", or "cubes" for files a third of the size);
        ``extract_kwargs`` (net_chunk, refine_steps, band) are passed on.  Files are ``data.write_ply``'s: binary little endian, fp32
        coordinates, the body packed on the device, one copy to the host per file.  Returns the mesh dict with ``vertex_normals``
        [V, 3] and ``paths`` (geometry, color, normal)."""
        unknown = set(extract_kwargs) - {"net_chunk", "refine_steps", "band"}
        if unknown:
            raise TypeError(f"export_observation_mesh passes net_chunk, refine_steps and band on (got {sorted(unknown)})")
        mesh = self.extract_observation_mesh(t, bound_min, bound_max, resolution, threshold=threshold, view_point=view_point, components=components,
                                             clean=True, simplify=simplify, method=method, **extract_kwargs)
        v, f = mesh["vertices"], mesh["triangles"]
        vn = self.engine.vertex_normals(v, f)
        colors = mesh["colors"].clamp(0.0, 1.0) if "colors" in mesh else torch.ones_like(v)
        prefix = str(prefix)
        paths = {k: f"{prefix}_{k}.ply" for k in ("geometry", "color", "normal")}
        write_ply(paths["geometry"], v, f, engine=self.engine)
        write_ply(paths["color"], v, f, colors=colors, engine=self.engine)
        write_ply(paths["normal"], v, f, colors=(-vn * 0.5 + 0.5).clamp(0.0, 1.0), engine=self.engine)
        mesh.update(vertex_normals=vn, paths=paths)
        return mesh

    @_on_device
    def geometric_error(self, mesh_or_vertices, depth, intrinsics, pose, depth_trunc, depth_scale=1.0) -> float:
        """The reference demo's 3D number for one frame (trainer_endosurf.py:418 / geo_errs): the ground-truth depth frame
        back-projected into a point cloud (``data.depth_points``: depth [H,W] z-depths, intrinsics, camera-to-world pose, pixels with
        0 < depth <= depth_trunc), and the mean distance from its points to the nearest mesh vertex times ``depth_scale``
        (``Engine.nearest``: exact, on the device).  ``mesh_or_vertices``: the dict of ``extract_observation_mesh`` or [V,3] vertices."""
        verts = mesh_or_vertices["vertices"] if isinstance(mesh_or_vertices, dict) else mesh_or_vertices
        verts = torch.as_tensor(verts, dtype=torch.float32).to(self.device)
        pts = depth_points(torch.as_tensor(depth, dtype=torch.float32).to(self.device), intrinsics, pose, depth_trunc)
        return cal_geometric_error(pts, verts, depth_scale, engine=self.engine)

    def _mesh_arg(self, mesh):
        """(vertices [V,3] fp32, triangles [T,3], the dict or None) of a mesh given as ``extract_observation_mesh``'s dict or as
        (vertices, triangles), on the renderer's device."""
        d = mesh if isinstance(mesh, dict) else None
        v, f = (mesh["vertices"], mesh["triangles"]) if d is not None else mesh
        v = torch.as_tensor(v, dtype=torch.float32).to(self.device)
        f = torch.as_tensor(f).to(self.device)
        return v, (f if f.dtype in (torch.int32, torch.int64) else f.to(torch.int64)), d

    @_on_device
    def surface_error(self, mesh, depth, intrinsics, pose, depth_trunc, depth_scale=1.0, thresholds=()) -> dict:
        """``geometric_error`` measured to the mesh's surface instead of its vertices, so that the number does not change with the
        resolution or the simplification of the same surface: the ground-truth cloud of ``data.depth_points`` (as there), and for each
        of its points the exact distance to the closest triangle (``Engine.point_to_mesh``, on the device) times ``depth_scale``.
        ``mesh``: the dict of ``extract_observation_mesh`` or (vertices, triangles).  Returns dict(``mean`` (= ``data.cal_surface_error``),
        ``rmse``, ``max``, ``vertex_mean`` (exactly ``geometric_error``'s value, for comparison), ``within``: for each tau of
        ``thresholds`` the fraction of points with distance <= tau, ``points``).  Reductions in fp64, one small copy to the host.  nan
        for an empty cloud, inf for a mesh without a valid triangle."""
        v, f, _ = self._mesh_arg(mesh)
        taus, scale = [float(t) for t in thresholds], float(depth_scale)
        pts = depth_points(torch.as_tensor(depth, dtype=torch.float32).to(self.device), intrinsics, pose, depth_trunc)
        out = {"vertex_mean": cal_geometric_error(pts, v, depth_scale, engine=self.engine), "points": int(pts.shape[0])}
        if pts.shape[0] == 0:
            out.update(mean=float("nan"), rmse=float("nan"), max=float("nan"), within=[float("nan")] * len(taus))
            return out
        d = self.engine.point_to_mesh(pts, v, f)[0].double()
        ds = d * scale
        # (mean: the expression of cal_surface_error, so that the two agree to the last bit)
        red = torch.stack([d.mean(), (ds * ds).mean().sqrt(), ds.max()] + [(ds <= t).double().mean() for t in taus]).tolist()
        out.update(mean=red[0] * scale, rmse=red[1], max=red[2], within=red[3:])
        return out

    @_on_device
    def render_mesh(self, mesh, intrinsics, pose, height, width, view_point=None, cull="none"):
        """The three pictures the reference's demo takes of an extracted mesh (vis_mesh through Open3D's Visualizer, the
        "Mesh / Texture / Normal" panels), from the pinhole camera ``intrinsics`` / camera-to-world ``pose`` of ``data.get_rays``,
        without a display: ``Engine.rasterize`` (csrc/raster.hip) once, shaded three times.  ``mesh``: the dict of
        ``extract_observation_mesh`` or (vertices, triangles).  Returns float images in [0, 1], [H,W,3], background 1.0:
        ``color`` (the vertex colours interpolated and clipped; grey 0.7 for a mesh without ``colors``), ``normal`` ((-n 0.5 + 0.5).clip(0, 1) of the
        interpolated, re-normalised vertex normals: the demo's paint), ``geometry`` (grey head-light shading |n . v|, v the unit direction
        from the surface point to the camera); and ``depth`` [H,W] (camera z, +inf on the background), ``mask`` [H,W] bool,
        ``triangle`` [H,W] int32, ``stats``.  Normals are the mesh's ``normals`` when present, else area-weighted triangle normals.
        ``view_point`` [3] replaces the camera position as the eye of the head light."""
        v, f, d = self._mesh_arg(mesh)
        H, W = int(height), int(width)
        cam = camera_params(intrinsics, pose)
        normals = d.get("normals") if d is not None else None
        if normals is None:
            f64 = f.long()
            fn = torch.linalg.cross(v[f64[:, 1]] - v[f64[:, 0]], v[f64[:, 2]] - v[f64[:, 0]]) if f.shape[0] else v.new_zeros(0, 3)
            normals = torch.zeros_like(v)
            for k in range(3):
                normals.index_add_(0, f64[:, k], fn)
            normals = normals / torch.linalg.norm(normals, dim=-1, keepdim=True).clamp_min(1e-30)
        colors = d.get("colors") if d is not None else None
        if colors is None:
            colors = torch.full_like(v, 0.7)
        attrs = torch.cat([f32(colors).to(self.device), f32(normals).to(self.device)], -1)
        ras = self.engine.rasterize(v, f, intrinsics, pose, H, W, attributes=attrs, cull=cull)
        hit = ras["triangle"] >= 0
        m3 = hit[..., None]
        one = torch.ones(H, W, 3, device=self.device)
        n = ras["attributes"][..., 3:6]
        n = n / torch.linalg.norm(n, dim=-1, keepdim=True).clamp_min(1e-30)
        # the surface point of a pixel: its ray K^-1 [j, i, 1] at the camera depth, rotated to the world
        R = torch.tensor(cam[:9].reshape(3, 3), dtype=torch.float32, device=self.device)
        tr = torch.tensor(cam[9:12], dtype=torch.float32, device=self.device)
        k00, k01, k02, k11, k12 = (float(c) for c in cam[12:17])
        ii, jj = torch.meshgrid(torch.arange(H, device=self.device, dtype=torch.float32), torch.arange(W, device=self.device, dtype=torch.float32),
                                indexing="ij")
        yc = (ii - k12) / k11
        xc = (jj - k02 - k01 * yc) / k00
        z = torch.where(hit, ras["depth"], torch.zeros_like(ras["depth"]))
        pw = (torch.stack([xc, yc, torch.ones_like(xc)], -1) * z[..., None]) @ R.T + tr
        eye = tr if view_point is None else torch.as_tensor(view_point, dtype=torch.float32).to(self.device).reshape(3)
        to_eye = eye - pw
        to_eye = to_eye / torch.linalg.norm(to_eye, dim=-1, keepdim=True).clamp_min(1e-30)
        shade = (n * to_eye).sum(-1, keepdim=True).abs().clamp(0.0, 1.0).expand(H, W, 3)
        return {"color": torch.where(m3, ras["attributes"][..., 0:3].clamp(0.0, 1.0), one),
                "normal": torch.where(m3, (-n * 0.5 + 0.5).clamp(0.0, 1.0), one), "geometry": torch.where(m3, shade, one),
                "depth": ras["depth"], "mask": hit, "triangle": ras["triangle"], "stats": ras["stats"]}

    @_on_device
    def mesh_depth_error(self, mesh, depth, mask, intrinsics, pose, depth_scale=1.0):
        """The 2D counterpart of ``geometric_error``: the mesh rasterised from the camera ``intrinsics`` / ``pose`` of a depth frame
        (``Engine.rasterize``: camera z per pixel), against that frame.  ``depth`` [H,W] (or [H,W,1]) z-depths, ``mask`` likewise (non-zero =
        the pixel counts).  Returns dict(``rmse`` = ``data.cal_rmse`` over the masked pixels the mesh covers, times ``depth_scale`` (nan
        when there is none), ``coverage`` = the fraction of masked pixels the mesh covers)."""
        v, f, _ = self._mesh_arg(mesh)
        d = torch.as_tensor(depth, dtype=torch.float32).to(self.device)
        m = torch.as_tensor(mask).to(self.device)
        d = d[..., 0] if d.dim() == 3 and d.shape[-1] == 1 else d
        m = (m[..., 0] if m.dim() == 3 and m.shape[-1] == 1 else m) != 0
        if d.dim() != 2 or m.shape != d.shape:
            raise ValueError(f"depth and mask must be [H, W] or [H, W, 1] (got {tuple(d.shape)}, {tuple(m.shape)})")
        ras = self.engine.rasterize(v, f, intrinsics, pose, d.shape[0], d.shape[1])
        both = m & (ras["triangle"] >= 0)
        n_mask, n_both = int(m.sum()), int(both.sum())
        mesh_depth = torch.where(both, ras["depth"], torch.zeros_like(d))
        rmse = cal_rmse(mesh_depth, torch.where(both, d, torch.zeros_like(d)), both.to(torch.float32)) * float(depth_scale) if n_both else float("nan")
        return {"rmse": rmse, "coverage": n_both / n_mask if n_mask else float("nan")}
