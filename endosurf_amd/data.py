"""Dataset-side callers of the hot path: what the reference's ``Dataset`` (src/dataset/dataset.py) does
between decoded images and the renderer — pinhole ray generation, the [n,h,w,9] ray tensor contract, the mask-guided
inverse-CDF pixel sampler and the per-iteration batch gather — as device-side torch code without host synchronisation.
File decoding (imageio / cv2 / pickle info files) is out of scope: a ``FrameSet`` is built from arrays already in memory."""
from __future__ import annotations

import contextlib
from typing import Dict, Optional, Sequence

import numpy as np
import torch


def get_rays(intrinsics: torch.Tensor, poses: torch.Tensor, w: int, h: int) -> torch.Tensor:
    """Dataset.get_rays (dataset.py:216-235): per frame d = normalize(K^-1 [x, y, 1]) rotated to world, o = pose translation.
    intrinsics, poses: [n,4,4] -> rays [n,h,w,6] (origin, unit direction)."""
    dev, dt = intrinsics.device, intrinsics.dtype
    k_inv = torch.inverse(intrinsics)[:, :3, :3]
    ys, xs = torch.meshgrid(torch.linspace(0, h - 1, h, device=dev, dtype=dt), torch.linspace(0, w - 1, w, device=dev, dtype=dt),
                            indexing="ij")
    p = torch.stack([xs, ys, torch.ones_like(xs)], -1)                               # [h,w,3]
    d = torch.einsum("nij,hwj->nhwi", k_inv, p)
    d = d / torch.linalg.norm(d, ord=2, dim=-1, keepdim=True)
    d = torch.einsum("nij,nhwj->nhwi", poses[:, :3, :3], d)
    o = poses[:, None, None, :3, 3].expand_as(d)
    return torch.cat([o, d], -1)


def assemble_rays(rays6: torch.Tensor, bounds: torch.Tensor, normalize_time: bool = True) -> torch.Tensor:
    """[n,h,w,9] = rays6 | per-frame (near, far) bounds | per-frame time (dataset.py:86-96); time = linspace(0,1,n) or the index."""
    n, h, w, _ = rays6.shape
    ts = torch.linspace(0.0, 1.0, n, device=rays6.device) if normalize_time else torch.arange(n, device=rays6.device, dtype=rays6.dtype)
    return torch.cat([rays6, bounds[:, None, None, :].expand(n, h, w, 2).to(rays6.dtype),
                      ts[:, None, None, None].expand(n, h, w, 1).to(rays6.dtype)], -1)


def ray_sampling_importance_from_masks(masks: torch.Tensor) -> torch.Tensor:
    """Dataset._ray_sampling_importance_from_masks (dataset.py:262-267).  masks [n,h,w,1] -> importance [n,h,w,1]:
    a visible pixel weighs 1 + (how often that pixel is masked out over the sequence, L2-normalised over the image)."""
    hidden = masks.shape[0] - masks.sum(dim=0)                 # per pixel: number of frames that mask it out
    return masks * (1.0 + hidden / torch.linalg.vector_norm(hidden))


def sampling_cdf(weights: torch.Tensor, floor: float = 1e-5) -> torch.Tensor:
    """Normalised running sum of ``weights + floor`` along the last axis: the table the inverse-CDF draw searches."""
    w = weights + floor
    return torch.cumsum(w / w.sum(dim=-1, keepdim=True), dim=-1)


def importance_sampling_coords(weights: torch.Tensor, n_samples: int, det: bool = False, u: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Dataset._importance_sampling_coords (dataset.py:237-260): ``n_samples`` indices per row of ``weights`` drawn by inverting
    the CDF of (weights + 1e-5) with searchsorted(right=True).  ``det``: evenly spaced quantiles; ``u``: caller-supplied uniform
    draws (reproducible tests); otherwise torch.rand on the weights' device."""
    cdf = sampling_cdf(weights)
    rows = tuple(cdf.shape[:-1])
    if det:
        u = torch.linspace(0.0, 1.0, n_samples, device=cdf.device).expand(*rows, n_samples)
    elif u is None:
        u = torch.rand(*rows, n_samples, device=cdf.device)
    return torch.searchsorted(cdf, u.contiguous(), right=True)


class FrameSet:
    """In-memory stand-in for the reference Dataset's tensors: colors [n,h,w,3], depths [n,h,w,1] (already scaled), masks.
    ``get_train_batch_data_by_index`` mirrors dataset.py:117-161 (one frame per iteration, pixels outside the colour mask are
    never drawn, mask-guided importance sampling by default) and stays on the device."""

    def __init__(self, colors, depths, intrinsics, poses, bounds, color_masks=None, depth_masks=None, near=None, far=None,
                 normalize_time: bool = True, list_train: Optional[Sequence[int]] = None, device="cuda"):
        dev = torch.device(device)
        T = lambda a: torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a, dtype=torch.float32).to(dev)
        self.device = dev
        self.colors, self.depths = T(colors), T(depths)
        self.n_frames, self.h, self.w = self.colors.shape[:3]
        if depth_masks is None:       # dataset.py:75-77: depths inside the [3 %, 99.5 %] percentile range are trusted
            d = self.depths.detach().cpu().numpy()
            self.near = float(np.percentile(d, 3.0)) if near is None else near
            self.far = float(np.percentile(d, 99.5)) if far is None else far
            depth_masks = ((self.depths > self.near) & (self.depths < self.far)).to(torch.float32)
        self.depth_masks = T(depth_masks)
        self.color_masks = T(color_masks) if color_masks is not None else torch.ones_like(self.depth_masks)
        self.masks = self.depth_masks * self.color_masks
        self.intrinsics, self.poses = T(intrinsics), T(poses)
        self.rays = assemble_rays(get_rays(self.intrinsics, self.poses, self.w, self.h), T(bounds), normalize_time)
        self.ray_importance_maps = ray_sampling_importance_from_masks(self.masks)
        self.list_train = list(range(self.n_frames)) if list_train is None else list(list_train)
        self._host_rng = np.random.default_rng(0)
        # per-frame sampling tables (the CDF over the colour-masked pixels, the index of the last kept pixel, the kept-pixel lists of
        # the uniform branch) are built lazily, one frame at a time, the first time a frame is drawn: no [n_frames, H*W] temporaries
        # at construction and no host round trip per batch afterwards
        self._tables = {}
        self._kept = {}

    _OWN_ARGS = ("depth_masks", "near", "far", "normalize_time", "list_train", "device")

    @classmethod
    def from_raw(cls, colors, depths, intrinsics, poses, bounds, color_masks=None, **normalization_args):
        """The ``FrameSet`` of a raw RGB-D sequence: metric depths [n,h,w] or [n,h,w,1], camera-to-world ``poses`` and ``bounds`` in
        the depths' unit.  What the reference splits between data/*/preprocess.py and Dataset.__init__: ``scene_normalization`` of the
        depths (masked by ``color_masks``), ``normalize_cameras``, depths and bounds divided by the scene radius.  The normalisation
        runs on the frame set's ``device``; keywords that are not ``FrameSet``'s own (``_OWN_ARGS``) go to ``scene_normalization``.
        ``scale_mat`` [4,4] fp32, ``depth_scale`` (float) and ``bbox_minmax`` [n,3,2] fp64 are kept as attributes, named as on the
        reference's Dataset."""
        own = {k: normalization_args.pop(k) for k in cls._OWN_ARGS if k in normalization_args}
        dev = torch.device(own.get("device", "cuda"))
        T = lambda a: None if a is None else torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a, dtype=torch.float32).to(dev)
        d, k, c2w, cm = T(depths), T(intrinsics), T(poses), T(color_masks)
        d = d[..., 0] if d.dim() == 4 else d
        normalization_args.setdefault("masks", cm)
        norm = scene_normalization(d, k, c2w, **normalization_args)
        k_n, c2w_n = normalize_cameras(k, c2w, norm["scale_mat"])
        scale = norm["depth_norm_scale"]
        cm = cm[..., None] if cm is not None and cm.dim() == 3 else cm
        fs = cls(colors, d[..., None] / scale, k_n, c2w_n, T(bounds) / scale, color_masks=cm, **own)
        fs.scale_mat, fs.depth_scale, fs.bbox_minmax = norm["scale_mat"], scale, norm["bbox_minmax"]
        return fs

    _STEREO_ARGS = ("max_disparity", "near", "far", "close", "engine", "poll")

    @classmethod
    def from_stereo(cls, colors_left, colors_right, intrinsics, poses, baseline, bounds=None, **args):
        """The ``FrameSet`` of a rectified stereo sequence: ``colors_left`` / ``colors_right`` [n,h,w,3] (uint8, or float in [0,1]),
        ``intrinsics`` and camera-to-world ``poses`` [n,4,4] of the left camera, ``baseline`` in the unit the depths shall have.
        ``stereo_depth`` runs per frame with the focal length ``intrinsics[i,0,0]`` (on the device for device tensors, through the numpy
        twin for host arrays); then ``from_raw`` with the left colours (uint8 colours divided by 255), these depths, ``color_masks`` =
        the closed masks and ``depth_masks`` = depth > 0 unless the caller passes its own.  ``bounds`` [n,2] default to the smallest and
        largest non-zero depth of each frame; a frame without a valid pixel raises ValueError.  Keywords: ``max_disparity`` (required),
        ``near``, ``far``, ``close``, ``engine``, ``poll`` and the matcher's (``stereo.MATCHER_ARGS``) go to ``stereo_depth``, the rest
        to ``from_raw``.  ``scale_mat``, ``depth_scale`` and ``bbox_minmax`` are attributes as after ``from_raw``."""
        from .stereo import MATCHER_ARGS
        matcher = {k: args.pop(k) for k in cls._STEREO_ARGS + MATCHER_ARGS if k in args}
        if "max_disparity" not in matcher:
            raise TypeError("from_stereo needs max_disparity")
        n = int(colors_left.shape[0])
        focal = torch.as_tensor(np.asarray(intrinsics) if not torch.is_tensor(intrinsics) else intrinsics)[:, 0, 0].double().cpu().tolist()
        depths, closed, found = [], [], []
        for i in range(n):
            r = stereo_depth(colors_left[i], colors_right[i], focal[i], baseline, **matcher)
            d = r["depth"]
            if not bool(r["depth_mask"].any()):
                raise ValueError(f"from_stereo: frame {i} has no valid pixel")
            seen = d[r["depth_mask"]]
            found.append(torch.stack([seen.min(), seen.max()]))
            depths.append(d)
            closed.append(r["color_mask"])
        depths, closed = torch.stack(depths), torch.stack(closed).to(torch.float32)
        bounds = torch.stack(found) if bounds is None else bounds
        args.setdefault("depth_masks", (depths > 0).to(torch.float32)[..., None])
        colors = colors_left if torch.is_tensor(colors_left) else torch.as_tensor(np.asarray(colors_left))
        if colors.dtype == torch.uint8:          # k / 255 from one table made on the host: the same fp32 values wherever the colours live
            colors = torch.from_numpy((np.arange(256) / 255.0).astype(np.float32)).to(colors.device)[colors.long()]
        return cls.from_raw(colors, depths, intrinsics, poses, bounds, color_masks=closed, **args)

    def _frame_tables(self, i: int):
        """(cdf [H*W] fp32, last kept pixel [] int64, colour-mask [H*W] bool) of frame ``i``; raises if its colour mask is empty
        (the reference's compaction would fail there as well, dataset.py:131-137)."""
        t = self._tables.get(i)
        if t is None:
            cm = self.color_masks[i, ..., 0].reshape(-1) == 1.0
            imp = self.ray_importance_maps[i, ..., 0].reshape(-1)
            # sampling over the colour-masked pixels only == sampling over all pixels with the others' weight removed; a zero weight
            # (instead of the reference's compaction) keeps shapes static.  The 1e-5 floor is applied to kept pixels only
            wts = torch.where(cm, imp + 1e-5, torch.zeros_like(imp))
            total = wts.sum()
            if not bool(total > 0):
                raise ValueError(f"frame {i}: the colour mask is empty, there is no pixel to sample")
            idx = torch.arange(cm.shape[0], device=self.device, dtype=torch.int32)
            last = torch.where(cm, idx, torch.zeros_like(idx)).amax().to(torch.int64)
            t = self._tables[i] = (torch.cumsum(wts / total, -1), last, cm)
        return t

    def get_train_batch_data_by_index(self, id_train=None, ray_batch=1024, mask_guided_ray_sampling=True, u=None) -> Dict[str, torch.Tensor]:
        if id_train is None:
            id_train = int(self._host_rng.choice(self.list_train))
        else:
            assert id_train in self.list_train, f"ID {id_train} is not in training list!"
        if mask_guided_ray_sampling:
            if u is None:
                u = torch.rand(ray_batch, device=self.device)
            cdf, last_kept, _ = self._frame_tables(id_train)
            sel = torch.searchsorted(cdf, u.reshape(-1).to(self.device).contiguous(), right=True)
            # clamp like the reference (max with 0, min with last kept pixel): u -> 1 rounds to the last colour-masked pixel
            sel = torch.minimum(sel, last_kept)
        else:
            kept = self._kept.get(id_train)
            if kept is None:
                kept = self._kept[id_train] = torch.nonzero(self._frame_tables(id_train)[2]).reshape(-1)      # once per frame
            sel = kept[torch.randperm(kept.numel(), device=self.device)[:ray_batch]]
        pick = lambda a: a[id_train].reshape(self.h * self.w, -1)[sel]
        return {"color": pick(self.colors), "rays": pick(self.rays), "depth": pick(self.depths), "mask": pick(self.masks),
                "color_mask": pick(self.color_masks), "depth_mask": pick(self.depth_masks)}

    def get_frame_data_by_index(self, idx):
        """dataset.py:163-181: whole frames (for evaluation / render_frames)."""
        return {"color": self.colors[idx], "rays": self.rays[idx], "depth": self.depths[idx], "mask": self.masks[idx],
                "color_mask": self.color_masks[idx], "depth_mask": self.depth_masks[idx]}


def cal_psnr(a, b, mask) -> float:
    """src/trainer/utils.py:340-354."""
    a, b, mask = (x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x) for x in (a, b, mask))
    if mask.ndim == a.ndim - 1:
        mask = mask[..., None]
    return float(20.0 * np.log10(1.0 / (((a - b) ** 2 * mask).sum() / ((np.sum(mask) + 1e-10) * 3.0)) ** 0.5))


def cal_rmse(a, b, mask) -> float:
    """src/trainer/utils.py:357-370."""
    a, b, mask = (x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x) for x in (a, b, mask))
    if mask.ndim == a.ndim - 1:
        mask = mask[..., None]
    return float((((a - b) ** 2 * mask).sum() / (np.sum(mask) + 1e-10)) ** 0.5)


def _on_gpu(*tensors) -> bool:
    return all(torch.is_tensor(t) and t.is_cuda for t in tensors if t is not None)


def _engine_for(t, engine):
    if engine is None:
        from .engine import Engine
        engine = Engine(t.device)
    return engine


def cal_ssim(a, b, mask, device=None, engine=None) -> float:
    """src/trainer/utils.py:444-457 (and the SSIM class above it): the mean structural similarity of two stacks [n,H,W,C] times
    ``mask`` ([n,H,W,1] or [n,H,W]; None = ones), with L = 1.  Device tensors go through ``Engine.ssim`` (csrc/metrics.hip; an
    ``Engine`` of their device is made when none is given), anything else through the numpy twin ``imaging.ssim``; ``device`` is
    accepted for the reference's signature and ignored.  Contract and the one divergence (L is not guessed from the image): DESIGN 7d."""
    if _on_gpu(a, b, mask):
        engine = _engine_for(a, engine)
        with torch.cuda.device(engine.device):
            return float(engine.ssim(a, b, mask)["mean"])
    from .imaging import ssim
    as_np = lambda x: None if x is None else (x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x))
    return ssim(as_np(a), as_np(b), as_np(mask))[0]


def cal_psnr_device(a, b, mask, engine=None) -> float:
    """``cal_psnr`` of fp32 device stacks [n,H,W,C] without copying them to the host: fp64 sums on the device
    (``Engine.masked_sq_sums``), two numbers read back."""
    from .imaging import psnr_from_sums
    engine = _engine_for(a, engine)
    with torch.cuda.device(engine.device):
        q = engine.masked_sq_sums(a, b, mask)
        return psnr_from_sums(float(q["S_total"]), float(q["M_total"]))


def cal_rmse_device(a, b, mask, engine=None) -> float:
    """``cal_rmse`` of fp32 device stacks, as ``cal_psnr_device``."""
    from .imaging import rmse_from_sums
    engine = _engine_for(a, engine)
    with torch.cuda.device(engine.device):
        q = engine.masked_sq_sums(a, b, mask)
        return rmse_from_sums(float(q["S_total"]), float(q["M_total"]))


def to8b(img):
    """An image in [0, 1] as the uint8 the reference writes its panels with (src/trainer/utils.py to8b: 255 clip(x, 0, 1), truncated);
    a numpy array, ready for ``write_png``."""
    x = img.detach().cpu().numpy() if torch.is_tensor(img) else np.asarray(img)
    return (255 * np.clip(x, 0, 1)).astype(np.uint8)


def write_png(path, array) -> None:
    """An 8-bit image as a PNG file with nothing but the standard library: ``array`` uint8 [H,W] / [H,W,1] (grey) or [H,W,3] (RGB), a
    numpy array or a tensor (a device tensor is copied to the host).  One IDAT chunk, every row with filter type 0, no interlace."""
    import struct
    import zlib
    x = array.detach().cpu().numpy() if torch.is_tensor(array) else np.asarray(array)
    if x.ndim == 3 and x.shape[-1] == 1:
        x = x[..., 0]
    if x.dtype != np.uint8 or x.ndim not in (2, 3) or (x.ndim == 3 and x.shape[-1] != 3) or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"write_png takes a non-empty uint8 [H, W], [H, W, 1] or [H, W, 3] image (got {x.dtype} {x.shape})")
    h, w = x.shape[:2]
    rows = np.ascontiguousarray(x).reshape(h, -1)
    raw = np.concatenate([np.zeros((h, 1), np.uint8), rows], axis=1).tobytes()          # filter byte 0 in front of every row

    def chunk(kind: bytes, body: bytes) -> bytes:
        return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)

    ihdr = struct.pack(">IIBBBBB", w, h, 8, 2 if x.ndim == 3 else 0, 0, 0, 0)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", ihdr) + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def depth_points(depth, intrinsics, pose, depth_trunc) -> torch.Tensor:
    """The point cloud of one depth frame (what the reference's gen_pcd makes through Open3D, src/trainer/utils.py:249-277, with
    ``project_valid_depth_only``): for every pixel with 0 < depth <= depth_trunc, in pixel order,
    pose[:3,:3] @ (K^-1 [x, y, 1] * depth) + pose[:3,3] with integer pixel coordinates: ``get_rays``' convention, depth being the
    z-depth of the point in the camera frame.  depth [H,W] (or [H,W,1]), intrinsics and pose [4,4] (camera to world; intrinsics
    may be [3,3]) -> [M,3] fp32 on ``depth``'s device.  One synchronisation (the number of valid pixels)."""
    d = torch.as_tensor(depth, dtype=torch.float32)
    if d.dim() == 3 and d.shape[-1] == 1:
        d = d[..., 0]
    if d.dim() != 2:
        raise ValueError(f"depth must be [H, W] or [H, W, 1] (got {tuple(d.shape)})")
    dev = d.device
    k = torch.as_tensor(intrinsics, dtype=torch.float32).to(dev)
    c2w = torch.as_tensor(pose, dtype=torch.float32).to(dev)
    h, w = d.shape
    ys, xs = torch.meshgrid(torch.arange(h, device=dev, dtype=torch.float32), torch.arange(w, device=dev, dtype=torch.float32), indexing="ij")
    valid = (d > 0) & (d <= float(depth_trunc))
    pix = torch.stack([xs[valid], ys[valid], torch.ones_like(xs[valid])], -1)                   # [M,3]
    cam = (pix @ torch.inverse(k[:3, :3]).T) * d[valid][:, None]
    return cam @ c2w[:3, :3].T + c2w[:3, 3][None]


def cal_geometric_error(points, vertices, depth_scale: float = 1.0, engine=None) -> float:
    """The reference's 3D metric for one frame (trainer_endosurf.py demo: ``pcd_gt.compute_point_cloud_distance(mesh vertices)``
    averaged, times the depth scale): mean over ``points`` [M,3] (the ground truth, ``depth_points``) of the distance to the nearest
    row of ``vertices`` [V,3], times ``depth_scale``.  Device tensors go through ``engine.nearest`` (an ``Engine`` of their device is
    made when none is given), anything else through the numpy twin ``meshing.nearest``.  nan for an empty cloud, inf for no vertices."""
    if torch.is_tensor(points) and torch.is_tensor(vertices) and points.is_cuda and vertices.is_cuda:
        if engine is None:
            from .engine import Engine
            engine = Engine(points.device)
        with torch.cuda.device(engine.device):
            dist, _ = engine.nearest(points, vertices)
        return float(dist.double().mean()) * float(depth_scale) if dist.numel() else float("nan")
    from .meshing import nearest
    as_np = lambda a: a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    dist, _ = nearest(as_np(points), as_np(vertices))
    return float(dist.astype(np.float64).mean()) * float(depth_scale) if dist.size else float("nan")


def cal_surface_error(points, vertices, triangles, depth_scale: float = 1.0, engine=None) -> float:
    """``cal_geometric_error`` measured to the surface instead of its vertices: the mean over ``points`` [M,3] of the exact distance to
    the triangle mesh ``vertices`` [V,3] / ``triangles`` [T,3] (``point_to_mesh``: the closest point of the closest triangle), times
    ``depth_scale``.  It does not depend on how finely the surface is tessellated.  Device tensors go through
    ``engine.point_to_mesh`` (an ``Engine`` of their device is made when none is given), anything else through the numpy twin
    ``meshing.point_to_mesh``.  nan for an empty cloud, inf for a mesh without a valid triangle."""
    if all(torch.is_tensor(a) and a.is_cuda for a in (points, vertices, triangles)):
        if engine is None:
            from .engine import Engine
            engine = Engine(points.device)
        with torch.cuda.device(engine.device):
            dist = engine.point_to_mesh(points, vertices, triangles)[0]
        return float(dist.double().mean()) * float(depth_scale) if dist.numel() else float("nan")
    from .meshing import point_to_mesh
    as_np = lambda a: a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    dist = point_to_mesh(as_np(points), as_np(vertices), as_np(triangles))[0]
    return float(dist.astype(np.float64).mean()) * float(depth_scale) if dist.size else float("nan")


# ---- scene normalisation (the reference's data/endonerf/preprocess.py:55-112 create_endonerf_info, without Open3D) -------
def _as_f32(a, device=None):
    """``a`` (numpy array or tensor) as an fp32 tensor, on ``device`` when one is given."""
    t = torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a, dtype=torch.float32)
    return t if device is None else t.to(device)


def depth_percentile(values, q):
    """np.percentile (linear) of the non-zero entries of ``values`` without an fp64 copy of them: with v the sorted non-zero fp32
    values, M their number, p = q / 100 (M - 1) and k = floor(p): v[k] + (p - k)(v[k+1] - v[k]) in fp64.  ``q`` is one percentage
    (-> float) or a sequence of them (-> tuple of floats, from one sort).  A device tensor is sorted on the device and the two
    elements each q needs are read back (torch.quantile refuses inputs above 16 M elements); anything else is sorted by numpy."""
    qs = [float(x) for x in (q if isinstance(q, (tuple, list, np.ndarray)) else [q])]
    if any(not 0.0 <= x <= 100.0 for x in qs):
        raise ValueError(f"percentiles must be in [0, 100] (got {q!r})")
    if torch.is_tensor(values) and values.is_cuda:
        x = values.detach().reshape(-1).float()
        v = torch.sort(x[x != 0]).values
    else:
        x = (values.detach().cpu().numpy() if torch.is_tensor(values) else np.asarray(values)).astype(np.float32).reshape(-1)
        v = np.sort(x[x != 0])
    M = int(v.shape[0])
    if M == 0:
        raise ValueError("depth_percentile: there is no non-zero value")
    ps = [x / 100.0 * (M - 1) for x in qs]
    ks = [min(int(np.floor(p)), M - 1) for p in ps]
    idx = [i for k in ks for i in (k, min(k + 1, M - 1))]
    ends = v[torch.as_tensor(idx, device=v.device)].double().tolist() if torch.is_tensor(v) else v[idx].astype(np.float64).tolist()
    out = tuple(ends[2 * i] + (p - k) * (ends[2 * i + 1] - ends[2 * i]) for i, (p, k) in enumerate(zip(ps, ks)))
    return out if isinstance(q, (tuple, list, np.ndarray)) else out[0]


def _compact(mask, *tensors):
    """The rows of every tensor where ``mask`` is set (one count read back for all of them)."""
    idx = torch.nonzero(mask).reshape(-1)
    return [t[idx] for t in tensors]


def _outlier_pass(pts, nb_points, radius_factor, engine):
    """One radius-outlier pass over ``pts`` [P,3] as the reference runs it (preprocess.py:79-80): radius = ``radius_factor`` x the fp64
    mean of the finite self-nearest distances, kept = ``radius_outlier_mask``.  (kept bool [P], radius 0-dim fp64), both on ``pts``'
    device; on the GPU the radius never leaves it."""
    if pts.is_cuda:
        dist, _ = engine.self_nearest(pts)
        fin = torch.isfinite(dist)
        radius = float(radius_factor) * (torch.where(fin, dist, torch.zeros_like(dist)).double().sum() / fin.sum())
        return engine.radius_outlier_mask(pts, nb_points, radius), radius
    from .meshing import radius_outlier_mask, self_nearest
    p = pts.numpy()
    dist, _ = self_nearest(p)
    fin = np.isfinite(dist)
    radius = float(radius_factor) * (dist[fin].astype(np.float64).mean() if fin.any() else float("nan"))
    return torch.from_numpy(radius_outlier_mask(p, nb_points, radius)), torch.tensor(radius, dtype=torch.float64)


def scene_normalization(depths, intrinsics, poses, masks=None, percentiles=(3.0, 99.9), down_sample=1.0, u=None, nb_points=5,
                        radius_factor=20.0, object_scale_in_sphere=0.6, pad=(-5.0, -5.0, 10.0), engine=None) -> Dict:
    """The unit-sphere normalisation of a raw RGB-D sequence, as the reference's create_endonerf_info derives it through Open3D
    (data/endonerf/preprocess.py:55-112): ``depths`` [n,H,W] (or [n,H,W,1]), ``intrinsics`` and camera-to-world ``poses`` [n,4,4],
    ``masks`` [n,H,W(,1)] (0 = ignore the pixel).  Device tensors go through the ``Engine`` (one of their device is made when none is
    given), anything else through the brute-force numpy twins of ``meshing`` -- O(P^2) per frame, so host arrays of real size want
    ``down_sample`` well below 1, or the device.

      1. depths are zeroed where ``masks == 0``; (close, inf) = ``depth_percentile`` of the non-zero depths at ``percentiles``; depths
         above inf and non-zero depths below close are zeroed (compared in fp64);
      2. per frame: ``depth_points(depth, K, pose, depth_trunc=inf)``; a pixel stays iff ``u[frame, y, x] < down_sample`` (``u``
         [n,H,W] uniform draws, torch.rand when not given; skipped entirely at ``down_sample >= 1``) -- a Bernoulli draw per pixel,
         where Open3D's random_down_sample shuffles and keeps an exact count; then one outlier pass: radius = ``radius_factor`` x the
         fp64 mean self-nearest distance, kept iff more than ``nb_points`` rows within it (``meshing.radius_outlier_mask``); the
         frame's box (lo_i, hi_i) is that of its kept points;
      3. the kept points of all frames, concatenated, go through the same outlier pass once more;
      4. centre = (lo + hi) / 2 of the merged box, radius = max |p - centre| / ``object_scale_in_sphere`` (fp64 on the fp32 points).

    Returns ``scale_mat`` [4,4] fp32 (diag(radius, radius, radius, 1), the centre as translation), ``depth_norm_scale`` (= radius,
    float), ``bbox_minmax`` [n,3,2] fp64 = stack([(lo_i - centre) / radius - pad / radius, (hi_i - centre) / radius + pad / radius], -1)
    (``pad`` in the depths' unit), ``close_depth``, ``inf_depth`` (floats), ``counts`` (per frame: valid, sampled, kept; merged: the
    kept total), ``points`` [kept total, 3] fp32, the merged cloud normalised into the sphere (frame by frame, pixel order inside a
    frame) and ``kept_mask`` [n,H,W] bool, the pixels those points come from.  Tensors live on ``depths``' device.
    A frame left without points raises ValueError.  Dropped rows are compacted, which costs the host one count per compaction."""
    d = _as_f32(depths)
    dev = d.device
    d = d[..., 0] if d.dim() == 4 else d
    k, c2w = _as_f32(intrinsics, dev), _as_f32(poses, dev)
    n = int(d.shape[0])
    if d.dim() != 3 or tuple(k.shape) != (n, 4, 4) or tuple(c2w.shape) != (n, 4, 4):
        raise ValueError(f"scene_normalization takes depths [n,H,W], intrinsics and poses [n,4,4] (got {tuple(d.shape)}, {tuple(k.shape)}, {tuple(c2w.shape)})")
    if masks is not None:
        m = _as_f32(masks, dev)
        d = torch.where((m[..., 0] if m.dim() == 4 else m) == 0, torch.zeros_like(d), d)
    close, inf = depth_percentile(d, tuple(percentiles))
    d64 = d.double()
    d = torch.where((d64 > inf) | ((d64 < close) & (d64 != 0)), torch.zeros_like(d), d)
    del d64
    ratio = float(down_sample)
    if ratio < 1.0:
        u = torch.rand(d.shape, device=dev) if u is None else _as_f32(u, dev).reshape(d.shape)
    if dev.type == "cuda":
        engine = _engine_for(d, engine)
    counts = {"valid": [], "sampled": [], "kept": [], "merged": 0}
    clouds, pixels, boxes = [], [], []
    hw = int(d.shape[1] * d.shape[2])
    with torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext():
        for i in range(n):
            pts = depth_points(d[i], k[i], c2w[i], depth_trunc=inf)
            pix = torch.nonzero(((d[i] > 0) & (d[i] <= inf)).reshape(-1)).reshape(-1)          # depth_points' pixels, in its order
            counts["valid"].append(int(pts.shape[0]))
            if ratio < 1.0:
                pts, pix = _compact(u[i].reshape(-1)[pix] < ratio, pts, pix)
            counts["sampled"].append(int(pts.shape[0]))
            pts, pix = _compact(_outlier_pass(pts, nb_points, radius_factor, engine)[0], pts, pix)
            counts["kept"].append(int(pts.shape[0]))
            if pts.shape[0] == 0:
                raise ValueError(f"scene_normalization: frame {i} is left without points ({counts['valid'][-1]} valid pixels, "
                                 f"{counts['sampled'][-1]} sampled)")
            clouds.append(pts)
            pixels.append(pix + i * hw)
            boxes.append(torch.stack([pts.amin(0), pts.amax(0)]))
        merged, pix = torch.cat(clouds), torch.cat(pixels)
        merged, pix = _compact(_outlier_pass(merged, nb_points, radius_factor, engine)[0], merged, pix)
    counts["merged"] = int(merged.shape[0])
    if merged.shape[0] == 0:
        raise ValueError("scene_normalization: the merged cloud is left without points")
    kept_mask = torch.zeros(n * hw, dtype=torch.bool, device=dev)
    kept_mask[pix] = True
    p64 = merged.double()
    centre = (p64.amin(0) + p64.amax(0)) / 2
    radius = torch.linalg.norm(p64 - centre, dim=-1).max() / float(object_scale_in_sphere)
    scale_mat = torch.diag(torch.cat([radius.expand(3), radius.new_ones(1)]))
    scale_mat[:3, 3] = centre
    box = torch.stack(boxes).double()          # [n, 2, 3]
    pad_n = torch.as_tensor([float(x) for x in pad], dtype=torch.float64, device=dev) / radius
    bbox_minmax = torch.stack([(box[:, 0] - centre) / radius - pad_n, (box[:, 1] - centre) / radius + pad_n], -1)
    return {"scale_mat": scale_mat.float(), "depth_norm_scale": float(radius), "bbox_minmax": bbox_minmax, "close_depth": close, "inf_depth": inf,
            "counts": counts, "points": ((p64 - centre) / radius).float(), "kept_mask": kept_mask.view(n, *d.shape[1:])}


def normalize_cameras(intrinsics, poses, scale_mat):
    """The cameras of the normalised scene: what the reference's Dataset.__init__ gets from decomposing ``world_mat @ scale_mat``
    (src/dataset/dataset.py:51-58), in closed form.  ``scale_mat`` = [[r I, c], [0, 1]] is a similarity, so K [R^T | -R^T t] scale_mat
    = r K [R^T | -R^T (t - c) / r]: the intrinsics and the rotation are unchanged, the camera centre becomes (t - c) / r (fp64, then
    the poses' dtype).  ``intrinsics`` and camera-to-world ``poses`` [n,4,4] -> (intrinsics, poses), tensors on ``poses``' device."""
    c2w = poses if torch.is_tensor(poses) else torch.as_tensor(np.asarray(poses))
    k = (intrinsics if torch.is_tensor(intrinsics) else torch.as_tensor(np.asarray(intrinsics))).to(c2w.device)
    s = (scale_mat if torch.is_tensor(scale_mat) else torch.as_tensor(np.asarray(scale_mat))).to(c2w.device).double()
    out = c2w.clone()
    out[..., :3, 3] = ((c2w[..., :3, 3].double() - s[:3, 3]) / s[0, 0]).to(c2w.dtype)
    return k.clone(), out


# ---- stereo pairs to depth frames (the reference's data/scared2019/preprocess.py:98-117, with the matcher it leaves to an external
# network) -------------------------------------------------------------------------------------------------------------
def disparity_to_depth(disp, disp_const, near=None, far=None) -> torch.Tensor:
    """The depth of a disparity map as the reference's SCARED preprocessing derives it (preprocess.py:100-107): ``disp_const / disp``
    where ``disp > 0`` and 0 elsewhere, then 0 where the depth is above ``far`` or below ``near`` (each may be None).  ``disp_const``
    = focal length x baseline.  The quotient is taken in fp64 and rounded to fp32 once, the comparisons are made in fp64: the same
    bits on the host and on the device.  Returns an fp32 tensor on ``disp``'s device."""
    d = torch.as_tensor(disp, dtype=torch.float32)
    seen = d > 0
    depth = torch.where(seen, float(disp_const) / torch.where(seen, d, torch.ones_like(d)).double(), torch.zeros_like(d, dtype=torch.float64))
    if far is not None:
        depth = torch.where(depth.float().double() > float(far), torch.zeros_like(depth), depth)
    if near is not None:
        depth = torch.where(depth.float().double() < float(near), torch.zeros_like(depth), depth)
    return depth.float()


def close_mask(mask, k) -> torch.Tensor:
    """Morphological closing of ``mask`` [..., H, W] with a ``k`` x ``k`` box, anchor at ``k // 2``: dilation (the maximum over the
    reflected box) then erosion (the minimum over the box), the border never winning either extreme.  What the reference gets from
    ``cv2.morphologyEx(depth_mask, cv2.MORPH_CLOSE, np.ones((k, k)))`` with ``k = int(w / 128)`` (preprocess.py:112-113); OpenCV is not
    a dependency and the result is not pinned against it.  Two ``max_pool2d`` over a padding of -inf; the mask's dtype is kept."""
    import torch.nn.functional as F
    m = torch.as_tensor(mask)
    k = int(k)
    if k < 1 or m.dim() < 2:
        raise ValueError(f"close_mask takes a mask [..., H, W] and k >= 1 (got {tuple(m.shape)}, k = {k})")
    a, b = k // 2, k - 1 - k // 2
    x = m.to(torch.float32).reshape(-1, 1, *m.shape[-2:])
    inf = float("inf")
    x = F.max_pool2d(F.pad(x, (b, a, b, a), value=-inf), k, 1)           # dilation: offsets -b .. a
    x = -F.max_pool2d(F.pad(-x, (a, b, a, b), value=-inf), k, 1)         # erosion: offsets -a .. b
    return x.reshape(m.shape).to(m.dtype)


def stereo_depth(left, right, focal, baseline, max_disparity, near=None, far=None, close=None, engine=None, **matcher_args) -> Dict:
    """A rectified stereo pair (or a stack of pairs) to depth: ``stereo.stereo_disparity`` -- census cost, semi-global matching,
    uniqueness, left-right and speckle tests, sub-pixel disparity -- then ``disparity_to_depth`` with ``focal * baseline`` and the two
    masks of the reference's preprocessing.  ``left`` / ``right`` [H,W(,3)] or [n,H,W(,3)], uint8 or float in [0,1]; the left image is
    the reference view.  Device tensors go through ``Engine.stereo_disparity`` (csrc/stereo.hip; an ``Engine`` of their device is
    made when none is given), anything else through the numpy twin; both give the same bits.  Returns tensors on the inputs' device:
    ``disparity`` fp32 (0 = no match), ``depth`` fp32 (z-depth, ``depth_points``' convention; 0 = none), ``valid`` bool (the matcher's),
    ``depth_mask`` bool (depth > 0) and ``color_mask`` bool (``close_mask(depth_mask, close or max(1, W // 128))``)."""
    if _on_gpu(left, right):
        engine = _engine_for(left, engine)
        with torch.cuda.device(engine.device):
            r = engine.stereo_disparity(left, right, max_disparity, **matcher_args)
        disparity, valid = r["disparity"], r["valid"]
    else:
        from .stereo import stereo_disparity
        as_np = lambda x: x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
        matcher_args.pop("poll", None)          # (how often the device's speckle filter reads its word back; the twin has none)
        r = stereo_disparity(as_np(left), as_np(right), max_disparity, **matcher_args)
        disparity, valid = torch.from_numpy(r["disparity"]), torch.from_numpy(r["valid"])
    depth = disparity_to_depth(disparity, float(focal) * float(baseline), near, far)
    depth_mask = depth > 0
    k = int(close) if close else max(1, int(disparity.shape[-1]) // 128)
    return {"disparity": disparity, "depth": depth, "valid": valid, "depth_mask": depth_mask, "color_mask": close_mask(depth_mask, k)}


# ---- binary PLY files (the reference's demo writes its meshes through Open3D, trainer_endosurf.py:447-466) ---------------
PLY_VERTEX_PROPS = ("x", "y", "z")
PLY_NORMAL_PROPS = ("nx", "ny", "nz")
PLY_COLOR_PROPS = ("red", "green", "blue")
PLY_FACE_LINE = "property list uchar int vertex_indices"


def ply_header(n_vertices, n_faces=None, colors=False, normals=False, comment=None) -> bytes:
    """The header ``write_ply`` puts in front of ``ply_body``: ``n_faces=None`` declares no face element (a point cloud)."""
    lines = ["ply", "format binary_little_endian 1.0"]
    if comment is not None:
        for c in str(comment).splitlines() or [""]:
            lines.append(f"comment {c}")
    lines.append(f"element vertex {int(n_vertices)}")
    lines += [f"property float {p}" for p in PLY_VERTEX_PROPS]
    if normals:
        lines += [f"property float {p}" for p in PLY_NORMAL_PROPS]
    if colors:
        lines += [f"property uchar {p}" for p in PLY_COLOR_PROPS]
    if n_faces is not None:
        lines += [f"element face {int(n_faces)}", PLY_FACE_LINE]
    lines.append("end_header")
    return ("\n".join(lines) + "\n").encode("ascii")


def _ply_vertex_dtype(colors, normals):
    fields = [(p, "<f4") for p in PLY_VERTEX_PROPS]
    if normals:
        fields += [(p, "<f4") for p in PLY_NORMAL_PROPS]
    if colors:
        fields += [(p, "u1") for p in PLY_COLOR_PROPS]
    return np.dtype(fields)          # packed: 12, 24, 15 or 27 bytes


_PLY_FACE_DTYPE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])          # packed: 13 bytes


def _ply_rows(a, name, n=None):
    a = np.asarray(a, np.float32)
    if a.ndim != 2 or a.shape[1] != 3 or (n is not None and a.shape[0] != n):
        raise ValueError(f"{name} must be [V, 3]" + (f" with V = {n}" if n is not None else "") + f" (got {a.shape})")
    return a


def ply_body(vertices, triangles=None, colors=None, normals=None) -> np.ndarray:
    """The body of a ``binary_little_endian 1.0`` PLY file as a uint8 array (numpy twin of ``Engine.ply_pack``).  Per vertex:
    ``float x y z`` (fp32), then ``float nx ny nz`` when ``normals`` [V, 3] are given, then ``uchar red green blue`` when ``colors``
    [V, 3] are given.  Colours are floats in [0, 1], quantised by the rule of ``to8b`` on fp32: trunc(255 * clip(c, 0, 1)), the product
    rounded to fp32 -- so a value below 0 gives 0, a value above 1 gives 255, 1.0 gives 255, 0.5 gives 127, and k / 255 gives k or k - 1
    as the fp32 product falls; NaN gives 0.  Then per triangle ``uchar 3`` and three ``int`` (int32) indices, 13 bytes.
    ``triangles=None`` gives a point cloud's body."""
    v = _ply_rows(vertices, "vertices")
    rec = np.zeros(len(v), _ply_vertex_dtype(colors is not None, normals is not None))
    for j, p in enumerate(PLY_VERTEX_PROPS):
        rec[p] = v[:, j]
    if normals is not None:
        nn = _ply_rows(normals, "normals", len(v))
        for j, p in enumerate(PLY_NORMAL_PROPS):
            rec[p] = nn[:, j]
    if colors is not None:
        c = _ply_rows(colors, "colors", len(v))
        c8 = to8b(np.where(np.isnan(c), np.float32(0), c))
        for j, p in enumerate(PLY_COLOR_PROPS):
            rec[p] = c8[:, j]
    parts = [np.frombuffer(rec.tobytes(), np.uint8)]
    if triangles is not None:
        t = np.asarray(triangles)
        t = np.zeros((0, 3), np.int32) if t.size == 0 else t
        if t.ndim != 2 or t.shape[1] != 3 or not np.issubdtype(t.dtype, np.integer):
            raise ValueError(f"triangles must be an integer [T, 3] array (got {t.dtype} {t.shape})")
        face = np.zeros(len(t), _PLY_FACE_DTYPE)
        face["n"] = 3
        face["v"] = t.astype(np.int32)
        parts.append(np.frombuffer(face.tobytes(), np.uint8))
    return np.concatenate(parts)


def write_ply(path, vertices, triangles=None, colors=None, normals=None, comment=None, engine=None) -> None:
    """A mesh or a point cloud as a ``binary_little_endian 1.0`` PLY file: ``ply_header`` then the body of ``ply_body``, whose
    docstring is the layout and the colour rule.  ``vertices`` [V, 3]; ``triangles`` [T, 3] integers or None (a point cloud: no face
    element); ``colors`` [V, 3] floats in [0, 1] or None; ``normals`` [V, 3] or None; ``comment``: one header line per line of text.
    When ``vertices`` is a device tensor the body is packed on the device (``Engine.ply_pack``; the other arrays are moved there if
    need be; an ``Engine`` of that device is made when none is given) and crosses to the host in one copy; anything else goes through
    the numpy packer.  Coordinates are written as fp32 (Open3D writes doubles)."""
    T = None if triangles is None else int(triangles.shape[0]) if hasattr(triangles, "shape") else len(triangles)
    if torch.is_tensor(vertices) and vertices.is_cuda:
        engine = _engine_for(vertices, engine)
        on = lambda a: None if a is None else torch.as_tensor(a).to(engine.device)
        with torch.cuda.device(engine.device):
            body = engine.ply_pack(vertices, on(triangles), on(colors), on(normals)).cpu().numpy()
    else:
        as_np = lambda a: None if a is None else (a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a))
        body = ply_body(as_np(vertices), as_np(triangles), as_np(colors), as_np(normals))
    with open(path, "wb") as f:
        f.write(ply_header(int(vertices.shape[0]) if hasattr(vertices, "shape") else len(vertices), T, colors is not None, normals is not None, comment))
        f.write(body.tobytes())


def read_ply(path) -> Dict[str, np.ndarray]:
    """What ``write_ply`` wrote, as numpy arrays: ``vertices`` [V, 3] float32, ``triangles`` [T, 3] int32 when the file has a face
    element, ``normals`` [V, 3] float32 and ``colors`` [V, 3] uint8 when it has them, ``comments`` (a list of strings) when it has any.
    Raises ValueError for any other PLY file: ascii or big-endian data, other elements, properties, types or orders, faces that are not
    triangles, a body of the wrong length."""
    with open(path, "rb") as f:
        raw = f.read()
    end = raw.find(b"end_header\n")
    if not raw.startswith(b"ply\n") or end < 0:
        raise ValueError(f"{path}: not a PLY file (no 'ply' magic or no end_header line)")
    try:
        lines = raw[:end].decode("ascii").split("\n")[1:-1]
    except UnicodeDecodeError:
        raise ValueError(f"{path}: the PLY header is not ASCII") from None
    body = raw[end + len(b"end_header\n"):]
    if not lines or not lines[0].startswith("format "):
        raise ValueError(f"{path}: the PLY header has no format line")
    if lines[0] != "format binary_little_endian 1.0":
        raise ValueError(f"{path}: only 'format binary_little_endian 1.0' is read (got {lines[0]!r})")
    comments = [ln[len("comment "):] for ln in lines[1:] if ln.startswith("comment ") or ln == "comment"]
    rest = [ln for ln in lines[1:] if not (ln.startswith("comment ") or ln == "comment")]
    if not rest or not rest[0].startswith("element vertex "):
        raise ValueError(f"{path}: expected 'element vertex N' (got {rest[0] if rest else 'nothing'!r})")
    try:
        V = int(rest[0].split()[2])
    except (IndexError, ValueError):
        raise ValueError(f"{path}: bad vertex count in {rest[0]!r}") from None
    face_at = [i for i, ln in enumerate(rest) if ln.startswith("element ") and i > 0]
    props = rest[1:face_at[0]] if face_at else rest[1:]
    want = {(c, n): [f"property float {p}" for p in PLY_VERTEX_PROPS] + ([f"property float {p}" for p in PLY_NORMAL_PROPS] if n else [])
            + ([f"property uchar {p}" for p in PLY_COLOR_PROPS] if c else []) for c in (False, True) for n in (False, True)}
    match = [k for k, v in want.items() if v == props]
    if not match:
        raise ValueError(f"{path}: vertex properties other than float x y z [float nx ny nz] [uchar red green blue]: {props}")
    has_colors, has_normals = match[0]
    T = None
    if face_at:
        tail = rest[face_at[0]:]
        if len(tail) != 2 or not tail[0].startswith("element face ") or tail[1] != PLY_FACE_LINE:
            raise ValueError(f"{path}: after the vertex element only 'element face N' with '{PLY_FACE_LINE}' is read (got {tail})")
        try:
            T = int(tail[0].split()[2])
        except (IndexError, ValueError):
            raise ValueError(f"{path}: bad face count in {tail[0]!r}") from None
    vdt = _ply_vertex_dtype(has_colors, has_normals)
    if V < 0 or (T is not None and T < 0) or len(body) != V * vdt.itemsize + (T or 0) * _PLY_FACE_DTYPE.itemsize:
        raise ValueError(f"{path}: the body has {len(body)} bytes, the header promises {V} vertices of {vdt.itemsize} bytes"
                         + (f" and {T} faces of 13" if T is not None else ""))
    rec = np.frombuffer(body, vdt, count=V)
    out = {"vertices": np.stack([rec[p] for p in PLY_VERTEX_PROPS], -1).astype(np.float32).reshape(V, 3)}
    if has_normals:
        out["normals"] = np.stack([rec[p] for p in PLY_NORMAL_PROPS], -1).astype(np.float32).reshape(V, 3)
    if has_colors:
        out["colors"] = np.stack([rec[p] for p in PLY_COLOR_PROPS], -1).astype(np.uint8).reshape(V, 3)
    if T is not None:
        face = np.frombuffer(body, _PLY_FACE_DTYPE, count=T, offset=V * vdt.itemsize)
        if T and (face["n"] != 3).any():
            raise ValueError(f"{path}: a face that is not a triangle")
        out["triangles"] = np.ascontiguousarray(face["v"]).astype(np.int32).reshape(T, 3)
    if comments:
        out["comments"] = comments
    return out
