"""The depth-fusion methods of ``engine.Engine`` (a mixin): the TSDF integration of a block of depth frames in one launch, the
elementwise finalisation and the trilinear volume sampler (csrc/fuse.hip); ``fusion`` is the specification and the fp64 twin (DESIGN.md
7p).  Arguments and results are device tensors; nothing is read back."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import fusion
from ._device import f32, u8
from ._lib import check, ptr


class FuseMixin:
    def _fuse_dev(self, a, what, shape=None, dtype=torch.float32):
        if not torch.is_tensor(a) or a.device != self.device or (shape is not None and tuple(a.shape) != tuple(shape)):
            got = f"{tuple(a.shape)} on {a.device}" if torch.is_tensor(a) else type(a).__name__
            raise ValueError(f"Engine.{what} takes a {'' if shape is None else list(shape)} tensor on {self.device}; device tensors only (got {got})")
        return a.detach().to(dtype).contiguous()

    def tsdf_state(self, N, with_color=True):
        """``fusion.new_state`` on the device: zeroed dict(tsdf_sum [N], weight [N], color_sum [N,3] or None)."""
        N = int(N)
        zeros = lambda *shape: torch.zeros(*shape, device=self.device)          # (never a slice of the step arena: the state outlives a step)
        return {"tsdf_sum": zeros(N), "weight": zeros(N), "color_sum": zeros(N, 3) if with_color else None}

    def _tsdf_state_arg(self, state, what):
        ts, wt, cs = state["tsdf_sum"], state["weight"], state.get("color_sum")
        N = int(ts.shape[0])
        for a, shape in ((ts, (N,)), (wt, (N,))) + (((cs, (N, 3)),) if cs is not None else ()):
            if not torch.is_tensor(a) or a.device != self.device or a.dtype != torch.float32 or tuple(a.shape) != shape or not a.is_contiguous():
                raise ValueError(f"Engine.{what}: the state must be contiguous fp32 tsdf_sum [N], weight [N] and color_sum [N, 3] or None on {self.device}")
        return ts, wt, cs, N

    def tsdf_integrate(self, state, positions, depth, cameras, color=None, mask=None, valid=None, trunc=None, depth_trunc=math.inf):
        """``fusion.integrate`` in ONE launch: the frames ``depth`` [F,H,W] (``color`` [F,H,W,3], ``mask`` [F,H,W], each or None) seen
        by ``cameras`` (``flow_cameras``: [F,17] fp64 on the device) into ``state`` (``tsdf_state``'s dict, updated in place and
        returned) at ``positions`` [N,3] (one lattice for all frames) or [F,N,3] (with ``valid`` [F,N] or None).  A voxel's frames are
        taken in index order inside its thread: the same bits however the frames are split into calls or the voxels into chunks."""
        if trunc is None:
            raise TypeError("tsdf_integrate needs trunc")
        trunc, depth_trunc = fusion.check_trunc(trunc, depth_trunc)
        ts, wt, cs, N = self._tsdf_state_arg(state, "tsdf_integrate")
        dep = self._fuse_dev(depth, "tsdf_integrate")
        if dep.dim() != 3:
            raise ValueError(f"tsdf_integrate takes depth [F, H, W] (got {tuple(dep.shape)})")
        F, H, W = (int(s) for s in dep.shape)
        pos = self._fuse_dev(positions, "tsdf_integrate")
        if tuple(pos.shape) not in ((N, 3), (F, N, 3)):
            raise ValueError(f"tsdf_integrate: {N} voxels and {F} frames take positions [{N}, 3] or [{F}, {N}, 3] (got {tuple(pos.shape)})")
        stride = N if pos.dim() == 3 else 0
        if not torch.is_tensor(cameras) or cameras.dtype != torch.float64 or cameras.device != self.device or tuple(cameras.shape) != (F, 17):
            raise ValueError(f"tsdf_integrate takes fp64 cameras [{F}, 17] on {self.device} (Engine.flow_cameras)")
        if (color is None) != (cs is None):
            raise ValueError("tsdf_integrate: color and the state's color_sum go together")
        col = None if color is None else self._fuse_dev(color, "tsdf_integrate", (F, H, W, 3))
        flags = lambda a, shape: u8(self._fuse_dev(a, "tsdf_integrate", shape, getattr(a, "dtype", None)) != 0)
        msk = None if mask is None else flags(mask, (F, H, W))
        valid = None if valid is None else flags(valid, (F, N))
        check(self.lib.es_tsdf_integrate(ptr(pos), stride, ptr(valid), N, F, ptr(dep), ptr(col), ptr(msk), ptr(cameras.contiguous()), H, W,
                                         trunc, depth_trunc, ptr(ts), ptr(wt), ptr(cs), self.st()), "es_tsdf_integrate")
        return state

    def tsdf_finalize(self, state):
        """``fusion.finalize`` in one launch: dict(tsdf [N], color [N,3] or None, weight [N] -- the state's own tensor)."""
        ts, wt, cs, N = self._tsdf_state_arg(state, "tsdf_finalize")
        tsdf, color = self.empty(N), (None if cs is None else self.empty(N, 3))
        check(self.lib.es_tsdf_finalize(ptr(ts), ptr(wt), ptr(cs), N, ptr(tsdf), ptr(color), self.st()), "es_tsdf_finalize")
        return {"tsdf": tsdf, "color": color, "weight": wt}

    def sample_volume(self, volume, points, bound_min, bound_max):
        """``fusion.sample_volume`` in one launch: ``volume`` [R,R,R] or [R,R,R,C] (C <= 8) at world ``points`` [M,3] -> (values [M] or
        [M,C] fp32, the fp64 blend rounded once; inside [M] bool).  The bounds are host numbers, read as fp64."""
        vol = self._fuse_dev(volume, "sample_volume")
        if vol.dim() not in (3, 4) or tuple(vol.shape[:3]) != (vol.shape[0],) * 3:
            raise ValueError(f"sample_volume takes a volume [R, R, R] or [R, R, R, C] (got {tuple(vol.shape)})")
        R, Cn = int(vol.shape[0]), (1 if vol.dim() == 3 else int(vol.shape[3]))
        pts = self._fuse_dev(points, "sample_volume")
        if pts.dim() != 2 or pts.shape[1] != 3:
            raise ValueError(f"sample_volume takes points [M, 3] (got {tuple(pts.shape)})")
        M = int(pts.shape[0])
        bounds = np.ascontiguousarray(np.concatenate([np.asarray(bound_min, np.float64).reshape(3), np.asarray(bound_max, np.float64).reshape(3)]))
        values, inside = self.empty(M, Cn), self.empty(M, dtype=torch.uint8)
        check(self.lib.es_volume_sample(ptr(vol), R, Cn, ptr(pts), M, bounds.ctypes.data_as(C.POINTER(C.c_double)), ptr(values), ptr(inside),
                                        self.st()), "es_volume_sample")
        return (values[:, 0] if vol.dim() == 3 else values), inside.view(torch.bool)
