"""The stereo methods of ``engine.Engine`` (a mixin): census transform, semi-global matching and disparity selection on the device,
csrc/stereo.hip; ``stereo`` is the specification and the twin, and every result here is its bits.  Results are device
tensors; nothing is read back except the one word the speckle filter polls."""
from __future__ import annotations

import torch

from . import stereo
from ._lib import EndoSurfHipError, check, ptr


class StereoMixin:
    # bytes of device memory one chunk of a stack may take (census, cost volume, S, scratch): a stack is processed in chunks of as many
    # pairs as fit, at least one.  An attribute, not an environment variable: ``engine.stereo_scratch_budget = ...``
    stereo_scratch_budget = 1 << 30

    def _stereo_grey(self, image, what):
        """``stereo.to_grey`` where the tensor lives: (uint8 [n,H,W] on this device, whether the input was a single image)."""
        x = torch.as_tensor(image)
        if x.is_floating_point():
            x = (x.detach().to(self.device, torch.float32).clamp(0, 1) * 255).to(torch.uint8)
        elif x.dtype != torch.uint8:
            raise ValueError(f"Engine.{what}: an image is uint8 or float in [0, 1] (got {x.dtype})")
        x = x.to(self.device)
        if x.dim() >= 3 and x.shape[-1] == 3:
            v = x.to(torch.int32)
            x = ((77 * v[..., 0] + 150 * v[..., 1] + 29 * v[..., 2] + 128) >> 8).to(torch.uint8)
        if x.dim() not in (2, 3):
            raise ValueError(f"Engine.{what} takes images [H, W(, 3)] or [n, H, W(, 3)] (got {tuple(x.shape)})")
        return (x[None] if x.dim() == 2 else x).contiguous(), x.dim() == 2

    def _stereo_chunk(self, n, H, W, D):
        """Pairs per chunk of a stack of ``n``: what ``stereo_scratch_budget`` admits, at least one, n H W D below 2^31."""
        per = H * W * (16 + 3 * D) + int(self.lib.es_stereo_scratch_bytes(1, H, W))
        return max(1, min(n, int(self.stereo_scratch_budget) // per, ((1 << 31) - 1) // (H * W * D)))

    def census(self, grey):
        """``stereo.census``: uint8 grey [H,W] or [n,H,W] -> int64 of the same shape."""
        g = torch.as_tensor(grey)
        if g.dtype != torch.uint8 or g.dim() not in (2, 3):
            raise ValueError(f"Engine.census takes uint8 grey [H, W] or [n, H, W] (got {g.dtype} {tuple(g.shape)})")
        g = g.to(self.device).contiguous()
        n, H, W = (1, *g.shape) if g.dim() == 2 else g.shape
        out = self.empty(g.shape, dtype=torch.int64)
        check(self.lib.es_stereo_census(ptr(g), int(n), int(H), int(W), ptr(out), self.st()), "es_stereo_census")
        return out

    def _sgm_into(self, gl, gr, D, dmin, p1, p2, paths, S):
        """S (a [c,H,W,D] uint16 slice, written) of the grey chunks ``gl`` / ``gr`` [c,H,W]: census, cost, aggregation."""
        c, H, W = (int(s) for s in gl.shape)
        st = self.st()
        cl, cr = self.empty(c, H, W, dtype=torch.int64), self.empty(c, H, W, dtype=torch.int64)
        check(self.lib.es_stereo_census(ptr(gl), c, H, W, ptr(cl), st), "es_stereo_census")
        check(self.lib.es_stereo_census(ptr(gr), c, H, W, ptr(cr), st), "es_stereo_census")
        cost = self.empty(c, H, W, D, dtype=torch.uint8)
        check(self.lib.es_sgm_cost(ptr(cl), ptr(cr), c, H, W, D, dmin, ptr(cost), st), "es_sgm_cost")
        check(self.lib.es_sgm_aggregate(ptr(cost), c, H, W, D, p1, p2, paths, ptr(S), st), "es_sgm_aggregate")

    def _stereo_pair(self, left, right, what):
        (gl, single), (gr, _) = self._stereo_grey(left, what), self._stereo_grey(right, what)
        if gl.shape != gr.shape:
            raise ValueError(f"Engine.{what}: a pair is two images of one shape (got {tuple(gl.shape)} and {tuple(gr.shape)})")
        return gl, gr, single

    def sgm_volume(self, left, right, max_disparity, min_disparity=0, p1=7, p2=60, paths=8):
        """``stereo.sgm_volume``: S [n,H,W,D] uint16 of a stack of pairs ([H,W,D] of one pair), images of any kind ``stereo.to_grey``
        takes.  The cost volume is scratch, made chunk by chunk under ``stereo_scratch_budget``."""
        D, dmin, p1, p2, paths = stereo.check_matcher(max_disparity, min_disparity, p1, p2, paths)[:5]
        gl, gr, single = self._stereo_pair(left, right, "sgm_volume")
        n, H, W = (int(s) for s in gl.shape)
        if H * W * D >= 1 << 31:
            raise EndoSurfHipError(f"sgm_volume: {H} x {W} x {D} does not fit int32 indices")
        S = self.empty(n, H, W, D, dtype=torch.uint16)
        step = self._stereo_chunk(n, H, W, D) if n else 1
        for a in range(0, n, step):
            self._sgm_into(gl[a:a + step], gr[a:a + step], D, dmin, p1, p2, paths, S[a:a + step])
        return S[0] if single else S

    def _sgm_select_into(self, S, dmin, uniqueness, lr_max, subpixel, out, scratch):
        c, H, W, D = (int(s) for s in S.shape)
        check(self.lib.es_sgm_select(ptr(S), c, H, W, D, dmin, uniqueness, lr_max, int(bool(subpixel)), ptr(out["d0"]), ptr(out["disparity"]),
                                     ptr(out["flags"]), ptr(out["valid"]), ptr(scratch), self.st()), "es_sgm_select")

    def _stereo_outputs(self, n, H, W):
        return {"disparity": self.empty(n, H, W), "valid": self.empty(n, H, W, dtype=torch.uint8),
                "d0": self.empty(n, H, W, dtype=torch.int32), "flags": self.empty(n, H, W, dtype=torch.uint8)}

    def _stereo_scratch(self, n, H, W):
        return self.empty(max(int(self.lib.es_stereo_scratch_bytes(n, H, W)), 16), dtype=torch.uint8)

    @staticmethod
    def _stereo_result(out, single):
        out = dict(out, valid=out["valid"].view(torch.bool))
        return {k: v[0] for k, v in out.items()} if single else out

    def sgm_select(self, S, min_disparity=0, uniqueness=10, lr_max=1, subpixel=True):
        """``stereo.select`` without the speckle filter: S uint16 [n,H,W,D] (or [H,W,D]) on this device, any values -> dict(disparity fp32, valid
        bool, d0 int32, flags uint8), each [n,H,W] ([H,W])."""
        if not torch.is_tensor(S) or S.dtype != torch.uint16 or S.dim() not in (3, 4) or S.device != self.device:
            raise ValueError(f"Engine.sgm_select takes S uint16 [n, H, W, D] or [H, W, D] on {self.device}")
        single = S.dim() == 3
        S = (S[None] if single else S).contiguous()
        n, H, W, D = (int(s) for s in S.shape)
        dmin, _, _, _, uniqueness, lr_max = stereo.check_matcher(D, min_disparity, uniqueness=uniqueness, lr_max=lr_max)[1:7]
        out = self._stereo_outputs(n, H, W)
        self._sgm_select_into(S, dmin, uniqueness, lr_max, subpixel, out, self._stereo_scratch(n, H, W))
        return self._stereo_result(out, single)

    def _speckle_into(self, out, size, max_diff, poll, scratch):
        """The speckle filter on the outputs ``out`` of one chunk, in place (``disparity`` and ``flags`` may be None)."""
        n, H, W = (int(s) for s in out["valid"].shape)
        poll = int(poll)
        if poll < 1:
            raise EndoSurfHipError(f"speckle_filter: poll must be at least 1 (got {poll})")
        if n == 0:
            return
        st = self.st()
        changed = self.empty(1, dtype=torch.int32)
        cap = H * W * n + poll          # (a label falls at least once per sweep until the fixed point)
        sweeps = 0
        while True:
            for i in range(poll):
                check(self.lib.es_speckle_label(ptr(out["d0"]), ptr(out["valid"]), n, H, W, max_diff, int(sweeps == 0 and i == 0), ptr(scratch),
                                                ptr(changed) if i == poll - 1 else None, st), "es_speckle_label")
            sweeps += poll
            if not int(changed.item()):
                break
            if sweeps >= cap:
                raise EndoSurfHipError(f"speckle_filter did not reach its fixed point in {sweeps} sweeps")
        check(self.lib.es_speckle_apply(n, H, W, size, ptr(scratch), ptr(out["valid"]), ptr(out["d0"]), ptr(out.get("disparity")),
                                        ptr(out.get("flags")), st), "es_speckle_apply")

    def speckle_filter(self, d0, valid, size, range=1, poll=8):
        """``stereo.speckle_keep``: d0 integer (any int32) and valid bool, [n,H,W] or [H,W] -> bool of the same shape, the valid pixels whose
        segment (valid 4-neighbours with |d0 - d0'| <= ``range``) has at least ``size`` pixels.  Labels are propagated by sweeps, one
        launch each; the host reads one word every ``poll`` sweeps.  The same bits for any ``poll``."""
        size, max_diff = stereo.check_matcher(1, speckle_size=size, speckle_range=range)[7:9]
        v = torch.as_tensor(valid).to(self.device)
        d = torch.as_tensor(d0).to(self.device, torch.int32)
        if v.shape != d.shape or v.dim() not in (2, 3):
            raise ValueError(f"Engine.speckle_filter takes d0 and valid of one shape, [n, H, W] or [H, W] (got {tuple(d.shape)}, {tuple(v.shape)})")
        single = v.dim() == 2
        out = {"valid": (v != 0).to(torch.uint8).reshape(-1, *v.shape[-2:]).contiguous(), "d0": d.reshape(-1, *d.shape[-2:]).contiguous().clone()}
        n, H, W = out["valid"].shape
        self._speckle_into(out, size, max_diff, poll, self._stereo_scratch(n, H, W))
        keep = out["valid"].view(torch.bool)
        return keep[0] if single else keep

    def stereo_disparity(self, left, right, max_disparity, min_disparity=0, p1=7, p2=60, paths=8, uniqueness=10, lr_max=1, subpixel=True,
                         speckle_size=0, speckle_range=1, poll=8):
        """``stereo.stereo_disparity`` on the device, chunk by chunk under ``stereo_scratch_budget``: dict(disparity fp32, valid bool,
        d0 int32, flags uint8), [n,H,W] for a stack and [H,W] for one pair."""
        D, dmin, p1, p2, paths, uniqueness, lr_max, speckle_size, speckle_range = stereo.check_matcher(
            max_disparity, min_disparity, p1, p2, paths, uniqueness, lr_max, speckle_size, speckle_range)
        gl, gr, single = self._stereo_pair(left, right, "stereo_disparity")
        n, H, W = (int(s) for s in gl.shape)
        if H * W * D >= 1 << 31:
            raise EndoSurfHipError(f"stereo_disparity: {H} x {W} x {D} does not fit int32 indices")
        out = self._stereo_outputs(n, H, W)
        step = self._stereo_chunk(n, H, W, D) if n else 1
        for a in range(0, n, step):
            c = min(step, n - a)
            S = self.empty(c, H, W, D, dtype=torch.uint16)
            self._sgm_into(gl[a:a + c], gr[a:a + c], D, dmin, p1, p2, paths, S)
            part = {k: v[a:a + c] for k, v in out.items()}
            scratch = self._stereo_scratch(c, H, W)
            self._sgm_select_into(S, dmin, uniqueness, lr_max, subpixel, part, scratch)
            if speckle_size > 0:
                self._speckle_into(part, speckle_size, speckle_range, poll, scratch)
        return self._stereo_result(out, single)
