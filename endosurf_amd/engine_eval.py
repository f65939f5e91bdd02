"""The frame-evaluation methods of ``engine.Engine`` (a mixin; csrc/metrics.hip): SSIM, masked squared sums, the eval picture's panels."""
from __future__ import annotations

import torch

from ._lib import EndoSurfHipError, check, ptr
from .imaging import PANELS, SSIM_MAX_CHANNELS, SSIM_WINDOW, normal_rotations, ssim_window


class EvalMixin:
    def _eval_stack(self, name, t, channels=None, like=None):
        """``t`` as the evaluation kernels read it: an fp32 [n,H,W,C] stack on this device, contiguous (a strided view is copied, never
        read through its strides).  Raises for another dtype, device or shape; launches nothing."""
        if not torch.is_tensor(t) or t.device != self.device or t.dtype != torch.float32:
            raise EndoSurfHipError(f"{name} must be an fp32 tensor on {self.device} (got "
                                        f"{(t.dtype, t.device) if torch.is_tensor(t) else type(t).__name__})")
        if t.dim() == 3 and channels in (None, 1):
            t = t.unsqueeze(-1)
        if t.dim() != 4 or (channels is not None and t.shape[-1] != channels) or (like is not None and t.shape != like.shape):
            want = tuple(like.shape) if like is not None else f"[n, H, W, {channels or 'C'}]"
            raise EndoSurfHipError(f"{name} must be {want} (got {tuple(t.shape)})")
        return t.detach().contiguous()

    def _eval_mask(self, mask, like):
        """A per-pixel mask [n,H,W] or [n,H,W,1] of the stack ``like`` as a contiguous fp32 [n,H,W]; None stays None (= ones)."""
        if mask is None:
            return None
        if not torch.is_tensor(mask) or mask.device != self.device or mask.dtype != torch.float32:
            raise EndoSurfHipError(f"mask must be an fp32 tensor on {self.device} or None")
        if mask.dim() == 4 and mask.shape[-1] == 1:
            mask = mask[..., 0]
        if mask.shape != like.shape[:3]:
            raise EndoSurfHipError(f"mask must be [n, H, W] or [n, H, W, 1] of the images (got {tuple(mask.shape)} for {tuple(like.shape)})")
        return mask.detach().contiguous()

    def _eval_out(self, out, numel):
        if out is None:
            return self.empty(numel, dtype=torch.float64)
        if out.dtype != torch.float64 or out.device != self.device or out.dim() != 1 or out.numel() != numel or not out.is_contiguous():
            raise EndoSurfHipError(f"out must be a contiguous fp64 [{numel}] on {self.device}")
        return out

    def _eval_scratch(self, scratch, fn_name, *dims):
        nbytes = self._scratch_bytes(fn_name, *dims)
        if scratch is None:
            return self.empty(max(nbytes, 8), dtype=torch.uint8)
        if scratch.device != self.device or not scratch.is_contiguous() or scratch.numel() * scratch.element_size() < nbytes:
            raise EndoSurfHipError(f"scratch must be a contiguous buffer of at least {nbytes} bytes on {self.device}")
        return scratch

    def ssim(self, a, b, mask=None, data_range: float = 1.0, full: bool = False, out=None, scratch=None):
        """The reference's ``cal_ssim`` of two fp32 stacks [n,H,W,C] (C <= 4) on this device (``imaging.ssim`` is the numpy twin and the
        specification): both times the per-pixel ``mask``, "valid" 11 x 11 window from the reference's 121-entry fp32 table, moments
        and map in fp64, ``data_range`` = L.  Returns dict(``mean`` [] fp64, ``per_frame`` [n] fp64, and with ``full`` ``map``
        [n,H-10,W-10,C] fp64), all on the device (no read-back); ``mean`` and ``per_frame`` are views of ``out`` [n+1] when one is given.
        Bit-identical from call to call, whatever ``scratch`` holds."""
        a = self._eval_stack("a", a)
        b = self._eval_stack("b", b, like=a)
        m = self._eval_mask(mask, a)
        n, H, W, Cn = (int(v) for v in a.shape)
        if H < SSIM_WINDOW or W < SSIM_WINDOW or not 1 <= Cn <= SSIM_MAX_CHANNELS:
            raise EndoSurfHipError(f"ssim needs images of at least {SSIM_WINDOW} x {SSIM_WINDOW} pixels and 1..{SSIM_MAX_CHANNELS} channels "
                                        f"(got {H} x {W} x {Cn})")
        if not (float(data_range) > 0.0 and float(data_range) < float("inf")):
            raise EndoSurfHipError(f"ssim: data_range must be finite and positive (got {data_range!r})")
        if self._ssim_window is None:
            self._ssim_window = torch.from_numpy(ssim_window()).to(self.device).contiguous()
        out = self._eval_out(out, n + 1)
        scratch = self._eval_scratch(scratch, "es_ssim_scratch_bytes", n, H, W)
        smap = self.empty(n, H - SSIM_WINDOW + 1, W - SSIM_WINDOW + 1, Cn, dtype=torch.float64) if full else None
        check(self.lib.es_ssim(ptr(a), ptr(b), ptr(m), ptr(self._ssim_window), n, H, W, Cn, float(data_range), ptr(scratch), ptr(out), ptr(smap),
                               self.st()), "es_ssim")
        if n == 0:
            out.fill_(float("nan"))
        res = {"mean": out[n], "per_frame": out[:n]}
        if full:
            res["map"] = smap
        return res

    def masked_sq_sums(self, a, b, mask=None, out=None, scratch=None):
        """Per frame of two fp32 stacks [n,H,W,C] on this device, in fp64: S = sum (a - b)^2 m, M = sum m (the per-pixel ``mask`` once
        per pixel) -- everything ``cal_psnr`` / ``cal_rmse`` need (``imaging.masked_sq_sums`` is the twin).  Returns dict(``S`` [n],
        ``M`` [n], ``S_total`` [], ``M_total`` []) of device fp64, views of ``out`` [2n+2] when one is given.  No read-back."""
        a = self._eval_stack("a", a)
        b = self._eval_stack("b", b, like=a)
        m = self._eval_mask(mask, a)
        n, H, W, Cn = (int(v) for v in a.shape)
        if H < 1 or W < 1 or not 1 <= Cn <= 16:
            raise EndoSurfHipError(f"masked_sq_sums needs non-empty images of 1..16 channels (got {H} x {W} x {Cn})")
        out = self._eval_out(out, 2 * n + 2)
        scratch = self._eval_scratch(scratch, "es_sq_sums_scratch_bytes", n, H, W)
        check(self.lib.es_masked_sq_sums(ptr(a), ptr(b), ptr(m), n, H, W, Cn, ptr(scratch), ptr(out), self.st()), "es_masked_sq_sums")
        if n == 0:
            out.zero_()
        return {"S": out[:n], "M": out[n:2 * n], "S_total": out[2 * n], "M_total": out[2 * n + 1]}

    def _panel_target(self, x, out, col):
        """(picture, pitch in bytes, column) a panel of the stack ``x`` [n,H,W,*] is written to: a fresh [n,H,W,3] or the caller's
        contiguous uint8 picture [n,H,W_total,3] from column ``col`` on."""
        n, H, W = (int(v) for v in x.shape[:3])
        if out is None:
            return self.empty(n, H, W, 3, dtype=torch.uint8), 3 * W, 0
        if out.dtype != torch.uint8 or out.device != self.device or out.dim() != 4 or not out.is_contiguous() or out.shape[0] != n \
                or out.shape[1] != H or out.shape[3] != 3 or int(col) < 0 or int(col) + W > out.shape[2]:
            raise EndoSurfHipError(f"a panel of {n} x {H} x {W} at column {col} needs a contiguous uint8 [{n}, {H}, >= {int(col) + W}, 3] "
                                        f"picture on {self.device}")
        return out, 3 * int(out.shape[2]), int(col)

    def panel_rgb(self, x, out=None, col: int = 0):
        """``gen_rgb``'s picture of an fp32 stack [n,H,W,3] (or grey [n,H,W] / [n,H,W,1]): uint8(clip(256 x, 0, 255)), as a new
        [n,H,W,3] or into the columns ``col``.. of the picture ``out`` [n,H,W_total,3] (returned).  Twin: ``imaging.panel_rgb``."""
        x = self._eval_stack("an rgb panel's image", x)
        if x.shape[-1] not in (1, 3):
            raise EndoSurfHipError(f"an rgb panel takes 1 or 3 channels (got {x.shape[-1]})")
        pic, pitch, col = self._panel_target(x, out, col)
        n, H, W, Cn = (int(v) for v in x.shape)
        check(self.lib.es_eval_panel_rgb(ptr(x), n, H, W, Cn, ptr(pic), pitch, col, self.st()), "es_eval_panel_rgb")
        return pic

    def panel_depth(self, d, depth_max=None, out=None, col: int = 0):
        """``gen_depth``'s picture of an fp32 depth stack [n,H,W,1] (or [n,H,W]): uint8(255 - clip(d / depth_max, 0, 1) 255) on three
        channels; ``depth_max=None``: the largest value of the stack (one reduction and read-back).  Twin: ``imaging.panel_depth``."""
        d = self._eval_stack("a depth panel's image", d, channels=1)
        if depth_max is None:
            depth_max = float(d.max()) if d.numel() else 1.0
        if not (float(depth_max) > 0.0 and float(depth_max) < float("inf")):
            raise EndoSurfHipError(f"panel_depth: depth_max must be finite and positive (got {depth_max!r})")
        pic, pitch, col = self._panel_target(d, out, col)
        n, H, W, _ = (int(v) for v in d.shape)
        check(self.lib.es_eval_panel_depth(ptr(d), n, H, W, float(depth_max), ptr(pic), pitch, col, self.st()), "es_eval_panel_depth")
        return pic

    def panel_normal(self, normals, poses, revert: bool = False, out=None, col: int = 0):
        """``gen_normal`` of an fp32 stack of world normals [n,H,W,3] and the camera-to-world ``poses`` [n,4,4] of its frames:
        n / (|n| + 1e-10) turned into each camera's frame by inv(pose[:3,:3]) (inverted in fp32 on the host: 9 floats per frame go to
        the kernel), negated with ``revert``.  Returns (the float picture [n,H,W,3] fp32, uint8(clip(128 n + 128, 0, 255)) as in
        ``panel_rgb``).  Twin: ``imaging.panel_normal``."""
        x = self._eval_stack("a normal panel's image", normals, channels=3)
        n, H, W, _ = (int(v) for v in x.shape)
        p = poses.detach().cpu().numpy() if torch.is_tensor(poses) else poses
        rot = normal_rotations(p)
        if rot.shape != (n, 3, 3):
            raise EndoSurfHipError(f"panel_normal needs one [4,4] pose per frame (got {rot.shape[0]} for {n} frames)")
        rot_d = torch.from_numpy(rot.reshape(n, 9).copy()).to(self.device)
        pic, pitch, col = self._panel_target(x, out, col)
        out_f = self.empty(n, H, W, 3)
        check(self.lib.es_eval_panel_normal(ptr(x), ptr(rot_d), n, H, W, int(bool(revert)), ptr(out_f), ptr(pic), pitch, col, self.st()),
              "es_eval_panel_normal")
        return out_f, pic

    def eval_panels(self, color_gt, color, depth_gt, depth, normal, poses, depth_max=None, revert: bool = False):
        """The five panels of the reference's eval picture (``imaging.PANELS``: rgb_gt, rgb_pred, depth_gt, depth_pred, normal_pred),
        each written by its kernel straight into its columns of one ``sheet`` [n,H,5W,3] uint8 (no concatenation).  Returns
        dict(``sheet``, ``panels`` = {name: the [n,H,W,3] view of its columns}, ``normal`` = the float camera-frame normals)."""
        color = self._eval_stack("color", color, channels=3)
        n, H, W, _ = (int(v) for v in color.shape)
        sheet = self.empty(n, H, len(PANELS) * W, 3, dtype=torch.uint8)
        stacks = {"rgb_gt": self._eval_stack("color_gt", color_gt, like=color), "rgb_pred": color,
                  "depth_gt": self._eval_stack("depth_gt", depth_gt, channels=1), "depth_pred": self._eval_stack("depth", depth, channels=1),
                  "normal_pred": self._eval_stack("normal", normal, like=color)}
        for k in ("depth_gt", "depth_pred"):
            if stacks[k].shape[:3] != color.shape[:3]:
                raise EndoSurfHipError(f"{k} must be [{n}, {H}, {W}, 1] (got {tuple(stacks[k].shape)})")
        normal_f = None
        for i, name in enumerate(PANELS):
            if name.startswith("rgb"):
                self.panel_rgb(stacks[name], out=sheet, col=i * W)
            elif name.startswith("depth"):
                self.panel_depth(stacks[name], depth_max, out=sheet, col=i * W)
            else:
                normal_f, _ = self.panel_normal(stacks[name], poses, revert, out=sheet, col=i * W)
        return {"sheet": sheet, "panels": {name: sheet[:, :, i * W:(i + 1) * W] for i, name in enumerate(PANELS)}, "normal": normal_f}
