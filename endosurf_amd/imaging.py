"""Frame evaluation, host side: the numpy twins of csrc/metrics.hip.  They are the specification of ``Engine.ssim`` /
``masked_sq_sums`` / ``eval_panels`` and restate the reference's ``cal_ssim`` / ``cal_psnr`` / ``cal_rmse`` /
``gen_rgb`` / ``gen_depth`` / ``gen_normal`` (src/trainer/utils.py:186-246, :340-457) in fp64 on the fp32 inputs.

Images are channel-last, ``[n, H, W, C]``; a mask is per pixel, ``[n, H, W]`` or ``[n, H, W, 1]``, any values, ``None`` = ones."""
from __future__ import annotations

import math

import numpy as np

SSIM_WINDOW = 11
SSIM_SIGMA = 1.5
SSIM_MAX_CHANNELS = 4
PANELS = ("rgb_gt", "rgb_pred", "depth_gt", "depth_pred", "normal_pred")          # the reference's order in an eval sheet


def ssim_window() -> np.ndarray:
    """The reference's 11 x 11 window as the fp32 table it convolves with: a Gaussian (sigma 1.5) made of Python floats, rounded to
    fp32, normalised in fp32, and its outer product rounded to fp32 again -- with the same torch ops, so the 121 entries are the
    reference's bit for bit.  After the last rounding the table is no longer an outer product: evaluate it with 121 taps."""
    import torch
    half = SSIM_WINDOW // 2
    g = torch.tensor([math.exp(-(x - half) ** 2 / float(2 * SSIM_SIGMA ** 2)) for x in range(SSIM_WINDOW)], dtype=torch.float32)
    g = (g / g.sum()).unsqueeze(1)
    return g.mm(g.t()).float().numpy().copy()


def _images(a, b, mask):
    """(a, b [n,H,W,C] fp32, mask [n,H,W] fp32 or None) with the shapes checked."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if a.ndim == 3:
        a, b = a[..., None], (b[..., None] if b.ndim == 3 else b)
    if a.ndim != 4 or a.shape != b.shape:
        raise ValueError(f"images must be two equal [n, H, W, C] stacks (got {a.shape}, {b.shape})")
    if mask is not None:
        mask = np.asarray(mask, np.float32)
        if mask.ndim == 4 and mask.shape[-1] == 1:
            mask = mask[..., 0]
        if mask.shape != a.shape[:3]:
            raise ValueError(f"mask must be [n, H, W] or [n, H, W, 1] of the images (got {mask.shape} for {a.shape})")
    return a, b, mask


def ssim(a, b, mask=None, data_range: float = 1.0, full: bool = False, reverse_taps: bool = False):
    """The reference's ``cal_ssim``: both images times the mask (in fp32, as it does), the five moments a, b, aa, bb, ab under the
    "valid" 11 x 11 window of ``ssim_window()`` accumulated in fp64, map = ((2 mu1 mu2 + C1)(2 s12 + C2)) / ((mu1^2 + mu2^2 + C1)
    (s1 + s2 + C2)) with C1 = (0.01 L)^2, C2 = (0.03 L)^2, L = ``data_range`` (the reference's guess of L from the image's range is
    not reproduced).  Returns (mean of the per-frame means, per-frame means [n] fp64) and with ``full`` the map [n, H-10, W-10, C]
    as a third item.  ``reverse_taps`` accumulates the 121 taps backwards (the size of the summation-order noise)."""
    a, b, mask = _images(a, b, mask)
    n, H, W, C = a.shape
    K = SSIM_WINDOW
    if H < K or W < K:
        raise ValueError(f"ssim needs images of at least {K} x {K} pixels (got {H} x {W})")
    if mask is not None:
        a, b = a * mask[..., None], b * mask[..., None]
    A, B = a.astype(np.float64), b.astype(np.float64)
    win = ssim_window().astype(np.float64)
    Ho, Wo = H - K + 1, W - K + 1
    m = [np.zeros((n, Ho, Wo, C)) for _ in range(5)]
    taps = [(i, j) for i in range(K) for j in range(K)]
    for i, j in (reversed(taps) if reverse_taps else taps):
        pa, pb = A[:, i:i + Ho, j:j + Wo], B[:, i:i + Ho, j:j + Wo]
        w = win[i, j]
        m[0] += w * pa
        m[1] += w * pb
        m[2] += w * (pa * pa)
        m[3] += w * (pb * pb)
        m[4] += w * (pa * pb)
    mu1, mu2 = m[0], m[1]
    s1, s2, s12 = m[2] - mu1 * mu1, m[3] - mu2 * mu2, m[4] - mu1 * mu2
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    smap = ((2.0 * (mu1 * mu2) + c1) * (2.0 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s1 + s2 + c2))
    per_frame = smap.reshape(n, -1).mean(axis=1) if n else np.zeros(0)
    mean = float(per_frame.mean()) if n else float("nan")
    return (mean, per_frame, smap) if full else (mean, per_frame)


def masked_sq_sums(a, b, mask=None):
    """Per frame, in fp64: S = sum (a - b)^2 m over pixels and channels, M = sum m over pixels (the mask once per pixel, not per
    channel).  Returns (S [n], M [n]); everything ``cal_psnr`` / ``cal_rmse`` need."""
    a, b, mask = _images(a, b, mask)
    n = a.shape[0]
    d = a.astype(np.float64) - b.astype(np.float64)
    m = np.ones(a.shape[:3]) if mask is None else mask.astype(np.float64)
    return (d * d * m[..., None]).reshape(n, -1).sum(axis=1), m.reshape(n, -1).sum(axis=1)


def psnr_from_sums(S, M):
    """20 log10(1 / sqrt(S / ((M + 1e-10) 3.0))): the reference's ``cal_psnr`` (the literal 3.0 whatever the channel count); +inf
    for S = 0.  Scalars or arrays."""
    with np.errstate(divide="ignore"):
        r = 20.0 * np.log10(1.0 / np.sqrt(np.asarray(S, np.float64) / ((np.asarray(M, np.float64) + 1e-10) * 3.0)))
    return float(r) if r.ndim == 0 else r


def rmse_from_sums(S, M):
    """sqrt(S / (M + 1e-10)): the reference's ``cal_rmse``."""
    r = np.sqrt(np.asarray(S, np.float64) / (np.asarray(M, np.float64) + 1e-10))
    return float(r) if r.ndim == 0 else r


def psnr(a, b, mask=None) -> float:
    """``cal_psnr`` of whole stacks: one sum over all frames."""
    S, M = masked_sq_sums(a, b, mask)
    return psnr_from_sums(S.sum(), M.sum())


def rmse(a, b, mask=None) -> float:
    """``cal_rmse`` of whole stacks: one sum over all frames."""
    S, M = masked_sq_sums(a, b, mask)
    return rmse_from_sums(S.sum(), M.sum())


def panel_rgb_values(x):
    """256 x in fp64, before clipping and truncation (what decides a byte of ``panel_rgb``)."""
    x = np.asarray(x, np.float32)
    if x.ndim == 3:
        x = np.stack([x, x, x], -1)
    return 256.0 * x.astype(np.float64)


def panel_rgb(x) -> np.ndarray:
    """``gen_rgb``'s picture: uint8(clip(256 x, 0, 255)), truncated (not ``data.to8b``); a grey [n,H,W] stack on three channels."""
    return np.clip(panel_rgb_values(x), 0.0, 255.0).astype(np.uint8)


def panel_depth_values(d, depth_max):
    d = np.asarray(d, np.float32)
    if d.ndim == 3:
        d = d[..., None]
    return 255.0 - np.clip(d.astype(np.float64) / float(depth_max), 0.0, 1.0) * 255.0


def panel_depth(d, depth_max=None) -> np.ndarray:
    """``gen_depth``'s picture (``filter=None``): uint8(255 - clip(d / depth_max, 0, 1) 255) on three equal channels;
    ``depth_max=None``: the largest value of the stack.  d [n,H,W,1] or [n,H,W]."""
    if depth_max is None:
        depth_max = float(np.asarray(d, np.float32).max())
    v = panel_depth_values(d, depth_max).astype(np.uint8)
    return np.concatenate([v, v, v], -1)


def normal_rotations(poses) -> np.ndarray:
    """inv(pose[:, :3, :3]) in fp32, [n,3,3]: what ``gen_normal`` turns world normals into the camera frame with."""
    p = np.asarray(poses, np.float32)
    return np.linalg.inv(p[:, :3, :3]).astype(np.float32)


def panel_normal_values(normals, poses, revert: bool = False):
    nrm = np.asarray(normals, np.float32).astype(np.float64)
    rot = normal_rotations(poses).astype(np.float64)
    if nrm.ndim != 4 or nrm.shape[-1] != 3 or rot.shape[0] != nrm.shape[0]:
        raise ValueError(f"normals must be [n, H, W, 3] with one pose per frame (got {nrm.shape}, {rot.shape[0]} poses)")
    unit = nrm / (np.sqrt((nrm * nrm).sum(-1, keepdims=True)) + 1e-10)
    cam = np.einsum("nij,nhwj->nhwi", rot, unit)
    return -cam if revert else cam


def panel_normal(normals, poses, revert: bool = False):
    """``gen_normal`` (``filter=None``): n / (|n| + 1e-10), rotated by inv(pose[:3,:3]) of its frame, negated with ``revert``.
    Returns (the float picture [n,H,W,3] fp32, uint8(clip(128 n + 128, 0, 255)))."""
    cam = panel_normal_values(normals, poses, revert)
    return cam.astype(np.float32), np.clip(128.0 * cam + 128.0, 0.0, 255.0).astype(np.uint8)


def sheet(panels) -> np.ndarray:
    """[n, H, 5 W, 3]: the five panels of ``PANELS`` side by side (the reference's eval picture without its text labels)."""
    return np.concatenate([panels[k] for k in PANELS], axis=2)
