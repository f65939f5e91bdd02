#!/usr/bin/env python3
"""Golden vectors for the frame evaluation: the REFERENCE's own cal_ssim / cal_psnr / cal_rmse / gen_rgb / gen_depth /
gen_normal (src/trainer/utils.py), run on the CPU on small synthetic frames, next to the fp64 results of the numpy twins in
endosurf_amd/imaging.py.  The reference module is imported with do-nothing stand-ins for the visualisation and logging packages it
names at import time; none of its text is copied, only the numbers it computes are stored.

    ENDOSURF_REFERENCE=/path/to/endosurf python tools/make_golden_eval.py        # writes tests/golden/eval_small.npz"""
import os
import sys
import types

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np
import torch

from endosurf_amd import imaging

STUBS = ("wandb", "cv2", "kornia", "lpips", "open3d", "imageio", "imageio.v2", "mcubes", "trimesh", "torch.utils.tensorboard")
# name: (frames, H, W, noise, mask kind, has depth and normals)
CASES = {
    "noise002_half": (2, 40, 56, 0.02, 0.5, False),
    "noise01_most": (2, 43, 75, 0.1, 0.8, True),            # neither side a multiple of 32
    "noise03_full": (1, 56, 88, 0.3, None, False),
    "noise01_soft": (1, 37, 50, 0.1, "soft", True),
    "equal_half": (1, 32, 45, 0.0, 0.5, False),             # SSIM exactly 1
    "single_entry": (1, 11, 11, 0.1, None, True),           # one map entry
}


class _Nothing:
    """What a stubbed package hands out: callable, chainable, and ``.to()`` returns itself."""

    def __call__(self, *a, **k):
        return self

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return self

    def to(self, *a, **k):
        return self


def import_reference_utils(root):
    nothing = _Nothing()

    def module_getattr(attr):
        if attr.startswith("__"):
            raise AttributeError(attr)
        return nothing

    for name in STUBS:
        m = types.ModuleType(name)
        m.__getattr__ = module_getattr
        m.__path__ = []
        sys.modules[name] = m
    sys.modules["imageio"].v2 = sys.modules["imageio.v2"]
    os.chdir(root)
    sys.path.insert(0, root)
    import src.trainer.utils as U
    return U


def smooth(rng, n, h, w, c, waves=4):
    """A smooth random image stack in about [0, 1]: a few random low-frequency cosines per channel."""
    yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    out = np.zeros((n, h, w, c))
    for k in range(waves):
        fy, fx, ph = rng.uniform(0.5, 4.0, (n, 1, 1, c)), rng.uniform(0.5, 4.0, (n, 1, 1, c)), rng.uniform(0, 6.28, (n, 1, 1, c))
        out += np.cos(6.28 * (fy * yy[None, ..., None] + fx * xx[None, ..., None]) + ph) / waves
    return 0.5 + 0.45 * out


def make_mask(rng, n, h, w, kind):
    if kind is None:
        return np.ones((n, h, w, 1), np.float32)
    field = smooth(rng, n, h, w, 1, waves=3)
    if kind == "soft":          # not 0 / 1: weights between and a little beyond
        return (1.4 * (field - 0.5) / 0.45 * 0.5 + 0.55).clip(-0.1, 1.2).astype(np.float32)
    cut = np.quantile(field, 1.0 - kind)
    return (field > cut).astype(np.float32)


def rigid(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    m = np.eye(4, dtype=np.float32)
    m[:3, :3] = q
    m[:3, 3] = rng.normal(size=3) * 0.3
    return m


def main():
    root = os.environ.get("ENDOSURF_REFERENCE") or (sys.argv[1] if len(sys.argv) > 1 else None)
    if not root or not os.path.isdir(root):
        raise SystemExit("set ENDOSURF_REFERENCE (or pass the path) to a checkout of the reference")
    U = import_reference_utils(os.path.abspath(root))
    rng = np.random.default_rng(2026)
    out = {"window": U.ssim.create_window(11, 1)[0, 0].numpy().astype(np.float32), "names": np.array(sorted(CASES))}
    worst = 0.0
    for name in sorted(CASES):
        n, h, w, noise, kind, has_geometry = CASES[name]
        a = smooth(rng, n, h, w, 3).astype(np.float32)
        b = (a + noise * rng.normal(size=a.shape)).astype(np.float32)
        cmask = make_mask(rng, n, h, w, kind)
        d = {"color_gt": a, "color": b, "color_mask": cmask}
        with torch.no_grad():
            d["ref_ssim"] = np.float32(U.cal_ssim(a, b, cmask, device="cpu").item())
            am, bm = torch.from_numpy(a * cmask).permute(0, 3, 1, 2), torch.from_numpy(b * cmask).permute(0, 3, 1, 2)
            d["ref_ssim_per_frame"] = U.ssim(am, bm, size_average=False).numpy().astype(np.float32)
        d["ref_psnr"] = np.float64(U.cal_psnr(a, b, cmask))
        d["ref_rmse_color"] = np.float64(U.cal_rmse(a, b, cmask))
        mean, per_frame = imaging.ssim(a, b, cmask)
        d["twin_ssim"], d["twin_ssim_per_frame"] = np.float64(mean), per_frame
        d["twin_psnr"], d["twin_rmse_color"] = np.float64(imaging.psnr(a, b, cmask)), np.float64(imaging.rmse(a, b, cmask))
        worst = max(worst, abs(float(d["ref_ssim"]) - mean))
        if has_geometry:
            depth_max = 1.5
            dgt = (0.2 + 1.6 * smooth(rng, n, h, w, 1)).astype(np.float32)          # some of it beyond depth_max
            dpr = (dgt + 0.05 * rng.normal(size=dgt.shape)).astype(np.float32)
            dmask = make_mask(rng, n, h, w, 0.7)
            nrm = (rng.normal(size=(n, h, w, 3)) * rng.uniform(0.1, 3.0, size=(n, h, w, 1))).astype(np.float32)
            nrm[:, ::5, ::7] = 0.0          # rays that hit nothing: exact zeros
            poses = np.stack([rigid(rng) for _ in range(n)])
            d.update(depth_gt=dgt, depth=dpr, mask=dmask, normal=nrm, poses=poses, depth_max=np.float64(depth_max))
            d["ref_rmse_depth"] = np.float64(U.cal_rmse(dgt, dpr, dmask))
            d["twin_rmse_depth"] = np.float64(imaging.rmse(dgt, dpr, dmask))
            d["ref_panel_rgb_gt"] = U.gen_rgb(a, n, w, h)[1]
            d["ref_panel_rgb_pred"] = U.gen_rgb(b, n, w, h)[1]
            d["ref_panel_depth_gt"] = U.gen_depth(dgt, n, w, h, depth_max)[1][..., :1]          # (three equal channels: one is kept)
            d["ref_panel_depth_pred"] = U.gen_depth(dpr, n, w, h, depth_max)[1][..., :1]
            d["ref_panel_depth_pred_automax"] = U.gen_depth(dpr, n, w, h, None)[1][..., :1]
            for rev in (False, True):
                f, show = U.gen_normal(nrm.copy(), torch.from_numpy(poses), n, w, h, revert=rev)
                d["ref_normal" + ("_revert" if rev else "")] = f.astype(np.float32)
                d["ref_panel_normal" + ("_revert" if rev else "")] = show
        for k, v in d.items():
            out[f"{name}/{k}"] = v
        print(f"{name}: reference ssim {float(d['ref_ssim']):.9f}, twin {mean:.12f}, |diff| {abs(float(d['ref_ssim']) - mean):.2e}; "
              f"psnr {float(d['ref_psnr']):.6f} / {float(d['twin_psnr']):.6f}")
    out["ssim_ref_fp32_err"] = np.float64(worst)
    path = os.path.join(REPO, "tests", "golden", "eval_small.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(f"ssim_ref_fp32_err = {worst:.3e}; wrote {path}: {size / 1024:.1f} KiB")
    assert size < 1000000, "the golden file must stay below the limit for a committed file"


if __name__ == "__main__":
    main()
