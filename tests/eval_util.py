"""Helpers shared by tests/test_eval_host.py and tests/test_gpu_eval.py: the golden file of the frame evaluation
(tests/golden/eval_small.npz, written by tools/make_golden_eval.py from the reference's own functions) and the rules a result is held to."""
import os

import numpy as np

from endosurf_amd import imaging

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_small.npz")
_G = None


def golden():
    global _G
    if _G is None:
        _G = dict(np.load(GOLDEN))
    return _G


def names(geometry=None):
    """The cases of the golden file; ``geometry=True``: those with depth, normals and panels."""
    g = golden()
    return [str(n) for n in g["names"] if geometry is None or (f"{n}/normal" in g) == geometry]


def case(name):
    g = golden()
    return {k.split("/", 1)[1]: v for k, v in g.items() if k.startswith(name + "/")}


def ssim_gate() -> float:
    """How far an SSIM mean may lie from the reference's stored fp32 value: 3 x the reference's own fp32-vs-fp64 error (the project's
    rule), floored at four fp32 steps at 1.0 because the reference returns one fp32 number."""
    return max(3.0 * float(golden()["ssim_ref_fp32_err"]), 2.0 ** -22)


def assert_bytes(got, ref, values, what):
    """The byte rule of the panels: a byte equals the reference's, or differs by 1 where the fp64 value before truncation lies within
    1e-4 of an integer.  No share of pixels is exempt otherwise.  Returns the number of bytes that used the exemption."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == np.uint8 and got.shape == ref.shape == values.shape, (what, got.dtype, got.shape, ref.shape, values.shape)
    diff = np.abs(got.astype(np.int16) - ref.astype(np.int16))
    near = np.abs(values - np.rint(values)) <= 1e-4
    bad = (diff > 1) | ((diff == 1) & ~near)
    assert not bad.any(), f"{what}: {int(bad.sum())} bytes differ from the reference's outside the rule (largest step {int(diff.max())})"
    return int((diff == 1).sum())


def panel_values(c):
    """{panel: the fp64 values before clipping and truncation} of a geometry case (what decides its bytes)."""
    three = lambda v: np.concatenate([v, v, v], -1)
    return {"rgb_gt": imaging.panel_rgb_values(c["color_gt"]), "rgb_pred": imaging.panel_rgb_values(c["color"]),
            "depth_gt": three(imaging.panel_depth_values(c["depth_gt"], float(c["depth_max"]))),
            "depth_pred": three(imaging.panel_depth_values(c["depth"], float(c["depth_max"]))),
            "normal_pred": 128.0 * imaging.panel_normal_values(c["normal"], c["poses"]) + 128.0}


def panel_refs(c):
    """{panel: the reference's bytes [n,H,W,3]} of a geometry case."""
    three = lambda v: np.concatenate([v, v, v], -1)
    return {"rgb_gt": c["ref_panel_rgb_gt"], "rgb_pred": c["ref_panel_rgb_pred"], "depth_gt": three(c["ref_panel_depth_gt"]),
            "depth_pred": three(c["ref_panel_depth_pred"]), "normal_pred": c["ref_panel_normal"]}


def random_images(seed, n, h, w, c, noise=0.1):
    """Two fp32 stacks and a blob-free random mask with some exact zeros: inputs for twin-against-device comparisons."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(size=(n, h, w, c)).astype(np.float32)
    b = (a + noise * rng.normal(size=a.shape)).astype(np.float32)
    m = (rng.uniform(size=(n, h, w, 1)) * (rng.uniform(size=(n, h, w, 1)) > 0.2)).astype(np.float32)
    return a, b, m
