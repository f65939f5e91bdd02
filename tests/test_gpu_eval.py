"""Frame evaluation on the device (csrc/metrics.hip: Engine.ssim / masked_sq_sums / panel_* / eval_panels,
EndoSurfRenderer.evaluate_frames) against the fp64 numpy twins in endosurf_amd.imaging, which tests/test_eval_host.py holds to the
reference's own numbers, and against those numbers themselves (tests/golden/eval_small.npz)."""
import ctypes as C

import numpy as np
import pytest
import torch

from endosurf_amd import data as D
from endosurf_amd import imaging as I
from eval_util import assert_bytes, case, names, panel_refs, panel_values, random_images, ssim_gate

pytestmark = pytest.mark.gpu

SHAPES = [(1, 11, 11, 3), (2, 43, 75, 3), (3, 64, 96, 1), (1, 512, 640, 3)]


@pytest.fixture(scope="module")
def eng():
    from endosurf_amd.engine import Engine
    return Engine("cuda")


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ssim_against_twin(eng, a, b, m, what):
    """Every map entry within 1e-10 of the twin's, the per-frame means and the mean within 1e-12 relative."""
    mean, per_frame, smap = I.ssim(a, b, m, full=True)
    got = eng.ssim(dev(a), dev(b), dev(m), full=True)
    assert got["map"].dtype == torch.float64 and tuple(got["map"].shape) == smap.shape and got["per_frame"].dtype == torch.float64
    worst = float(np.abs(got["map"].cpu().numpy() - smap).max())
    pf = got["per_frame"].cpu().numpy()
    rel_pf = float(np.abs(pf / per_frame - 1.0).max())
    rel_mean = abs(float(got["mean"]) / mean - 1.0)
    print(f"EVAL_MEASURED ssim {what}: map max |dev - twin| {worst:.2e}, per-frame rel {rel_pf:.2e}, mean rel {rel_mean:.2e} (mean {mean:.9f})")
    assert worst <= 1e-10 and rel_pf <= 1e-12 and rel_mean <= 1e-12
    return got


@pytest.mark.parametrize("name", names())
def test_ssim_on_the_golden_cases(eng, name):
    c = case(name)
    got = ssim_against_twin(eng, c["color_gt"], c["color"], c["color_mask"], name)
    assert abs(float(got["mean"]) - float(c["ref_ssim"])) <= ssim_gate()
    assert np.abs(got["per_frame"].cpu().numpy() - c["ref_ssim_per_frame"]).max() <= ssim_gate()
    assert D.cal_ssim(dev(c["color_gt"]), dev(c["color"]), dev(c["color_mask"]), engine=eng) == float(got["mean"])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("masked", [True, False])
def test_ssim_equals_the_twin(eng, shape, masked):
    a, b, m = random_images(sum(shape), *shape)
    ssim_against_twin(eng, a, b, m if masked else None, f"{shape} masked={masked}")


def test_ssim_is_bit_identical_and_ignores_what_the_scratch_held(eng):
    a, b, m = (dev(x) for x in random_images(3, 2, 75, 140, 3))
    first = eng.ssim(a, b, m, full=True)
    again = eng.ssim(a, b, m, full=True)
    for k in ("mean", "per_frame", "map"):
        assert torch.equal(first[k], again[k]), k
    nbytes = int(eng.lib.es_ssim_scratch_bytes(2, 75, 140))
    assert nbytes == 8 * 2 * 3 * 5          # one fp64 per frame and 32 x 32 tile of the 65 x 130 map
    scratch = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")          # NaN bytes
    out = torch.full((3,), float("nan"), dtype=torch.float64, device="cuda")
    dirty = eng.ssim(a, b, m, out=out, scratch=scratch)
    assert torch.equal(dirty["per_frame"], first["per_frame"]) and torch.equal(dirty["mean"], first["mean"])          # full=False, same bits
    assert dirty["per_frame"].data_ptr() == out.data_ptr() and bool(torch.isfinite(out).all())
    # a strided view is copied, never read through its strides
    wide = torch.rand(2, 75, 140, 6, device="cuda")
    view = wide[..., ::2]
    assert not view.is_contiguous()
    assert torch.equal(eng.ssim(view, b, m)["mean"], eng.ssim(view.contiguous(), b, m)["mean"])
    assert torch.equal(eng.ssim(a, b, m[..., 0])["mean"], first["mean"])          # [n,H,W] mask
    q1, q2 = eng.masked_sq_sums(a, b, m), eng.masked_sq_sums(a, b, m, scratch=torch.full((1 << 16,), 0xFF, dtype=torch.uint8, device="cuda"))
    assert all(torch.equal(q1[k], q2[k]) for k in q1)


@pytest.mark.parametrize("shape", SHAPES + [(2, 5, 7, 3), (1, 100, 333, 1)], ids=lambda s: "x".join(map(str, s)))
def test_masked_sq_sums_equal_fp64_numpy(eng, shape):
    a, b, m = random_images(7 + sum(shape), *shape)
    forms = {"[n,H,W,1]": m, "[n,H,W]": m[..., 0], "None": None, "zero": np.zeros_like(m)}
    for what, mask in forms.items():
        d = a.astype(np.float64) - b.astype(np.float64)
        m64 = np.ones(shape[:3]) if mask is None else mask.astype(np.float64).reshape(shape[:3])
        S = (d * d * m64[..., None]).reshape(shape[0], -1).sum(1)
        M = m64.reshape(shape[0], -1).sum(1)
        got = eng.masked_sq_sums(dev(a), dev(b), dev(mask))
        gS, gM = got["S"].cpu().numpy(), got["M"].cpu().numpy()
        rel = lambda x, y: float(np.abs(x - y).max() / max(np.abs(y).max(), 1e-300)) if np.abs(y).max() > 0 else float(np.abs(x).max())
        print(f"EVAL_MEASURED sq sums {shape} mask {what}: S rel {rel(gS, S):.2e} M rel {rel(gM, M):.2e}")
        assert np.all(np.abs(gS - S) <= 1e-12 * np.abs(S)) and np.all(np.abs(gM - M) <= 1e-12 * np.abs(M))
        assert abs(float(got["S_total"]) - S.sum()) <= 1e-12 * abs(S.sum()) and abs(float(got["M_total"]) - M.sum()) <= 1e-12 * abs(M.sum())
        tS, tM = I.masked_sq_sums(a, b, mask)
        assert np.all(np.abs(gS - tS) <= 1e-12 * np.abs(tS)) and np.all(np.abs(gM - tM) <= 1e-12 * np.abs(tM))
        psnr, rmse = I.psnr_from_sums(float(got["S_total"]), float(got["M_total"])), I.rmse_from_sums(float(got["S_total"]), float(got["M_total"]))
        assert not np.isnan(psnr) and not np.isnan(rmse)
        if what == "zero":
            assert rmse == 0.0 and psnr == float("inf")
        else:
            full = np.broadcast_to(m64[..., None], a.shape[:3] + (1,))
            assert psnr == pytest.approx(D.cal_psnr(a.astype(np.float64), b.astype(np.float64), full), rel=1e-9)
            assert D.cal_psnr_device(dev(a), dev(b), dev(mask), engine=eng) == psnr and D.cal_rmse_device(dev(a), dev(b), dev(mask), engine=eng) == rmse


@pytest.mark.parametrize("name", names())
def test_psnr_rmse_on_the_golden_cases(eng, name):
    c = case(name)
    q = eng.masked_sq_sums(dev(c["color_gt"]), dev(c["color"]), dev(c["color_mask"]))
    psnr, rmse = I.psnr_from_sums(float(q["S_total"]), float(q["M_total"])), I.rmse_from_sums(float(q["S_total"]), float(q["M_total"]))
    ref_p, ref_r = float(c["ref_psnr"]), float(c["ref_rmse_color"])
    assert (np.isinf(ref_p) and psnr == ref_p) or abs(psnr - ref_p) <= 1e-5 * abs(ref_p)
    assert abs(rmse - ref_r) <= 1e-5 * abs(ref_r)
    if "depth" in c:
        qd = eng.masked_sq_sums(dev(c["depth_gt"]), dev(c["depth"]), dev(c["mask"]))
        assert abs(I.rmse_from_sums(float(qd["S_total"]), float(qd["M_total"])) - float(c["ref_rmse_depth"])) <= 1e-5 * float(c["ref_rmse_depth"])


@pytest.mark.parametrize("name", names(geometry=True))
def test_panels_against_the_reference(eng, name):
    c = case(name)
    out = eng.eval_panels(dev(c["color_gt"]), dev(c["color"]), dev(c["depth_gt"]), dev(c["depth"]), dev(c["normal"]), dev(c["poses"]),
                          float(c["depth_max"]))
    n, h, w, _ = c["color"].shape
    sheet = out["sheet"].cpu().numpy()
    assert sheet.shape == (n, h, 5 * w, 3) and sheet.dtype == np.uint8
    vals, refs = panel_values(c), panel_refs(c)
    for i, k in enumerate(I.PANELS):
        got = out["panels"][k].cpu().numpy()
        assert np.array_equal(got, sheet[:, :, i * w:(i + 1) * w])
        print(f"EVAL_MEASURED device panel {k} {name}: {assert_bytes(got, refs[k], vals[k], k)} of {got.size} bytes differ by one")
    nf = out["normal"].cpu().numpy()
    assert nf.dtype == np.float32 and np.abs(nf.astype(np.float64) - c["ref_normal"]).max() <= 1e-6
    assert np.abs(nf - I.panel_normal(c["normal"], c["poses"])[0]).max() <= 1e-6
    rev_f, rev_b = eng.panel_normal(dev(c["normal"]), c["poses"], revert=True)
    assert np.abs(rev_f.cpu().numpy().astype(np.float64) - c["ref_normal_revert"]).max() <= 1e-6
    assert_bytes(rev_b.cpu().numpy(), c["ref_panel_normal_revert"], 128.0 * I.panel_normal_values(c["normal"], c["poses"], True) + 128.0, "reverted")
    auto = eng.panel_depth(dev(c["depth"]), None).cpu().numpy()
    assert_bytes(auto, np.concatenate([c["ref_panel_depth_pred_automax"]] * 3, -1),
                 np.concatenate([I.panel_depth_values(c["depth"], float(c["depth"].max()))] * 3, -1), "depth with its own maximum")
    grey = eng.panel_rgb(dev(c["color"][..., 0])).cpu().numpy()
    assert np.array_equal(grey, I.panel_rgb(c["color"][..., 0]))


def test_panels_in_a_sheet_touch_only_their_columns(eng):
    c = case(names(geometry=True)[0])
    n, h, w, _ = c["color"].shape
    total, col = 2 * w + 9, w + 4
    for paint in ("rgb", "depth", "normal"):
        sheet = torch.full((n, h, total, 3), 0xA5, dtype=torch.uint8, device="cuda")
        if paint == "rgb":
            alone = eng.panel_rgb(dev(c["color"]))
            eng.panel_rgb(dev(c["color"]), out=sheet, col=col)
        elif paint == "depth":
            alone = eng.panel_depth(dev(c["depth"]), 1.5)
            eng.panel_depth(dev(c["depth"]), 1.5, out=sheet, col=col)
        else:
            alone = eng.panel_normal(dev(c["normal"]), c["poses"])[1]
            eng.panel_normal(dev(c["normal"]), c["poses"], out=sheet, col=col)
        s = sheet.cpu().numpy()
        assert np.array_equal(s[:, :, col:col + w], alone.cpu().numpy()), paint
        assert (s[:, :, :col] == 0xA5).all() and (s[:, :, col + w:] == 0xA5).all(), paint
        assert not (alone.cpu().numpy() == 0xA5).all()


def test_bad_arguments_raise_before_any_launch(eng):
    from endosurf_amd._lib import EndoSurfHipError
    a = torch.rand(2, 12, 16, 3, device="cuda")
    five = torch.rand(1, 12, 12, 5, device="cuda")
    bad = [lambda: eng.ssim(a[:, :10], a[:, :10]), lambda: eng.ssim(a[:, :, :10], a[:, :, :10]), lambda: eng.ssim(a, a[:, :11]),
           lambda: eng.ssim(a.double(), a.double()), lambda: eng.ssim(a, a, torch.ones(2, 12, 15, device="cuda")),
           lambda: eng.ssim(a.cpu(), a.cpu()), lambda: eng.ssim(a, a, data_range=0.0), lambda: eng.ssim(five, five),
           lambda: eng.masked_sq_sums(a, a.half()), lambda: eng.masked_sq_sums(a, a[:1]), lambda: eng.masked_sq_sums(a, a, torch.ones(2, 12, 16, 2, device="cuda")),
           lambda: eng.panel_rgb(a[..., :2]), lambda: eng.panel_rgb((a * 255).to(torch.uint8)), lambda: eng.panel_depth(a[..., :1], depth_max=0.0),
           lambda: eng.panel_depth(a), lambda: eng.panel_normal(a, np.tile(np.eye(4, dtype=np.float32), (3, 1, 1))),
           lambda: eng.panel_rgb(a, out=torch.zeros(2, 12, 20, 3, dtype=torch.uint8, device="cuda"), col=5),
           lambda: eng.panel_rgb(a, out=torch.zeros(2, 12, 20, 3, device="cuda"), col=0)]
    for i, f in enumerate(bad):
        with pytest.raises(EndoSurfHipError):
            f()
            pytest.fail(f"call {i} was accepted")
    # the C entries themselves: status 1 with a message, nothing launched on the dummy buffer
    lib = eng.lib
    dummy = torch.zeros(4096, dtype=torch.float64, device="cuda")
    p = C.c_void_p(dummy.data_ptr())
    assert lib.es_ssim(p, p, None, p, 1, 10, 64, 3, 1.0, p, p, None, None) == 1 and b"11" in lib.es_last_error()
    assert lib.es_ssim(p, p, None, p, 1, 64, 64, 5, 1.0, p, p, None, None) == 1 and b"channel" in lib.es_last_error()
    assert lib.es_ssim(p, p, None, p, 4000, 512, 640, 3, 1.0, p, p, None, None) == 1 and b"2^31" in lib.es_last_error()
    assert lib.es_ssim(p, p, None, None, 1, 64, 64, 3, 1.0, p, p, None, None) == 1 and b"window" in lib.es_last_error()
    assert lib.es_ssim(p, p, None, p, 1, 64, 64, 3, float("nan"), p, p, None, None) == 1 and b"data_range" in lib.es_last_error()
    assert lib.es_ssim(p, p, None, p, 1, 64, 64, 3, 1.0, None, p, None, None) == 1 and b"scratch" in lib.es_last_error()
    assert lib.es_ssim(p, p, None, p, 1, 64, 64, 3, 1.0, p, C.c_void_p(dummy.data_ptr() + 4), None, None) == 1 and b"aligned" in lib.es_last_error()
    assert lib.es_ssim(None, None, None, None, 0, 64, 64, 3, 1.0, None, None, None, None) == 0          # an empty batch: nothing to do
    assert lib.es_ssim_scratch_bytes(1, 10, 64) == -1 and lib.es_sq_sums_scratch_bytes(-1, 8, 8) == -1
    assert lib.es_masked_sq_sums(p, p, None, 1, 0, 8, 3, p, p, None) == 1 and lib.es_masked_sq_sums(p, None, None, 1, 8, 8, 3, p, p, None) == 1
    assert lib.es_masked_sq_sums(p, p, None, 1, 8, 8, 17, p, p, None) == 1 and b"channel" in lib.es_last_error()
    assert lib.es_eval_panel_rgb(p, 1, 8, 8, 2, p, 24, 0, None) == 1 and b"1 or 3" in lib.es_last_error()
    assert lib.es_eval_panel_rgb(p, 1, 8, 8, 3, p, 23, 0, None) == 1 and b"pitch" in lib.es_last_error()
    assert lib.es_eval_panel_rgb(p, 1, 8, 8, 3, p, 48, 9, None) == 1 and lib.es_eval_panel_rgb(p, 1, 8, 8, 3, p, 48, -1, None) == 1
    assert lib.es_eval_panel_depth(p, 1, 8, 8, 0.0, p, 24, 0, None) == 1 and b"depth_max" in lib.es_last_error()
    assert lib.es_eval_panel_normal(p, None, 1, 8, 8, 0, None, p, 24, 0, None) == 1 and b"rotation" in lib.es_last_error()
    assert lib.es_eval_panel_normal(p, p, 1, 8, 9000, 0, None, p, 27000, 0, None) == 1
    torch.cuda.synchronize()
    assert int(dummy.abs().sum()) == 0


# ---- through the renderer, on the trained golden ---------------------------------------------------------------------------------------
def test_evaluate_frames_on_the_trained_case():
    """Two 40 x 48 frames of the trained golden case at two times; the ground truth is the render of the same cameras at slightly later
    times (so PSNR is finite and SSIM below 1).  ``color`` / ``depth`` / ``normal_world`` are ``render_frames``' own images; ``normal`` is
    gen_normal's float result of the latter."""
    from gpu_util import renderer_for_case
    from oracle_util import load_case
    r = renderer_for_case(load_case("trained_deform"))
    n, h, w = 2, 40, 48
    K = torch.tensor([[60.0, 0, 23.5, 0], [0, 60.0, 19.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    poses = torch.eye(4).repeat(n, 1, 1)
    poses[:, :3, 3] = torch.tensor([[0.0, 0.0, -1.5], [0.1, -0.05, -1.45]])
    ang = 0.08
    poses[1, :3, :3] = torch.tensor([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]], dtype=torch.float32)
    rays = D.assemble_rays(D.get_rays(K[None].repeat(n, 1, 1).cuda(), poses.cuda(), w, h), torch.zeros(n, 2, device="cuda"))
    rays[0, ..., 8], rays[1, ..., 8] = 0.37, 0.61
    kw = dict(iter_step=1, ray_chunk=512, perturb_overwrite=False)
    later = rays.clone()
    later[..., 8] += 0.04
    truth = r.render_frames(later, **kw)
    gt_c, gt_d = truth["color"].view(n, h, w, 3).clone(), truth["depth"].view(n, h, w, 1).clone()
    rng = np.random.default_rng(11)
    cmask = dev((rng.uniform(size=(n, h, w, 1)) > 0.1).astype(np.float32))
    dmask = cmask * dev((rng.uniform(size=(n, h, w, 1)) > 0.2).astype(np.float32))
    depth_max, ds = 2.0, 1.7
    own = r.render_frames(rays, **kw)
    out = r.evaluate_frames(rays, gt_c, gt_d, dmask, cmask, poses.cuda(), depth_max, depth_scale=ds, **kw)
    assert torch.equal(out["color"].reshape(-1, 3), own["color"]) and torch.equal(out["depth"].reshape(-1, 1), own["depth"])
    assert torch.equal(out["normal_world"].reshape(-1, 3), own["normal"])
    host = {k: out[k].cpu().numpy() for k in ("color", "depth", "normal_world", "normal")}
    gc, gd, cm, dm = gt_c.cpu().numpy(), gt_d.cpu().numpy(), cmask.cpu().numpy(), dmask.cpu().numpy()
    assert set(out["stats"]) == {"psnr_rgb_vr", "ssim_rgb_vr", "rmse_d_vr"} and all(type(v) is float for v in out["stats"].values())
    mean, per_frame = I.ssim(gc, host["color"], cm)
    S, M = I.masked_sq_sums(gc, host["color"], cm)
    Sd, Md = I.masked_sq_sums(gd, host["depth"], dm)
    st = out["stats"]
    print(f"EVAL_MEASURED evaluate_frames: {st}; twins ssim {mean!r} psnr {I.psnr_from_sums(S.sum(), M.sum())!r} rmse {ds * I.rmse_from_sums(Sd.sum(), Md.sum())!r}")
    assert 0.0 < st["ssim_rgb_vr"] < 1.0 and np.isfinite(st["psnr_rgb_vr"]) and st["rmse_d_vr"] > 0.0
    assert abs(st["ssim_rgb_vr"] / mean - 1.0) <= 1e-12
    assert abs(st["psnr_rgb_vr"] / I.psnr_from_sums(S.sum(), M.sum()) - 1.0) <= 1e-12
    assert abs(st["rmse_d_vr"] / (ds * I.rmse_from_sums(Sd.sum(), Md.sum())) - 1.0) <= 1e-12
    pf = {k: v.cpu().numpy() for k, v in out["per_frame"].items()}
    assert all(v.dtype == np.float64 and v.shape == (n,) for v in pf.values())
    assert np.abs(pf["ssim"] / per_frame - 1.0).max() <= 1e-12 and np.abs(pf["psnr"] / I.psnr_from_sums(S, M) - 1.0).max() <= 1e-12
    assert np.abs(pf["rmse"] / (ds * I.rmse_from_sums(Sd, Md)) - 1.0).max() <= 1e-12
    # the host route of data.py on the same arrays (fp32 numpy sums; the depth scaled in fp32 as the reference scales it)
    assert abs(st["psnr_rgb_vr"] / D.cal_psnr(gc, host["color"], cm) - 1.0) <= 1e-6
    assert abs(st["rmse_d_vr"] / D.cal_rmse(gd * np.float32(ds), host["depth"] * np.float32(ds), dm) - 1.0) <= 1e-6
    # pictures
    want_f, want_b = I.panel_normal(host["normal_world"], poses.numpy())
    assert np.abs(host["normal"] - want_f).max() <= 1e-6
    sheet = out["sheet"].cpu().numpy()
    assert sheet.shape == (n, h, 5 * w, 3) and sheet.dtype == np.uint8
    twins = {"rgb_gt": (I.panel_rgb(gc), I.panel_rgb_values(gc)), "rgb_pred": (I.panel_rgb(host["color"]), I.panel_rgb_values(host["color"])),
             "depth_gt": (I.panel_depth(gd, depth_max), np.concatenate([I.panel_depth_values(gd, depth_max)] * 3, -1)),
             "depth_pred": (I.panel_depth(host["depth"], depth_max), np.concatenate([I.panel_depth_values(host["depth"], depth_max)] * 3, -1)),
             "normal_pred": (want_b, 128.0 * I.panel_normal_values(host["normal_world"], poses.numpy()) + 128.0)}
    for i, k in enumerate(I.PANELS):
        got = out["panels"][k].cpu().numpy()
        assert np.array_equal(sheet[:, :, i * w:(i + 1) * w], got), k
        assert_bytes(got, twins[k][0], twins[k][1], k)
    assert sheet[:, :, :2 * w].std() > 1.0          # something was drawn
