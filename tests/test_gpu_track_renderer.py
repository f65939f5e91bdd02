"""GPU, renderer level: the surface-track methods of the renderer (renderer_track.py over csrc/deform.hip) against the fp64 oracle and
against the host twin driven by ``renderer.deform``.  Budgets as in tests/test_gpu_track.py; figures are printed."""
import numpy as np
import pytest
import torch

import weightgen
from gpu_util import net_cfg, renderer_for, state_to_ckpt
from oracle_util import RENDER_CFG
from track_util import FLT_MAX, RHO, TOL, assert_contraction, budget, deform_fn, draw, oracle_net, rownorm

from endosurf_amd import tracking

pytestmark = pytest.mark.gpu

SEED, MODE = 11, "trained"
KEYS = ("points", "step", "iters", "converged")


@pytest.fixture(scope="module")
def S():
    r = renderer_for(SEED, MODE, True)
    net64 = oracle_net(weightgen.make_state(SEED, MODE, True), torch.float64)
    return dict(r=r, net64=net64, fn64=deform_fn(net64))


def _e_fwd(S, x, *times):
    """The largest error (row 2-norm) of ``renderer.deform`` against the fp64 oracle at host points ``x`` and each of ``times``."""
    e = 0.0
    for t in times:
        tt = t.expand(x.shape[0]) if t.numel() == 1 else t
        e = max(e, float(rownorm(S["r"].deform(x, t).cpu().double() - S["fn64"](x.double(), tt.double())).max()))
    return e


def test_renderer_methods_against_the_oracle(S):
    r, fn64 = S["r"], S["fn64"]
    x, t_from, t_to = draw(SEED, 200)
    assert_contraction(S["net64"], x, t_from, t_to)
    e_fwd = _e_fwd(S, x, t_from, t_to)
    xd, tf, tt = x.cuda(), t_from.cuda(), t_to.cuda()
    c = r.to_canonical(xd, tf)
    assert c.is_cuda and c.shape == (200, 3)
    back = r.to_observed(c, tf)
    assert set(back) == set(KEYS) and all(back[k].is_cuda for k in KEYS) and back["iters"].dtype == torch.int32
    assert bool(back["converged"].all())
    e_back = float(rownorm(back["points"].cpu().double() - x.double()).max())
    w = r.warp_points(xd, tf, tt)
    ref = tracking.warp_points(fn64, x.double(), t_from.double(), t_to.double(), max_iters=200, tol=1e-13)
    assert bool(ref["converged"].all()) and bool(w["converged"].all())
    e_warp = float(rownorm(w["points"].cpu().double() - ref["points"]).max())
    print(f"\ne_fwd {e_fwd:.3e} budget {budget(e_fwd):.3e}: canonical and back {e_back:.3e}, warp against the oracle {e_warp:.3e}")
    assert e_back <= budget(e_fwd) and e_warp <= budget(e_fwd)


@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
def test_one_launch_solver_equals_the_twin_over_renderer_deform(S, warm):
    r = S["r"]
    x, _, _ = draw(SEED, 130)
    t_from, times = 0.3, torch.tensor([0.31, 0.32, 0.9])
    assert_contraction(S["net64"], x, torch.tensor([t_from]), *times.reshape(-1, 1))
    xd = x.cuda()
    twin = tracking.track_points(r.deform, xd, t_from, times.cuda(), warm_start=warm, max_iters=64, tol=TOL)
    got = r.track_points(xd, t_from, times, warm_start=warm)
    assert got["points"].shape == (3, 130, 3) and got["canonical"].shape == (130, 3) and got["iters"].shape == (3, 130)
    assert all(got[k].is_cuda for k in got)
    assert bool(got["converged"].all()) and bool(twin["converged"].all())
    d = float(rownorm(got["points"] - twin["points"]).max())
    di = int((got["iters"] - twin["iters"]).abs().max())
    print(f"\nwarm {warm}: |kernel - twin| {d:.3e} (bound {2 * TOL / (1 - RHO):.3e}), |iters - twin| {di}, evaluations {int(got['iters'].sum())}")
    assert torch.equal(got["canonical"], twin["canonical"])
    assert d <= 2 * TOL / (1 - RHO) and di <= 1


def test_track_mesh_on_a_small_extracted_mesh(S):
    r = S["r"]
    mesh = r.extract_observation_mesh(0.3, [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0], 24)
    v = mesh["vertices"]
    V = v.shape[0]
    times = [0.3, 0.31, 0.32, 0.9]
    vh = v.cpu()
    rho = assert_contraction(S["net64"], vh, *[torch.tensor([t]) for t in times])
    e_fwd = _e_fwd(S, vh, torch.tensor([0.3]))
    out = r.track_mesh(mesh, t=0.3, times=times)
    assert out["triangles"] is mesh["triangles"]
    assert out["vertices"].shape == (4, V, 3) and out["displacement"].shape == (4, V) and out["canonical"].shape == (V, 3)
    e0 = float(rownorm(out["vertices"][0] - v).max())
    print(f"\nV {V} rho {rho:.3f} e_fwd {e_fwd:.3e}: frame 0 off by {e0:.3e} (budget {budget(e_fwd):.3e}), iters max {int(out['iters'].max())}, "
          f"evaluations {int(out['iters'].sum())}, largest displacement {float(out['displacement'].max()):.3f}")
    assert bool(out["converged"].all())
    assert e0 <= budget(e_fwd) and float(out["displacement"][0].max()) < budget(e_fwd)
    # vertices and triangles given apart, cold: the same positions within the twin's bound
    cold = r.track_mesh(v, mesh["triangles"], t=0.3, times=times, warm_start=False)
    assert cold["triangles"] is mesh["triangles"] and bool(cold["converged"].all())
    assert float(rownorm(cold["vertices"] - out["vertices"]).max()) <= 2 * TOL / (1 - RHO)


def test_host_inputs(S):
    """A Python float, a host tensor and a numpy array are moved to the renderer's device, not handed to a kernel as they are: each
    call equals the call with device tensors bit for bit.  The new methods come first; ``sdf_observed`` last."""
    r = S["r"]
    x, t_from, _ = draw(SEED, 100)
    xd, td = x.cuda(), t_from.cuda()
    t3 = torch.full((100,), 0.3, device="cuda")
    c_dev = r.to_canonical(xd, td)
    assert torch.equal(r.to_canonical(x, t_from), c_dev) and torch.equal(r.to_canonical(x.numpy(), t_from.numpy()), c_dev)
    c3 = r.to_canonical(xd, t3)
    assert torch.equal(r.to_canonical(x, 0.3), c3) and torch.equal(r.to_canonical(xd, torch.tensor(0.3)), c3)
    o_dev, o3 = r.to_observed(c_dev, td), r.to_observed(c3, t3)
    for got, want in ((r.to_observed(c_dev.cpu(), t_from), o_dev), (r.to_observed(c3.cpu().numpy(), 0.3), o3),
                      (r.to_observed(c3, torch.tensor([0.3])), o3)):
        assert all(torch.equal(got[k], want[k]) for k in KEYS)
    s_dev, s3 = r.sdf_observed(xd, td), r.sdf_observed(xd, t3)
    assert torch.equal(r.sdf_observed(x, t_from), s_dev) and torch.equal(r.sdf_observed(xd, t_from), s_dev)
    assert torch.equal(r.sdf_observed(x.numpy(), 0.3), s3) and torch.equal(r.sdf_observed(x, torch.tensor([0.3])), s3)


def test_without_a_deformation_network():
    r = renderer_for(SEED, MODE, False)
    x, t_from, _ = draw(SEED, 70)
    xd = x.cuda()
    assert torch.equal(r.to_canonical(x, t_from), xd) and bool((r.deform(xd, 0.5) == 0).all())
    out = r.to_observed(xd, t_from)
    assert torch.equal(out["points"], xd) and bool((out["step"] == 0).all()) and bool((out["iters"] == 1).all()) and bool(out["converged"].all())
    tr = r.track_points(xd, 0.2, [0.3, 0.9])
    assert torch.equal(tr["points"], xd[None].expand(2, 70, 3)) and bool(tr["converged"].all())


def test_the_cap_and_the_refused_update_at_renderer_level(S):
    """max_iters = 3 at tol 1e-7 leaves every row unconverged; a deformation whose squared step overflows is refused row by row, and the
    fp32 host twin driven by ``renderer.deform`` gives the same three arrays."""
    from endosurf_amd import EndoSurfRenderer
    x, _, t_to = draw(SEED, 70)
    xd, td = x.cuda(), t_to.cuda()
    capped = S["r"].to_observed(xd, td, max_iters=3, tol=1e-7)
    assert bool((capped["iters"] == 3).all()) and not bool(capped["converged"].any()) and bool(torch.isfinite(capped["points"]).all())
    with pytest.raises(ValueError):
        S["r"].to_observed(xd, td, max_iters=0)
    with pytest.raises(ValueError):
        S["r"].to_observed(xd, td, tol=float("nan"))
    state = weightgen.make_state(SEED, MODE, True)
    state["deform_network.net.8.bias"] = np.full(3, 3e38, np.float32)
    r = EndoSurfRenderer(dict(RENDER_CFG), net_cfg(True), device="cuda")
    r.load_checkpoint(state_to_ckpt(state, True))
    out = r.to_observed(xd, td)
    assert bool((out["iters"] == 1).all()) and bool((out["step"] == FLT_MAX).all()) and torch.equal(out["points"], xd)
    assert not bool(out["converged"].any())
    ty, ts, ti = tracking.inverse_deform(r.deform, xd, td, max_iters=64, tol=TOL)
    assert torch.equal(out["points"], ty) and torch.equal(out["step"], ts) and torch.equal(out["iters"], ti)
