"""The OPT-IN split-precision family (csrc/infer_x3r.hip, query_x3.hip, x3r_core.h) through the shape tests of the fp32 family
(test_gpu_forward_shapes.py): row by row against the fp64 oracle, MAXIMUM gates, points screened away from the ReLU kinks, at the
family's own tile edges (a wave owns 16 points in k_deform_jvp_x3r, 32 in the VJP / SDF / colour kernels, 128-point blocks in
k_query_sdf_x3r), NaN-filled workspaces.

  A  es_point_forward_x3: every buffer of every row -- dense point counts around 16 / 32 / 64 / 128, with ES_PF_SAVE (the training
     chain: split deformation and colour kernels around the fp32 SDF kernels) and without (split SDF kernel too), 20 031 rows and the
     fused 65 536 + 3 072 launch (deform_jvp_x3r_with_tail), the shipped routing threshold, the three point sources
  C  es_query_sdf_x3 at the sizes the product sends it (>= 8 193 points, or strided with ray_done: always the 128-point-block kernel)
     and Engine.ray_marching with split_precision: bracket and secant steps on the values the split kernel returned

Helpers, seeds and point sets are those of test_gpu_forward_shapes.py (``split=True``), so the oracle's passes are shared when both
modules run in one session.  Gates: shapes_util.FORWARD_GATE unchanged; the query's 1e-5 and 3 x the fp32 kernel's error + 2e-6 of
test_gpu_query_x3.py.  The split VJP sweep does not compute the time adjoint, so tbar is compared only on the rows the fp32 tile
bodies write (the colour-less tail of the fused training launch).  Every case asserts that the split family ran.  Worst errors per
case and buffer go to forward_shapes_x3.json in the log directory of test_gpu_backward.py."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import test_gpu_forward_shapes as F
from oracle import endosurf_oracle as O
from shapes_util import routes_split, split_chain

pytestmark = pytest.mark.gpu
NAN = float("nan")


# ------------------------------------------------------------------------------------------------------------------------------
# A. point forward
# ------------------------------------------------------------------------------------------------------------------------------
DENSE_M = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1024, 1100, 1400]


@pytest.mark.parametrize("save", [True, False])
@pytest.mark.parametrize("use_deform", [True, False])
@pytest.mark.parametrize("M", DENSE_M)
@pytest.mark.parametrize("color", [True, False])
def test_point_forward_dense(use_deform, M, color, save):
    """One row before, on and behind a wave's 16 / 32 points, a 64-row colour tile and a 128-row block; 16 / 18 / 22 jvp tiles."""
    F._dense("trained", use_deform, M, color, save=save, poison=NAN, split=True)


@pytest.mark.parametrize("save", [True, False])
@pytest.mark.parametrize("M", [65, 1100])
def test_point_forward_dense_init_weights(M, save):
    F._dense("init", True, M, True, save=save, split=True)


@pytest.mark.parametrize("save", [True, False])
@pytest.mark.parametrize("poison", [None, NAN])
def test_point_forward_workspace_history(poison, save):
    """M = 65 right behind M = 1400 on one engine: recycled memory, or a workspace filled with NaN before the launch."""
    F._dense("trained", True, 1400, True, save=save, split=True)
    F._dense("trained", True, 65, True, save=save, poison=poison, split=True)


def _tail_is_fp32(use_deform, save, M, m_color):
    """The fused training launch (point_fwd.hip: ES_PF_SAVE, a deformation network, a colour-less tail behind a 128-aligned main part)
    runs the tail's rows as fp32 tile bodies, which write the time adjoint."""
    return use_deform and save and 0 < m_color < M and m_color % 128 == 0


@pytest.mark.parametrize("save", [True, False])
@pytest.mark.parametrize("name", list(F.LARGE))
def test_point_forward_large(name, save):
    """20 031 rows (ragged last tile of every launch) and 65 536 + 3 072 with a colour-less tail, the layout of the split headline: on
    the row subsets of the fp32 case, into a NaN-filled workspace; every row [0, M) finite."""
    M, m_color, use_deform, K, x, d, t, redrawn = F._large_inputs(name)
    eng, weff, packed, net = F._setup("trained", use_deform)
    dev = lambda a: a.cuda().contiguous()
    ctx = F._launch(eng, weff, packed, eng.points(x=dev(x), t=dev(t), dirs=dev(d)), F._flags(use_deform, True, save), m_color, poison=NAN,
                    split=True)
    tail_names = F._names(use_deform, False) if _tail_is_fp32(use_deform, save, M, m_color) else None
    F._compare_large(f"X3_A_large_{name}" + ("" if save else "_nosave"), name, ctx, net, K, x, d, t, m_color, use_deform, redrawn, split=True,
                     tail_names=tail_names)


@pytest.mark.parametrize("save", [True, False])
def test_point_forward_shipped_threshold(save):
    """x3_infer_min left at its default: M = 16 383 stays on the fp32 kernels, M = 16 384 goes split.  Both on a row subset."""
    eng, weff, packed, net = F._setup("trained", True)
    M = 16384
    assert eng.x3_infer_min == M
    K = F._subset_rows(M, 17)
    x, d, t, redrawn = F._screened(("x3_threshold_in",), M, 8000 + M, True, screen=K)
    ref, own32 = F._reference(("x3_threshold",), net, x[K], d[K], t[K], True)
    dev = lambda a: a.cuda().contiguous()
    flags = F._flags(True, True, save)
    with split_chain(eng, True, infer_min=None):
        assert not routes_split(eng, M - 1, save) and routes_split(eng, M, save)
        below = eng.point_forward(eng.points(x=dev(x[:M - 1]), t=dev(t[:M - 1]), dirs=dev(d[:M - 1])), weff, packed, flags)
        torch.cuda.synchronize()
    assert below.px3 is None and not below.x3_chain, "16 383 points went to the split family"
    ctx = F._launch(eng, weff, packed, eng.points(x=dev(x), t=dev(t), dirs=dev(d)), flags, poison=NAN, split=True, infer_min=None)
    case = "X3_A_threshold_16384" + ("" if save else "_nosave")
    F._note(case, redrawn=redrawn)
    F._compare(case, ctx, ref, own32, K, names=F._names(True, True, split=True))
    F._finite(ctx, F._names(True, True, split=True), M)
    assert K[-1] == M - 1          # extra: the fp32 kernels one point below the threshold, on the same rows but the last
    F._compare(case.replace("16384", "16383_fp32"), below, {k: v[:-1] for k, v in ref.items()}, own32, K[:-1])


@pytest.mark.parametrize("save", [True, False])
@pytest.mark.parametrize("use_deform", [True, False])
@pytest.mark.parametrize("n,N", F.RAY_SAMPLES)
def test_point_source_ray_samples(n, N, use_deform, save):
    """Mode 1 (ldz > n_per_ray, d.z < 0, |d.z| = 1e-3) into the 16- and 32-points-per-wave row mappings."""
    F._ray_samples(n, N, use_deform, split=True, save=save)


@pytest.mark.parametrize("save", [True, False])
@pytest.mark.parametrize("use_deform", [True, False])
def test_point_source_samples_then_points_small(use_deform, save):
    F._samples_then_points_small(use_deform, split=True, save=save)


@pytest.mark.parametrize("save", [True, False])
def test_point_source_training_step_layout(save):
    """Mode 2 at the size of every training step: 1 024 x 64 ray samples + 3 072 explicit points, m_color = 65 536."""
    tail_names = F._names(True, False) if _tail_is_fp32(True, save, 65536 + 3072, 65536) else None
    F._training_step_layout(split=True, save=save, tail_names=tail_names)


@pytest.mark.parametrize("save", [True, False])
@pytest.mark.parametrize("use_deform", [True, False])
def test_point_source_shared_time(use_deform, save):
    F._shared_time(use_deform, split=True, save=save)


# ------------------------------------------------------------------------------------------------------------------------------
# C. the split query at the sizes the product uses
# ------------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _poisoned(eng, value=NAN):
    """Every fp32 buffer Engine.empty hands out inside starts from ``value``."""
    plain = eng.empty
    eng.empty = lambda *s, **k: plain(*s, **k).fill_(value) if k.get("dtype", torch.float32) == torch.float32 else plain(*s, **k)
    try:
        yield
    finally:
        del eng.empty


@pytest.mark.parametrize("use_deform", [True, False])
@pytest.mark.parametrize("M", [8193, 8320, 16385, 20031])
def test_query_sdf_flat(M, use_deform):
    """Engine.query_sdf with split_precision: 1, 0, 1 and 63 rows into the last 128-point block.  sdf is continuous across the ReLU
    kinks: no screening, EVERY row against OracleNet.sdf_observed in fp64."""
    eng, weff, packed, net = F._setup("trained", use_deform)
    rng = np.random.default_rng(5 + M)
    x = torch.from_numpy(rng.uniform(-0.8, 0.8, size=(M, 3)).astype(np.float32))
    t = torch.from_numpy(rng.uniform(size=(M,)).astype(np.float32))
    xd, td = x.cuda().contiguous(), t.cuda().contiguous()
    with split_chain(eng), _poisoned(eng):
        assert eng._use_x3(M) and M >= eng.x3_query_min
        got = eng.query_sdf(eng.points(x=xd, t=td), weff, packed, use_deform)
        eng.split_precision = False          # extra: the fp32 kernel on the same rows (split_chain restores the setting)
        assert not eng._use_x3(M)
        got32 = eng.query_sdf(eng.points(x=xd, t=td), weff, packed, use_deform)
        torch.cuda.synchronize()
    with torch.no_grad():
        ref = net.sdf_observed(x.double(), t.double()[:, None])[:, 0]
    assert tuple(got.shape) == (M,) and bool(torch.isfinite(got).all()), (~torch.isfinite(got)).nonzero().flatten()[:8]
    e = (got.cpu().double() - ref).abs()
    err, err32 = float(e.max()), float((got32.cpu().double() - ref).abs().max())
    F._note(f"X3_C_flat_{int(use_deform)}_{M}", sdf=[err, err32], rows=M)
    assert err < 1e-5 and err <= 3 * err32 + 2e-6, (err, err32, "rows", e.argsort(descending=True)[:6].tolist())


def _done_pattern(name, N, rays_per_block):
    blk = np.arange(N) // rays_per_block
    done = np.zeros(N, np.int32)
    if name == "all":
        done[:] = 1
    elif name == "whole_blocks":          # every other 128-point block finished
        done[blk % 2 == 1] = 1
    elif name == "half_blocks":           # the second half of every block's rays finished: no block may be skipped
        done[np.arange(N) % rays_per_block >= rays_per_block // 2] = 1
    elif name == "last_block_live":       # one live ray, in the (at N = 515 ragged) last block
        done[:] = 1
        done[N - 1] = 0
    elif name == "last_block_done":       # only the last block finished
        done[blk == blk[-1]] = 1
    else:
        assert name == "none"
    return done


@pytest.mark.parametrize("pattern", ["none", "all", "whole_blocks", "half_blocks", "last_block_live", "last_block_done"])
@pytest.mark.parametrize("use_deform", [True, False])
@pytest.mark.parametrize("N,B", [(512, 16), (515, 16), (512, 32), (515, 32)])
def test_query_sdf_strided(N, B, use_deform, pattern):
    """es_query_sdf_x3 in its strided / ray_done form (k_query_sdf_x3r whatever M; 8 or 4 rays per 128-point block, at N = 515 a ragged
    last block of 48 / 96 points): the B proposals [col0, col0 + B) of every ray into the same columns of a [N, 48] sentinel buffer.
    Columns outside stay the sentinel bit for bit; a block whose rays are all finished is skipped (sentinel); every other point
    -- all of them, live ray or not -- holds the oracle's value."""
    from endosurf_amd import _lib
    col0, ld = 8, 48
    rpb = 128 // B
    eng, weff, packed, net = F._setup("trained", use_deform)
    rays, zmax, rng = F._ray_set(N, 600 + N + B)
    zfull = (torch.from_numpy(rng.uniform(size=(N, ld))).double() * zmax[:, None]).float()
    key = ("x3_query", N, B, use_deform)
    if key not in F._ORACLE:
        x, _, t = F._ray_points(rays, zfull[:, col0:col0 + B])
        with torch.no_grad():
            F._ORACLE[key] = net.sdf_observed(x, t[:, None])[:, 0].reshape(N, B)
    ref = F._ORACLE[key]
    rays_d, z_d = rays.cuda().contiguous(), zfull.cuda().contiguous()
    done = _done_pattern(pattern, N, rpb)
    done_d = None if pattern == "none" else torch.from_numpy(done).cuda()
    out = torch.full((N, ld), F.SENTINEL, device="cuda")
    p = eng.points(rays=rays_d, z=z_d, n_per_ray=B, ldz=ld)
    p.z = C.c_void_p(z_d.data_ptr() + 4 * col0)
    _lib.check(eng.lib.es_query_sdf_x3(C.byref(p), _lib.ptr(eng.packed_x3(weff, use_deform)), _lib.ptr(weff), C.c_void_p(out.data_ptr() + 4 * col0), ld,
                                       _lib.ptr(done_d) if done_d is not None else None, int(use_deform), eng.st()), "es_query_sdf_x3")
    torch.cuda.synchronize()
    got = out.cpu()
    bits = lambda a: a.contiguous().view(torch.int32)
    sent = bits(torch.full((1,), F.SENTINEL))[0]
    outside = torch.ones(ld, dtype=torch.bool); outside[col0:col0 + B] = False
    assert bool((bits(got)[:, outside] == sent).all()), "columns outside [col0, col0 + B) were written"
    win = got[:, col0:col0 + B]
    is_sent = bits(win) == sent
    # a block = 128 consecutive points = rpb consecutive rays (B divides 128): skipped iff all of its rays are finished
    blk = np.arange(N) // rpb
    skipped = np.array([pattern != "none" and bool(done[blk == b].all()) for b in range(blk[-1] + 1)])[blk]
    skipped_t = torch.from_numpy(skipped)
    assert bool(is_sent[skipped_t].all()), ("a block of finished rays was written", (~is_sent[skipped_t].all(1)).nonzero().flatten()[:8])
    assert not bool(is_sent[~skipped_t].any()), ("unwritten proposals", np.flatnonzero(~skipped)[is_sent[~skipped_t].any(1).numpy()][:8])
    expect = {"none": 0, "all": N, "half_blocks": 0, "last_block_live": (N - 1) // rpb * rpb, "last_block_done": N - (N - 1) // rpb * rpb}
    if pattern in expect:
        assert int(skipped.sum()) == expect[pattern], (int(skipped.sum()), expect[pattern])
    else:
        assert 0 < int(skipped.sum()) < N
    assert bool(torch.isfinite(win).all())
    if (~skipped).any():
        e = (win[~skipped_t].double() - ref[~skipped_t]).abs()
        worst = float(e.max())
        bad_rays = np.flatnonzero(~skipped)[e.max(1)[0].argsort(descending=True)[:6].numpy()]
    else:
        worst, bad_rays = 0.0, []
    F._note(f"X3_C_strided_{int(use_deform)}_{N}x{B}_{pattern}", sdf=[worst, None], rows=int((~skipped).sum()) * B, skipped_rays=int(skipped.sum()))
    assert worst < 1e-5, (worst, "rays", list(bad_rays))


# ---- ray marching ------------------------------------------------------------------------------------------------------------
def _march_inputs(use_deform):
    """515 SyntheticScene rays (those of the fp32 file's case; the first 512 serve the 512-ray cases), the 128 proposal depths per ray
    (es_ray_setup) and the fp64 sdf at the proposals' points."""
    key = ("x3_march", use_deform)
    if key not in F._ORACLE:
        from endosurf_amd.trainer import SyntheticScene
        eng, weff, packed, net = F._setup("trained", use_deform)
        rays = SyntheticScene("cuda", seed=17).batch(515)["rays"].contiguous()
        dprop = eng.empty(515, 128)
        eng.ray_setup(rays, None, 128, 0.0, 1, dprop)
        torch.cuda.synchronize()
        x, _, t = F._ray_points(rays.cpu(), dprop.cpu())
        with torch.no_grad():
            F._ORACLE[key] = (rays.cpu(), dprop.cpu(), net.sdf_observed(x, t[:, None])[:, 0].reshape(515, 128))
    return F._ORACLE[key]


@pytest.mark.parametrize("use_deform", [True, False])
@pytest.mark.parametrize("march_block", [32, 0])
@pytest.mark.parametrize("N", [512, 515])
def test_ray_marching_split(N, march_block, use_deform):
    """Engine.ray_marching with split_precision sends the proposals to es_query_sdf_x3 (4 strided launches with ray_done, or one flat
    launch of N x 128 points) and the 8 secant queries of N points to the fp32 kernel.  Ray marching is a discrete function of the sdf
    values, so it is checked on the values the kernels returned: (1) the proposals' sdf (march_begin's kept buffer) against fp64 --
    in the block path a proposal is either the oracle's value or the 0 the skipped tiles leave, and a ray that is not finished
    when a block starts has all of that block; (2) flags / bracket / first estimate against oracle.march_bracket on those values;
    (3) eight secant iterations against oracle.secant_step fed with the kernel's own mid-point values, those values against fp64;
    (4) Engine.ray_marching itself against the result of (3)."""
    eng, weff, packed, net = F._setup("trained", use_deform)
    rays, dprop, ref = (a[:N] for a in _march_inputs(use_deform))
    rays_d = rays.cuda().contiguous()
    n, B = 128, march_block
    blocks = bool(B and N * B >= 16384)
    old = eng.march_block
    eng.march_block = march_block
    try:
        with split_chain(eng), _poisoned(eng):
            assert eng._use_x3(N * (B if blocks else n)) and not eng._use_x3(N)
            ms = eng.march_begin(rays_d, weff, packed, use_deform)
            torch.cuda.synchronize()
            kept_dprop, sdf = (a.cpu().reshape(N, n) for a in ms["keep"])          # (the one-launch query returns its values flat)
            state, flags, d_pred = ms["state"].clone(), ms["flags"].clone(), ms["d_pred"].clone()
            d_direct = eng.ray_marching(rays_d, weff, packed, use_deform)
            torch.cuda.synchronize()
    finally:
        eng.march_block = old
    assert blocks == bool(march_block) and torch.equal(kept_dprop, dprop)
    # (1) the proposals' values
    assert bool(torch.isfinite(sdf).all())
    err = (sdf.double() - ref).abs()
    val = -sdf.double()                                                    # endosurf.py:375 with tau = 0
    if blocks:
        unwritten = (sdf == 0) & (err >= 1e-5)
        for b in range(1, n // B):
            nv = b * B
            done = ((val[:, :nv - 1] * val[:, 1:nv]) < 0).any(1) | ~(val[:, 0] < 0)          # es_march_progress's definition
            assert not bool(unwritten[~done, nv:nv + B].any()), ("a live ray misses proposals of block", b)
        assert not bool(unwritten[:, :B].any()), "the first block has no ray_done"
        err = torch.where(unwritten, torch.zeros_like(err), err)
        n_unwritten = int(unwritten.sum())
    else:
        n_unwritten = 0
    worst = float(err.max())
    assert worst < 1e-5, (worst, "rays", err.max(1)[0].argsort(descending=True)[:6].tolist())
    # (2) bracket search on the kernel's values
    want = O.march_bracket(val, dprop.double())
    mask, m0, d_low, f_low, d_high, f_high = want
    d0 = eng.empty(N, 1)
    _lib_check_finish(eng, d_pred, flags, N, d0)
    F._check_find((state.cpu(), flags.cpu(), d_pred.cpu(), d0.cpu()[:, 0]), want, ("x3 march", N, march_block, use_deform))
    assert int(mask.sum()) >= N // 4
    # (3) the secant iterations, mid-point values from the fp32 query (N < x3_query_min)
    ref_pred = O.secant_estimate(d_low, f_low, d_high, f_high)
    x_d, t_d = eng.empty(N, 3), eng.empty(N)
    worst_d = worst_f = 0.0
    with split_chain(eng):
        for it in range(8):
            eng.secant_points(rays_d, d_pred, N, x_d, t_d)
            f_mid = eng.query_sdf(eng.points(x=x_d, t=t_d), weff, packed, use_deform)
            torch.cuda.synchronize()
            with torch.no_grad():
                f64 = net.sdf_observed(x_d.cpu().double(), t_d.cpu().double()[:, None])[:, 0]
            worst_f = max(worst_f, float((f_mid.cpu().double() - f64)[mask].abs().max()))
            eng.secant_update(f_mid, N, 0.0, state, d_pred)
            torch.cuda.synchronize()
            d_low, f_low, d_high, f_high, ref_pred = O.secant_step(d_low, f_low, d_high, f_high, ref_pred, f_mid.cpu().double())
            ed = ((d_pred.cpu().double() - ref_pred).abs() / ref_pred.abs().clamp(min=1.0))[mask]
            worst_d = max(worst_d, float(ed.max()))
    assert worst_f < 1e-5 and worst_d < 1e-5, (worst_f, worst_d)
    # (4) the product's call: the same launches on the same inputs
    d = d_direct.cpu()[:, 0].double()
    assert torch.equal(torch.isinf(d), ~mask & m0) and torch.equal(d == 0, ~m0), "inf / 0 pattern"
    worst_call = float(((d - ref_pred).abs() / ref_pred.abs().clamp(min=1.0))[mask].max())
    F._note(f"X3_C_march_{int(use_deform)}_{N}_{march_block}", sdf=[worst, None], secant_mid=worst_f, d_pred=worst_d, d_call=worst_call,
            hits=int(mask.sum()), unwritten=n_unwritten)
    assert worst_call < 1e-5, worst_call


def _lib_check_finish(eng, d_pred, flags, N, d_out):
    from endosurf_amd import _lib
    _lib.check(eng.lib.es_march_finish(_lib.ptr(d_pred), _lib.ptr(flags), N, _lib.ptr(d_out), eng.st()), "es_march_finish")
    torch.cuda.synchronize()
