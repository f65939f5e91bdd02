"""The forward kernels against the fp64 oracle AWAY from the golden shape (48 rays x 32 + 32 samples, 192 points) and the few point
counts of test_gpu_point.py: row by row at the shapes where tiles, pad rows, launch layouts and point sources change.

  A  point forward: every output buffer of every row (x_c, sdf, feat, g_c, J d, g_o, rgb, the time adjoint) with MAXIMUM gates on test
     points screened away from the ReLU kinks; dense point counts, the fused colour-less-tail launches at 68 608 rows (oracle on a row
     subset), es_point_forward_rows, the layout without ES_PF_SAVE, the three point sources, workspace history
  B  es_query_sdf_rays: strided output into a sentinel-filled buffer, the ray_done tile skip
  C  ray marching: bracket search / early exit / secant update on synthetic profiles against oracle.march_bracket / secant_step, and
     Engine.ray_marching on the network at training size (block path and one-launch path)
  D  the sampling chain (es_sample_z and the launch-by-launch form) at other sample counts, up-sampling steps and on degenerate rays

The reference of every comparison is the oracle in fp64 (oracle/endosurf_oracle.py); kernel-against-kernel only where stated as an
extra.  Worst errors per case are written to forward_shapes.json in the log directory of test_gpu_backward.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import weightgen
from oracle import endosurf_oracle as O
from oracle_util import RENDER_CFG
from shapes_util import FORWARD_GATE, RELU_MARGIN, SEED, inputs, oracle_net, relu_margin, routes_split, split_chain
from test_gpu_backward import LOG

pytestmark = pytest.mark.gpu
_REPORT, _REPORT_X3, _ENGINES, _ORACLE = {}, {}, {}, {}


def _note(case, **values):
    """Cases of the split-precision family (test_gpu_forward_shapes_x3.py; their names start with X3_) go to forward_shapes_x3.json."""
    report, name = (_REPORT_X3, "forward_shapes_x3.json") if case.startswith("X3_") else (_REPORT, "forward_shapes.json")
    report.setdefault(case, {}).update(values)
    os.makedirs(LOG, exist_ok=True)
    with open(os.path.join(LOG, name), "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)


def _setup(mode="trained", use_deform=True):
    """One engine (one caching-allocator history) per weight set for the whole module: (engine, weff, packed, fp64 oracle net)."""
    key = (mode, use_deform)
    if key not in _ENGINES:
        from endosurf_amd import params
        from endosurf_amd.engine import Engine
        eng = Engine("cuda")
        flat = torch.from_numpy(params.flatten_state(weightgen.make_state(SEED, mode, use_deform))).cuda()
        weff, packed = eng.weightnorm_pack(flat, use_deform)
        _ENGINES[key] = (eng, weff, packed, oracle_net(mode, use_deform))
    return _ENGINES[key]


def _flags(use_deform, color, save=True):
    from endosurf_amd import _lib
    return (_lib.PF_DEFORM if use_deform else 0) | (_lib.PF_COLOR if color else 0) | (_lib.PF_SAVE if save else 0)


# ------------------------------------------------------------------------------------------------------------------------------
# A. point forward, row by row, buffer by buffer
# ------------------------------------------------------------------------------------------------------------------------------
# Maximum gates over ALL compared rows: shapes_util.FORWARD_GATE, ~8 x the worst error of any case of this file on an MI355X.
GATE = FORWARD_GATE


def _oracle_rows(net, x, d, t, color, dtype=torch.float64):
    """OracleNet.point_eval on (x, d, t) in ``dtype`` -> {buffer name: float64 ndarray}.  tbar = d sdf / d t = <g_c, d x_c / d t> by autograd."""
    c = lambda a: a.to(dtype)
    if dtype != torch.float64:
        net = O.OracleNet({k: v.to(dtype) for k, v in net.p.items()}, net.use_deform)
    x, d, t = c(x), c(d), c(t).reshape(-1, 1)
    with torch.no_grad():
        pe = net.point_eval(x, d, t, with_color=color)
    out = dict(xc=pe["x_c"], sdf=pe["sdf"], gc=pe["g_c"], go=pe["g_o"])
    if net.use_deform:
        out["v"] = torch.einsum("mik,mk->mi", pe["J"], d)             # the kernels carry J d (JVP) and J^T g_c (VJP), not J
        tt = t.clone().requires_grad_(True)
        dx, _ = net.deform(x, tt, with_jac=False)
        out["tbar"] = torch.autograd.grad(net.sdf_net(x + dx, with_grad=False)[0].sum(), tt)[0]
    if color:
        out["feat"], out["rgb"] = pe["feat"], pe["rgb"]
    return {k: v.detach().double().numpy() for k, v in out.items()}


def _reference(key, net, x, d, t, color):
    """fp64 oracle + the oracle's own fp32 error on the same rows, cached per ``key`` (several launch layouts share one set of points)."""
    if key not in _ORACLE:
        ref = _oracle_rows(net, x, d, t, color)
        r32 = _oracle_rows(net, x, d, t, color, torch.float32)
        _ORACLE[key] = (ref, {k: float(np.abs(r32[k] - ref[k]).max()) for k in ref})
    return _ORACLE[key]


def _compare(case, ctx, ref, own32, rows, names=None, gate=GATE):
    """Workspace rows ``rows`` against the oracle (row i of ``ref`` belongs to workspace row rows[i]): the maximum error of every buffer
    in ``names`` (default: all of ``ref``) under ``gate``; nothing in these rows may be non-finite."""
    rows_t = torch.as_tensor(np.asarray(rows, np.int64), device="cuda")
    worst, bad = {}, {}
    for k in (names or ref):
        got = ctx.view(k).index_select(0, rows_t).double().cpu().numpy().reshape(len(rows), -1)
        want = ref[k].reshape(len(rows), -1)
        assert np.isfinite(got).all(), (case, k, "non-finite rows", np.asarray(rows)[~np.isfinite(got).all(1)][:8])
        err = np.abs(got - want).max(1)
        worst[k] = float(err.max())
        if worst[k] >= gate[k]:
            bad[k] = (worst[k], gate[k], "rows", [int(r) for r in np.asarray(rows)[np.argsort(-err)[:6]]], "oracle fp32", own32.get(k))
    _note(case, **{k: [worst[k], own32.get(k)] for k in worst}, rows=len(rows))
    assert not bad, (case, bad)
    return worst


def _finite(ctx, names, M):
    for k in names:
        v = ctx.view(k)[:M]
        assert bool(torch.isfinite(v).all()), (k, "non-finite values in rows [0, M)", (~torch.isfinite(v).reshape(M, -1).all(1)).nonzero().flatten()[:8])


def _names(use_deform, color, split=False):
    """(the split-precision VJP sweep does not compute the time adjoint: no tbar there)"""
    return ["xc", "sdf", "gc", "go"] + (["v"] + ([] if split else ["tbar"]) if use_deform else []) + (["feat", "rgb"] if color else [])


def _launch(eng, weff, packed, pts, flags, m_color=0, poison=None, split=False, infer_min=1):
    """``split``: the launch goes through the split-precision family (shapes_util.split_chain, restored behind the call), and did:
    Engine.point_forward's routing condition holds on the arguments, the context carries the split weights, and with ES_PF_SAVE it is
    marked as the split training chain's."""
    from endosurf_amd import _lib
    if poison is not None:          # the workspace starts from ``poison`` in every word instead of whatever torch.empty returns
        plain = eng.empty
        eng.empty = lambda *s, **k: plain(*s, **k).fill_(poison)
    try:
        with split_chain(eng, split, infer_min):
            routed = routes_split(eng, pts.M, bool(flags & _lib.PF_SAVE))
            ctx = eng.point_forward(pts, weff, packed, flags, m_color)
    finally:
        if poison is not None:
            del eng.empty
    torch.cuda.synchronize()
    if split:
        assert routed and ctx.px3 is not None and ctx.x3_chain == bool(flags & _lib.PF_SAVE), (routed, ctx.x3_chain)
    return ctx


def _screened(key, M, seed, use_deform, screen=None, mode="trained"):
    """shapes_util.inputs, cached: (x, d, t, number of redrawn points)."""
    if key not in _ORACLE:
        n = [0]
        x, d, t, *_ = inputs(M, seed, use_deform, screen=screen, mode=mode, count=n)
        _ORACLE[key] = (x, d, t, n[0])
    return _ORACLE[key]


def _dense(mode, use_deform, M, color, save=True, poison=None, split=False):
    eng, weff, packed, net = _setup(mode, use_deform)
    x, d, t, redrawn = _screened(("dense_in", mode, use_deform, M), M, 7000 + M, use_deform, mode=mode)
    dev = lambda a: a.cuda().contiguous()
    ctx = _launch(eng, weff, packed, eng.points(x=dev(x), t=dev(t), dirs=dev(d)), _flags(use_deform, color, save), poison=poison, split=split)
    ref, own32 = _reference(("dense", mode, use_deform, M), net, x, d, t, True)          # (without colour: the same buffers but feat / rgb)
    case = f"A_dense_{mode}_{int(use_deform)}_{M}_{int(color)}" + ("" if save else "_nosave") + ("" if poison is None else "_poison")
    case = "X3_" * split + case
    _note(case, redrawn=redrawn)
    _compare(case, ctx, ref, own32, np.arange(M), names=_names(use_deform, color, split))
    return ctx


@pytest.mark.parametrize("use_deform", [True, False])
@pytest.mark.parametrize("M", [1, 63, 64, 65, 127, 128, 129, 1024, 1100, 1400])
@pytest.mark.parametrize("color", [True, False])
def test_point_forward_dense(use_deform, M, color):
    """Every pad-row count of the 128-row workspace and of the 64-row colour launch, 16 / 18 / 22 deformation tiles beyond one round."""
    _dense("trained", use_deform, M, color)


@pytest.mark.parametrize("M", [65, 1100])
def test_point_forward_dense_init_weights(M):
    _dense("init", True, M, True)


@pytest.mark.parametrize("use_deform", [True, False])
@pytest.mark.parametrize("M", [65, 1100])
def test_point_forward_without_save(use_deform, M):
    """The no-grad layout (no ES_PF_SAVE: other offsets, no streamed activations): the same gates.  Whether it is bit-identical to the
    ES_PF_SAVE run is reported, not asserted: nothing in the library promises it."""
    a = _dense("trained", use_deform, M, True, save=False)
    b = _dense("trained", use_deform, M, True, save=True)
    _note(f"A_dense_trained_{int(use_deform)}_{M}_1_nosave",
          bit_identical_to_save={k: bool(torch.equal(a.view(k), b.view(k))) for k in _names(use_deform, True)})


@pytest.mark.parametrize("poison", [None, float("nan")])
def test_point_forward_workspace_history(poison):
    """M = 65 right behind M = 1400 on one engine: recycled memory, or a workspace filled with NaN before the launch."""
    _dense("trained", True, 1400, True)
    _dense("trained", True, 65, True, poison=poison)


def _subset_rows(M, seed, n_random=1400):
    """~2 000 rows: the first and last 130, 64 rows around every multiple of 16 384, the rest drawn at random."""
    rng = np.random.default_rng(seed)
    K = set(range(min(130, M))) | set(range(max(M - 130, 0), M))
    for b in range(16384, M, 16384):
        K |= set(range(b - 32, min(b + 32, M)))
    K |= set(int(i) for i in rng.integers(0, M, size=n_random))
    return np.array(sorted(K))


LARGE = {          # M, m_color, use_deform
    "ragged_20031": (20031, 0, True),
    "train_68608_deform": (65536 + 3072, 65536, True),
    "train_68608_nodeform": (65536 + 3072, 65536, False),
}


def _large_inputs(name):
    M, m_color, use_deform = LARGE[name]
    K = _subset_rows(M, 11)
    if 0 < m_color < M:
        K = np.array(sorted(set(K) | set(range(m_color - 64, m_color + 64))))
    x, d, t, redrawn = _screened(("large_in", name), M, 8000 + M, use_deform, screen=K)
    return M, m_color, use_deform, K, x, d, t, redrawn


def _compare_large(case, name, ctx, net, K, x, d, t, m_color, use_deform, redrawn, split=False, tail_names=None):
    """Rows K of a launch with a colour-less tail behind ``m_color`` coloured rows: the coloured rows against the oracle with colour,
    the tail rows against the oracle without (``tail_names``: their buffers, default those of the coloured rows but feat / rgb)."""
    M = x.shape[0]
    n_color = m_color if 0 < m_color < M else M
    Kc, Kt = K[K < n_color], K[K >= n_color]
    _note(case, redrawn=redrawn)
    ref, own32 = _reference(("large", name, "colour"), net, x[Kc], d[Kc], t[Kc], True)
    _compare(case + "_colour", ctx, ref, own32, Kc, names=_names(use_deform, True, split))
    if len(Kt):
        ref, own32 = _reference(("large", name, "tail"), net, x[Kt], d[Kt], t[Kt], False)
        _compare(case + "_tail", ctx, ref, own32, Kt, names=tail_names or _names(use_deform, False, split))
    _finite(ctx, _names(use_deform, False, split), M)
    _finite(ctx, ["feat", "rgb"], n_color)


@pytest.mark.parametrize("name,save", [(n, True) for n in LARGE] + [("ragged_20031", False), ("train_68608_deform", False)])
def test_point_forward_large(name, save):
    """20 031 rows (ragged last tile of every launch) and the fused training launch 65 536 + 3 072 with a colour-less tail: the tail's
    half-height deformation tiles in front, its [sdf + vjp] tiles inside the main deformation launch (without a deformation network: its
    SDF tiles at the head of the colour launch).  With and without ES_PF_SAVE."""
    M, m_color, use_deform, K, x, d, t, redrawn = _large_inputs(name)
    eng, weff, packed, net = _setup("trained", use_deform)
    dev = lambda a: a.cuda().contiguous()
    ctx = _launch(eng, weff, packed, eng.points(x=dev(x), t=dev(t), dirs=dev(d)), _flags(use_deform, True, save), m_color)
    _compare_large(f"A_large_{name}" + ("" if save else "_nosave"), name, ctx, net, K, x, d, t, m_color, use_deform, redrawn)


ROWS_ORDER = {"forward": [(65536, 1024), (66560, 2048)], "reverse": [(66560, 2048), (65536, 1024)]}


@pytest.mark.parametrize("use_deform,order", [(True, "forward"), (True, "reverse"), (False, "forward")])
def test_point_forward_rows_training_layout(use_deform, order):
    """es_point_forward_rows on a workspace laid out for 65 536 + 3 072 rows that starts as NaN: the main part, then the colour-less tail
    in two 64-aligned pieces (half-height bodies), in either order.  Tail rows against the oracle; the main rows are bit-for-bit what
    they were before the tail calls."""
    from endosurf_amd.engine import PointCtx
    name = "train_68608_deform" if use_deform else "train_68608_nodeform"
    M, m_color, use_deform, K, x, d, t, redrawn = _large_inputs(name)
    eng, weff, packed, net = _setup("trained", use_deform)
    dev = lambda a: a.cuda().contiguous()
    ctx = PointCtx(eng, eng.points(x=dev(x), t=dev(t), dirs=dev(d)), _flags(use_deform, True), m_color)
    ctx.ws.fill_(float("nan"))
    eng.point_forward_rows(ctx, weff, packed, 0, m_color)
    torch.cuda.synchronize()
    names = _names(use_deform, True)
    before = {k: ctx.view(k)[:m_color].clone() for k in names}
    assert bool(torch.isnan(ctx.view("sdf")[m_color:]).all()), "the main part wrote tail rows"
    for i, (row0, nrows) in enumerate(ROWS_ORDER[order]):
        eng.point_forward_rows(ctx, weff, packed, row0, nrows)
        torch.cuda.synchronize()
        if i == 0:
            other = ROWS_ORDER[order][1]
            assert bool(torch.isnan(ctx.view("sdf")[other[0]:other[0] + other[1]]).all()), "a tail piece wrote rows of the other piece"
    for k in names:
        assert torch.equal(ctx.view(k)[:m_color], before[k]), (k, "main rows changed by the tail calls")
    _compare_large(f"A_rows_{name}_{order}", name, ctx, net, K, x, d, t, m_color, use_deform, redrawn)


@pytest.mark.parametrize("use_deform", [True, False])
@pytest.mark.parametrize("tail", [64, 192])
def test_point_forward_rows_short_tail(use_deform, tail):
    """m_color = 256 with a 64- and a 192-row tail (4 / 12 half-height deformation tiles, 2 / 6 [sdf + vjp] half tiles): oracle on all
    rows, through es_point_forward (the fused layout) and through es_point_forward_rows (main part, then the tail)."""
    from endosurf_amd.engine import PointCtx
    mc, M = 256, 256 + tail
    eng, weff, packed, net = _setup("trained", use_deform)
    n = [0]
    x, d, t, *_ = inputs(M, 9000 + M, use_deform, count=n)
    dev = lambda a: a.cuda().contiguous()
    pts = eng.points(x=dev(x), t=dev(t), dirs=dev(d))
    fused = _launch(eng, weff, packed, pts, _flags(use_deform, True), mc, poison=float("nan"))
    rows = PointCtx(eng, pts, _flags(use_deform, True), mc)
    rows.ws.fill_(float("nan"))
    eng.point_forward_rows(rows, weff, packed, 0, mc)
    eng.point_forward_rows(rows, weff, packed, mc, tail)
    torch.cuda.synchronize()
    refc, ownc = _reference(("tail", use_deform, M, "colour"), net, x[:mc], d[:mc], t[:mc], True)
    reft, ownt = _reference(("tail", use_deform, M, "tail"), net, x[mc:], d[mc:], t[mc:], False)
    for label, ctx in (("fused", fused), ("rows", rows)):
        case = f"A_tail_{int(use_deform)}_{M}_{label}"
        _note(case, redrawn=n[0])
        _compare(case + "_colour", ctx, refc, ownc, np.arange(mc))
        _compare(case + "_tail", ctx, reft, ownt, np.arange(mc, M))


# ---- point sources ---------------------------------------------------------------------------------------------------------
def _ray_set(N, seed):
    """Rays [N, 9] (fp32) inside the unit sphere: origins in [-0.3, 0.3]^3, unit directions of any orientation -- every third one with
    d.z < 0, rays 1 and 2 (if present) with d.z = +1e-3 / -1e-3 -- one time per ray; zmax [N]: the depth up to which o + d / (d.z + 1e-6) z
    stays inside [-0.75, 0.75]^3."""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-0.3, 0.3, size=(N, 3))
    d = rng.normal(size=(N, 3)); d /= np.linalg.norm(d, axis=-1, keepdims=True)
    d[:, 2] = np.where(np.abs(d[:, 2]) < 0.05, 0.05, d[:, 2])
    d[::3, 2] = -np.abs(d[::3, 2])
    for i, dz in ((1, 1e-3), (2, -1e-3)):
        if i < N:
            d[i, 2] = dz
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    for i, dz in ((1, 1e-3), (2, -1e-3)):
        if i < N:
            d[i, 2] = dz
    rays = np.concatenate([o, d, np.zeros((N, 2)), rng.uniform(size=(N, 1))], -1).astype(np.float32)
    r64 = torch.from_numpy(rays).double()
    zmax = 0.45 / O.d_over_z(r64[:, 3:6]).abs().max(-1)[0]
    return torch.from_numpy(rays), zmax, rng


def _ray_points(rays, z):
    """The point source's arithmetic in fp64 (chain_common.h load_point = reference endosurf.py:66, :87, :153) on the fp32 inputs."""
    r = rays.double()
    N, n = z.shape
    x = r[:, None, :3] + O.d_over_z(r[:, 3:6])[:, None, :] * z.double()[:, :, None]
    return x.reshape(-1, 3), r[:, None, 3:6].expand(N, n, 3).reshape(-1, 3), r[:, None, 8].expand(N, n).reshape(-1)


def _screened_z(net, rays, zmax, N, n, rng, rows=None):
    """z [N, n] (fp32, unsorted: the point source does not care) with every sample -- or the samples with flat index in ``rows`` --
    redrawn until its point keeps RELU_MARGIN from every ReLU kink."""
    z = torch.from_numpy(rng.uniform(size=(N, n))).double() * zmax[:, None]
    z = z.float()
    rows = torch.arange(N * n) if rows is None else torch.as_tensor(np.asarray(rows, np.int64))
    redrawn = 0
    for _ in range(64):
        x, d, t = _ray_points(rays, z)
        near = rows[relu_margin(net, x[rows], d[rows], t[rows][:, None]) < RELU_MARGIN]
        if near.numel() == 0:
            return z, redrawn
        redrawn += near.numel()
        z.view(-1)[near] = (torch.from_numpy(rng.uniform(size=near.numel())).double() * zmax[near // n]).float()
    raise AssertionError("could not place the samples away from the ReLU kinks")


RAY_SAMPLES = [(1, 77), (32, 7), (64, 5), (100, 7), (128, 3)]


def _ray_samples(n, N, use_deform, split=False, save=True):
    eng, weff, packed, net = _setup("trained", use_deform)
    rays, zmax, rng = _ray_set(N, 300 + n)
    z, redrawn = _screened_z(net, rays, zmax, N, n, rng)
    ldz, col0 = n + 9, 5
    zfull = torch.from_numpy(rng.uniform(-5.0, 5.0, size=(N, ldz)).astype(np.float32))          # what a wrong stride would read: far outside
    zfull[:, col0:col0 + n] = z
    rays_d, z_d = rays.cuda().contiguous(), zfull.cuda().contiguous()
    pts = eng.points(rays=rays_d, z=z_d, n_per_ray=n, ldz=ldz)
    pts.z = C.c_void_p(z_d.data_ptr() + 4 * col0)
    ctx = _launch(eng, weff, packed, pts, _flags(use_deform, True, save), poison=float("nan"), split=split)
    x, d, t = _ray_points(rays, z)
    ref, own32 = _reference(("mode1", use_deform, n, N), net, x, d, t, True)
    case = "X3_" * split + f"A_mode1_{int(use_deform)}_{n}x{N}" + ("" if save else "_nosave")
    _note(case, redrawn=redrawn)
    _compare(case, ctx, ref, own32, np.arange(N * n), names=_names(use_deform, True, split))


@pytest.mark.parametrize("use_deform", [True, False])
@pytest.mark.parametrize("n,N", RAY_SAMPLES)
def test_point_source_ray_samples(n, N, use_deform):
    """Mode 1: z is a column window [5, 5 + n) of a wider array (ldz = n + 9), n is or is not a multiple of a tile, N n is not a multiple
    of 128 (n = 128 aside); rays with d.z < 0 and |d.z| = 1e-3."""
    _ray_samples(n, N, use_deform)


def _samples_then_points_small(use_deform, split=False, save=True):
    eng, weff, packed, net = _setup("trained", use_deform)
    N, n, Ma, mc = 7, 32, 37, 192
    rays, zmax, rng = _ray_set(N, 411)
    z, redrawn = _screened_z(net, rays, zmax, N, n, rng)
    cnt = [0]
    xa, _, ta, *_ = inputs(Ma, 412, use_deform, count=cnt)
    rays_d, z_d = rays.cuda().contiguous(), z.cuda().contiguous()
    pts = eng.points(rays=rays_d, z=z_d, n_per_ray=n, x=xa.cuda().contiguous(), t=ta.cuda().contiguous())
    assert (pts.mode, pts.M_split, pts.M) == (2, N * n, N * n + Ma)
    ctx = _launch(eng, weff, packed, pts, _flags(use_deform, True, save), mc, poison=float("nan"), split=split)
    xs, ds, ts = _ray_points(rays, z)
    dflt = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64).expand(Ma, 3)          # explicit points of mode 2 carry no direction
    x, d, t = torch.cat([xs, xa.double()]), torch.cat([ds, dflt]), torch.cat([ts, ta.double()])
    key = f"A_mode2_small_{int(use_deform)}"
    case = "X3_" * split + key + ("" if save else "_nosave")
    _note(case, redrawn=redrawn + cnt[0])
    ref, own32 = _reference((key, "colour"), net, x[:mc], d[:mc], t[:mc], True)
    _compare(case + "_colour", ctx, ref, own32, np.arange(mc), names=_names(use_deform, True, split))
    ref, own32 = _reference((key, "tail"), net, x[mc:], d[mc:], t[mc:], False)
    _compare(case + "_tail", ctx, ref, own32, np.arange(mc, N * n + Ma), names=_names(use_deform, False, split))


@pytest.mark.parametrize("use_deform", [True, False])
def test_point_source_samples_then_points_small(use_deform):
    """Mode 2: 7 x 32 ray samples followed by 37 explicit points, 192 of the samples coloured (the tail holds samples AND points)."""
    _samples_then_points_small(use_deform)


def _training_step_layout(split=False, save=True, tail_names=None):
    eng, weff, packed, net = _setup("trained", True)
    N, n, Ma = 1024, 64, 3072
    M = N * n + Ma
    K = _subset_rows(M, 13)
    K = np.array(sorted(set(K) | set(range(N * n - 64, N * n + 64))))
    Ks, Ka = K[K < N * n], K[K >= N * n] - N * n
    rays, zmax, rng = _ray_set(N, 421)
    z, redrawn = _screened_z(net, rays, zmax, N, n, rng, rows=Ks)
    cnt = [0]
    xa, _, ta, *_ = inputs(Ma, 422, True, screen=Ka, count=cnt)
    pts = eng.points(rays=rays.cuda().contiguous(), z=z.cuda().contiguous(), n_per_ray=n, x=xa.cuda().contiguous(), t=ta.cuda().contiguous())
    ctx = _launch(eng, weff, packed, pts, _flags(True, True, save), N * n, split=split)
    xs, ds, ts = _ray_points(rays, z)
    key = "A_mode2_train"
    case = "X3_" * split + key + ("" if save else "_nosave")
    _note(case, redrawn=redrawn + cnt[0])
    ref, own32 = _reference((key, "colour"), net, xs[Ks], ds[Ks], ts[Ks], True)
    _compare(case + "_colour", ctx, ref, own32, Ks, names=_names(True, True, split))
    dflt = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64).expand(len(Ka), 3)
    ref, own32 = _reference((key, "tail"), net, xa[Ka].double(), dflt, ta[Ka].double(), False)
    _compare(case + "_tail", ctx, ref, own32, Ka + N * n, names=tail_names or _names(True, False, split))
    _finite(ctx, _names(True, False, split), M)
    _finite(ctx, ["feat", "rgb"], N * n)


def test_point_source_training_step_layout():
    """Mode 2 at the size of every training step: 1 024 x 64 ray samples (all coloured) followed by 3 072 explicit points."""
    _training_step_layout()


def _shared_time(use_deform, split=False, save=True):
    eng, weff, packed, net = _setup("trained", use_deform)
    M, rng = 333, np.random.default_rng(431)
    t0 = torch.tensor([0.3125])
    x, d, *_ = inputs(M, 432, use_deform)
    redrawn = 0
    for _ in range(64):
        near = (relu_margin(net, x.double(), d.double(), t0.double().expand(M)[:, None]) < RELU_MARGIN).nonzero().flatten()
        if near.numel() == 0:
            break
        redrawn += near.numel()
        x[near] = torch.from_numpy(rng.uniform(-0.7, 0.7, size=(near.numel(), 3)).astype(np.float32))
    else:
        raise AssertionError("could not place the points away from the ReLU kinks")
    pts = eng.points(x=x.cuda().contiguous(), t=t0.cuda(), dirs=d.cuda().contiguous())
    assert pts.t_scalar == 1
    ctx = _launch(eng, weff, packed, pts, _flags(use_deform, True, save), poison=float("nan"), split=split)
    ref, own32 = _reference(("tscalar", use_deform), net, x, d, t0.expand(M), True)
    case = "X3_" * split + f"A_tscalar_{int(use_deform)}" + ("" if save else "_nosave")
    _note(case, redrawn=redrawn)
    _compare(case, ctx, ref, own32, np.arange(M), names=_names(use_deform, True, split))


@pytest.mark.parametrize("use_deform", [True, False])
def test_point_source_shared_time(use_deform):
    """Mode 0 with t_scalar = 1: one time value for all 333 points (renderonpts' shared-time form)."""
    _shared_time(use_deform)


# ------------------------------------------------------------------------------------------------------------------------------
# B. es_query_sdf_rays: strided output, ray_done tile skip
# ------------------------------------------------------------------------------------------------------------------------------
SENTINEL = -12345.6787109375          # exactly representable; no SDF value comes near it


def _query_rays(eng, weff, packed, use_deform, rays_d, z_d, col0, B, out, done):
    from endosurf_amd import _lib
    N = rays_d.shape[0]
    p = eng.points(rays=rays_d, z=z_d, n_per_ray=B, ldz=z_d.shape[1])
    p.z = C.c_void_p(z_d.data_ptr() + 4 * col0)
    _lib.check(eng.lib.es_query_sdf_rays(C.byref(p), _lib.ptr(packed), _lib.ptr(weff), C.c_void_p(out.data_ptr() + 4 * col0), out.shape[1],
                                         _lib.ptr(done) if done is not None else None, int(use_deform), eng.st()), "es_query_sdf_rays")
    torch.cuda.synchronize()


def _done_pattern(name, N):
    done = np.zeros(N, np.int32)
    if name == "all":
        done[:] = 1
    elif name == "alternating_rays":
        done[1::2] = 1
    elif name == "alternating_pairs":
        done[(np.arange(N) // 2) % 2 == 1] = 1
    elif name == "one_live_in_last_tile":
        done[:] = 1
        done[N - 1] = 0
    else:
        assert name == "none"
    return done


QUERY_CASES = {          # N, B, first column, ld_out, use_deform: tile height 32 (redirected from 16) | 32 | 64 (two rays per tile) | 64 (0.64 rays per tile)
    "96x32": (96, 32, 64, 128, True), "400x32": (400, 32, 32, 128, True), "400x32_nodeform": (400, 32, 96, 128, False),
    "1024x32": (1024, 32, 64, 128, True), "300x100": (300, 100, 28, 128, True),
}


@pytest.mark.parametrize("pattern", ["none", "all", "alternating_rays", "alternating_pairs", "one_live_in_last_tile"])
@pytest.mark.parametrize("name", list(QUERY_CASES))
def test_query_sdf_rays(name, pattern):
    """The B proposals [col0, col0 + B) of every ray into columns [col0, col0 + B) of a [N, 128] buffer that holds a sentinel: written
    columns against OracleNet.sdf_observed (<= 4 096 sampled points), every other column still the sentinel bit for bit.  With
    ray_done: live rays hold the oracle's values, finished rays the sentinel or the correct value, nothing else."""
    N, B, col0, ld, use_deform = QUERY_CASES[name]
    eng, weff, packed, net = _setup("trained", use_deform)
    rays, zmax, rng = _ray_set(N, 500 + N + B)
    zfull = (torch.from_numpy(rng.uniform(size=(N, ld))).double() * zmax[:, None]).float()
    key = ("query", name)
    if key not in _ORACLE:
        pick = np.sort(rng.choice(N * B, size=min(4096, N * B), replace=False))
        x, _, t = _ray_points(rays, zfull[:, col0:col0 + B])
        with torch.no_grad():
            _ORACLE[key] = (pick, net.sdf_observed(x[pick], t[pick][:, None])[:, 0].numpy())
    pick, ref = _ORACLE[key]
    rays_d, z_d = rays.cuda().contiguous(), zfull.cuda().contiguous()
    tile = 32 if N * B <= 16384 else 64
    done = _done_pattern(pattern, N)
    out = torch.full((N, ld), SENTINEL, device="cuda")
    _query_rays(eng, weff, packed, use_deform, rays_d, z_d, col0, B, out, None if pattern == "none" else torch.from_numpy(done).cuda())
    got = out.cpu()
    bits = lambda a: a.contiguous().view(torch.int32)
    sent = bits(torch.full((1,), SENTINEL))[0]
    outside = torch.ones(ld, dtype=torch.bool); outside[col0:col0 + B] = False
    assert bool((bits(got)[:, outside] == sent).all()), "columns outside [col0, col0 + B) were written"
    win = got[:, col0:col0 + B]
    is_sent = bits(win) == sent
    live = torch.from_numpy(done == 0)
    assert not bool(is_sent[live].any()), ("live rays with unwritten proposals", is_sent[live].any(1).nonzero().flatten()[:8])
    if pattern == "all":
        assert bool(is_sent.all()), "every ray is finished: nothing may be written"
    # sampled points: the oracle's value (live rays: always; finished rays: unless the tile was skipped)
    v = win.reshape(-1)[pick].double().numpy()
    s = is_sent.reshape(-1)[pick].numpy()
    pick_live = live.numpy()[pick // B]
    err = np.abs(v - ref)
    assert not s[pick_live].any()
    worst = float(err[~s].max()) if (~s).any() else 0.0
    _note(f"B_{name}_{pattern}", sdf=worst, compared=int((~s).sum()), skipped_rays=int(is_sent.all(1).sum()))
    assert worst < 1e-5, worst
    if pattern != "none":
        # extra (kernel against kernel): whatever a finished ray holds besides the sentinel is the value of the run without ray_done
        full = torch.full((N, ld), SENTINEL, device="cuda")
        _query_rays(eng, weff, packed, use_deform, rays_d, z_d, col0, B, full, None)
        fw = full.cpu()[:, col0:col0 + B]
        assert bool((is_sent | (bits(win) == bits(fw))).all()), "a finished ray holds something that is neither the sentinel nor its value"
        # whole tiles of finished rays are skipped: the early exit is there (not a correctness property, but the point of the argument)
        if pattern in ("all", "one_live_in_last_tile"):
            assert int(is_sent.all(1).sum()) >= N - 1 - tile // min(B, tile)


# ------------------------------------------------------------------------------------------------------------------------------
# C. ray marching on synthetic profiles
# ------------------------------------------------------------------------------------------------------------------------------
TAUS = [0.0, 0.05, -0.05]


def _profiles(n, tau32, extra_at=()):
    """Rows of sdf - tau (exactly representable magnitudes, or exactly 0) -> sdf [R, n] fp32.  Crossings 'at section k' sit between
    samples k and k + 1."""
    P, M = 0.25, -0.375
    secs = sorted({k for k in (0, 30, 31, 32, 62, 63, 64, 94, 95, 96, n - 2) + tuple(extra_at) if 0 <= k <= n - 2})
    rows = []

    def row(fill):
        return np.full(n, fill, np.float64)
    for k in secs:
        r = row(P); r[k + 1:] = M; rows.append(r)                                   # outside -> inside at k: a hit
        r = row(M); r[k + 1:] = P; rows.append(r)                                   # first proposal occupied
        r = row(P); r[k + 1:] = M; r[min(k + 3, n):] = P; r[min(k + 6, n):] = M     # several crossings: the first wins
        rows.append(r)
        r = row(P); r[k + 1:] = M; r[k] = 0.0; rows.append(r)                       # an exact 0 in front of the change: product 0, no change there
        r = row(P); r[k + 1:] = M; r[k + 1] = 0.0; rows.append(r)                   # ... behind it
        if k >= 2:
            r = row(P); r[1] = 0.0; r[2:] = M; r[k + 1:] = P; rows.append(r)        # in through an exact 0, then inside -> outside first: no hit
            r = row(P); r[1] = 0.0; r[2:] = M; r[k + 1:] = P; r[min(k + 4, n):] = M; rows.append(r)
    for c in (P, M, 0.0):
        rows.append(row(c))
    r = row(P); r[0] = 0.0; r[n // 2:] = M; rows.append(r)                          # first proposal exactly on the surface: occupied
    u = np.stack(rows)
    sdf = (u + float(tau32)).astype(np.float32)
    sdf[u == 0.0] = tau32
    if tau32 == 0.0:
        sdf[-1, 0] = -0.0
        sdf[-2, ::2] = -0.0          # the all-zero profile with both signs of zero
    return sdf


def _dprop(R, n):
    return (0.5 + np.arange(R)[:, None] / 1024.0 + np.arange(n)[None, :] / 128.0).astype(np.float32)


def _march_find(eng, sdf, dprop, tau):
    from endosurf_amd import _lib
    N, n = sdf.shape
    sdf_d, dp_d = torch.from_numpy(sdf).cuda().contiguous(), torch.from_numpy(dprop).cuda().contiguous()
    state, flags, d_pred = eng.empty(N, 4).fill_(float("nan")), eng.empty(N, dtype=torch.int32).fill_(-1), eng.empty(N).fill_(float("nan"))
    _lib.check(eng.lib.es_march_find(_lib.ptr(sdf_d), _lib.ptr(dp_d), N, n, float(tau), _lib.ptr(state), _lib.ptr(flags), _lib.ptr(d_pred), eng.st()),
               "es_march_find")
    d_out = eng.empty(N, 1).fill_(float("nan"))
    _lib.check(eng.lib.es_march_finish(_lib.ptr(d_pred), _lib.ptr(flags), N, _lib.ptr(d_out), eng.st()), "es_march_finish")
    torch.cuda.synchronize()
    return state.cpu(), flags.cpu(), d_pred.cpu(), d_out.cpu()[:, 0]


def _bracket64(sdf, dprop, tau32):
    """oracle.march_bracket on the fp32 inputs: val = -(sdf - tau) (endosurf.py:375)."""
    val = -(torch.from_numpy(sdf).double() - float(tau32))
    return O.march_bracket(val, torch.from_numpy(dprop).double())


def _check_find(got, want, what):
    state, flags, d_pred, d_out = got
    mask, m0, d_low, f_low, d_high, f_high = want
    want_flags = mask.to(torch.int32) + 2 * m0.to(torch.int32)
    assert torch.equal(flags, want_flags), (what, "flags", (flags != want_flags).nonzero().flatten()[:8], flags[flags != want_flags][:8],
                                            want_flags[flags != want_flags][:8])
    ref_state = torch.stack([d_low, f_low, d_high, f_high], -1)[mask]
    assert float((state[mask].double() - ref_state).abs().max()) < 1e-6 if mask.any() else True, (what, "state")
    ref_pred = O.secant_estimate(d_low, f_low, d_high, f_high)[mask]
    if mask.any():
        assert float(((d_pred[mask].double() - ref_pred).abs() / ref_pred.abs().clamp(min=1.0)).max()) < 2e-6, (what, "d_pred")
    ref_out = torch.where(mask, O.secant_estimate(d_low, f_low, d_high, f_high), torch.full_like(d_low, float("inf")))
    ref_out[~m0] = 0.0
    assert torch.equal(torch.isinf(d_out), torch.isinf(ref_out)) and torch.equal(d_out == 0, ref_out == 0), (what, "inf / 0 pattern")
    assert bool((d_out[mask] == d_pred[mask]).all())


@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("n", [2, 3, 64, 65, 66, 128, 129, 200])
def test_march_find_synthetic(n, tau):
    """es_march_find + es_march_finish against oracle.march_bracket: first crossing at section 0, 62, 63, 64, n - 2 (one lane's stride
    ends at 63 | 64), several crossings, inside -> outside first, first proposal occupied, exact zeros (product 0 is no sign change),
    constant profiles, -0.0; 1, 3, 4, 5 and 257 rays (four waves per workgroup)."""
    eng = _setup("trained", True)[0]
    tau32 = np.float32(tau)
    base = _profiles(n, tau32)
    for N in (1, 3, 4, 5, 257):
        idx = (np.arange(N) * 7 + N) % len(base) if N < len(base) else np.arange(N) % len(base)
        sdf, dprop = base[idx], _dprop(N, n)
        _check_find(_march_find(eng, sdf, dprop, tau32), _bracket64(sdf, dprop, tau32), (n, tau, N))
    # every profile once
    sdf, dprop = base, _dprop(len(base), n)
    want = _bracket64(sdf, dprop, tau32)
    _check_find(_march_find(eng, sdf, dprop, tau32), want, (n, tau, "all"))
    if n >= 3:
        assert bool(want[0].any()) and bool((~want[0] & want[1]).any()) and bool((~want[1]).any())          # hits, misses and occupied starts


@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("n_valid", [32, 64, 96])
def test_march_progress_synthetic(n_valid, tau):
    """es_march_progress at n = 128 in blocks of 32: ``done`` equals its definition (first proposal occupied, or a sign change among the
    first n_valid proposals), AND for every finished ray es_march_find gives the same result on the profile whose columns >= n_valid read
    0.0 (what the block path leaves there) as on the full profile -- the property the early exit rests on, for tau != 0 as well."""
    from endosurf_amd import _lib
    eng = _setup("trained", True)[0]
    n, tau32 = 128, np.float32(tau)
    sdf = _profiles(n, tau32, extra_at=(n_valid - 3, n_valid - 2, n_valid - 1, n_valid))
    N = sdf.shape[0]
    dprop = _dprop(N, n)
    sdf_d = torch.from_numpy(sdf).cuda().contiguous()
    done = eng.empty(N, dtype=torch.int32).fill_(-1)
    _lib.check(eng.lib.es_march_progress(_lib.ptr(sdf_d), N, n, n_valid, float(tau32), _lib.ptr(done), eng.st()), "es_march_progress")
    torch.cuda.synchronize()
    val = -(torch.from_numpy(sdf).double() - float(tau32))
    want = ((val[:, :n_valid - 1] * val[:, 1:n_valid]) < 0).any(1) | ~(val[:, 0] < 0)
    assert torch.equal(done.cpu() != 0, want), ("done", (done.cpu().bool() != want).nonzero().flatten()[:8])
    assert bool(want.any()) and bool((~want).any())
    cut = sdf.copy(); cut[:, n_valid:] = 0.0
    full64, cut64 = _bracket64(sdf, dprop, tau32), _bracket64(cut, dprop, tau32)
    fin = want
    assert torch.equal(full64[0][fin], cut64[0][fin]) and torch.equal(full64[1][fin], cut64[1][fin]), "the early exit changes the oracle's result"
    hit = fin & full64[0]
    for a, b in zip(full64[2:], cut64[2:]):
        assert torch.equal(a[hit], b[hit])
    got_full, got_cut = _march_find(eng, sdf, dprop, tau32), _march_find(eng, cut, dprop, tau32)
    _check_find(got_full, full64, ("progress full", n_valid, tau))
    assert torch.equal(got_full[1][fin], got_cut[1][fin])
    assert torch.equal(got_full[0][hit], got_cut[0][hit]) and torch.equal(got_full[2][hit], got_cut[2][hit])
    assert torch.equal(got_full[3][fin], got_cut[3][fin])
    # (the profiles hold the critical ray: not finished, its first crossing in the section n_valid - 1 | n_valid, which the cut hides)
    edge = ~fin & full64[0] & (val[:, n_valid - 1] * val[:, n_valid] < 0)
    assert bool(edge.any()) and (tau != 0.0 or not bool(cut64[0][edge].any()))


@pytest.mark.parametrize("tau", [0.0, 0.05])
def test_secant_iterations_synthetic(tau):
    """es_secant_points + es_secant_update, eight iterations on the SDF of a sphere (evaluated here in fp64 at the kernel's points and
    rounded), against oracle.secant_step: f_mid = sdf - tau is NOT negated (unlike the bracket's values) and the points use d / d.z
    without the epsilon of the sampling code (endosurf.py:427)."""
    from endosurf_amd import _lib
    eng = _setup("trained", True)[0]
    tau32 = np.float32(tau)
    N, n = 261, 128
    rng = np.random.default_rng(77)
    rays = weightgen.make_rays(78, N)
    # |d.z| = 1e-3 (d / d.z differs from d / (d.z + 1e-6) by 1e-3): rays along +x / -x whose points o + s d / d.z cross the sphere for
    # s around 1.5e-3; and d.z < 0 (d / d.z is then the direction of -d)
    rays[3, :6], rays[4, :6] = [-1.5, 0.01, 0.02, 1.0, 0.0, 1e-3], [1.5, -0.02, 0.01, 1.0, 0.0, -1e-3]
    rays[5, 3:6] = -rays[5, 3:6]
    r64 = torch.from_numpy(rays).double()
    o, dz = r64[:, :3], r64[:, 3:6] / r64[:, 5:6]
    centre, radius = torch.tensor([0.02, -0.03, 0.05], dtype=torch.float64), 0.55
    f = lambda p: (p - centre).norm(dim=-1) - radius
    dprop = (0.8 + np.arange(n)[None, :] * (1.4 / 127) + rng.uniform(0, 0.005, size=(N, 1))).astype(np.float32)
    dprop[3:5] *= 1e-3
    sdf = f(o[:, None, :] + torch.from_numpy(dprop).double()[:, :, None] * dz[:, None, :]).float().numpy()
    state, flags, d_pred, _ = _march_find(eng, sdf, dprop, tau32)
    mask, m0, d_low, f_low, d_high, f_high = _bracket64(sdf, dprop, tau32)
    assert int(mask.sum()) > N // 2 and bool(mask[3:6].all())
    state_d, pred_d = state.cuda().contiguous(), d_pred.cuda().contiguous()
    rays_d = torch.from_numpy(rays).cuda().contiguous()
    x_d, t_d = eng.empty(N, 3), eng.empty(N)
    ref_pred = O.secant_estimate(d_low, f_low, d_high, f_high)
    worst_x = worst_d = 0.0
    for it in range(8):
        eng.secant_points(rays_d, pred_d, N, x_d, t_d)
        torch.cuda.synchronize()
        x = x_d.cpu().double()
        assert torch.equal(t_d.cpu(), torch.from_numpy(rays[:, 8]))
        x_ref = o + pred_d.cpu().double()[:, None] * dz
        ex = (x - x_ref).abs().max(-1)[0] / x_ref.abs().max(-1)[0].clamp(min=1.0)          # (every ray, hit or not)
        worst_x = max(worst_x, float(ex.max()))
        f_mid32 = f(x).float()                                              # "sdf" at the kernel's points; both sides see these numbers
        eng.secant_update(f_mid32.cuda().contiguous(), N, float(tau32), state_d, pred_d)
        torch.cuda.synchronize()
        d_low, f_low, d_high, f_high, ref_pred = O.secant_step(d_low, f_low, d_high, f_high, ref_pred, f_mid32.double() - float(tau32))
        ed = ((pred_d.cpu().double() - ref_pred).abs() / ref_pred.abs().clamp(min=1.0))[mask]
        worst_d = max(worst_d, float(ed.max()))
        es = (state_d.cpu().double() - torch.stack([d_low, f_low, d_high, f_high], -1)).abs()[mask]
        assert float(es.max()) < 1e-5, (it, "state", float(es.max()))
    _note(f"C_secant_tau{tau}", x=worst_x, d_pred=worst_d, hits=int(mask.sum()))
    assert worst_x < 1e-6 and worst_d < 1e-5, (worst_x, worst_d)


# ---- on the network, at training size -----------------------------------------------------------------------------------------
def _march_oracle(use_deform):
    """OracleRenderer.ray_marching in fp64 on 515 SyntheticScene rays (the first 512 serve the 512-ray cases: the rays do not
    interact) + its own fp32 run + the proposals' values of the fp64 run."""
    key = ("march", use_deform)
    if key not in _ORACLE:
        from endosurf_amd.trainer import SyntheticScene
        rays = SyntheticScene("cuda", seed=17).batch(515)["rays"].cpu()
        net = _setup("trained", use_deform)[3]
        seen = []
        plain = net.sdf_observed
        net.sdf_observed = lambda p, t: (seen.append(plain(p, t)), seen[-1])[1]
        try:
            d64 = O.OracleRenderer(net, RENDER_CFG).ray_marching(rays.double())[:, 0]
        finally:
            del net.sdf_observed
        val = -seen[0].reshape(515, 128)
        net32 = O.OracleNet({k: v.float() for k, v in net.p.items()}, use_deform)
        d32 = O.OracleRenderer(net32, RENDER_CFG).ray_marching(rays)[:, 0]
        _ORACLE[key] = (rays, d64, d32.double(), val)
    return _ORACLE[key]


@pytest.mark.parametrize("use_deform", [True, False])
@pytest.mark.parametrize("march_block", [32, 0])
@pytest.mark.parametrize("N", [512, 515])
def test_ray_marching_training_size(N, march_block, use_deform):
    """Engine.ray_marching against OracleRenderer.ray_marching in fp64: the block path with early exit (32-point tiles at 512 rays,
    64-point tiles at 515) and the one-launch path.  Rays on which fp32 and fp64 may legitimately disagree about a sign -- a proposal
    within 1e-5 of the surface up to the bracket -- are left out of the pattern comparison (a handful)."""
    eng, weff, packed, net = _setup("trained", use_deform)
    rays, d64, d32, val = (a[:N] for a in _march_oracle(use_deform))
    sign = torch.sign(val[:, :-1] * val[:, 1:])
    first = torch.where((sign < 0).any(1), (sign < 0).float().argmax(1) + 1, torch.full((N,), 127))          # last proposal that matters
    close = ((val.abs() < 1e-5) & (torch.arange(128)[None, :] <= first[:, None])).any(1)
    keep = ~close
    old = eng.march_block
    eng.march_block = march_block
    try:
        d = eng.ray_marching(rays.cuda().contiguous(), weff, packed, use_deform)
        torch.cuda.synchronize()
    finally:
        eng.march_block = old
    d = d.cpu()[:, 0].double()
    fin = torch.isfinite(d64) & (d64 != 0) & keep
    assert int(close.sum()) <= 8 and int(fin.sum()) >= N // 4, (int(close.sum()), int(fin.sum()))
    assert torch.equal(torch.isinf(d)[keep], torch.isinf(d64)[keep]) and torch.equal((d == 0)[keep], (d64 == 0)[keep])
    budget = 3 * float((d32 - d64)[fin].abs().max()) + 2e-5
    worst = float((d - d64)[fin].abs().max())
    _note(f"C_network_{int(use_deform)}_{N}_{march_block}", d=worst, budget=budget, excluded=int(close.sum()), hits=int(fin.sum()),
          misses=int(torch.isinf(d64).sum()), occupied=int((d64 == 0).sum()))
    assert worst < budget, (worst, budget)


# ------------------------------------------------------------------------------------------------------------------------------
# D. the sampling chain at other settings
# ------------------------------------------------------------------------------------------------------------------------------
def _sampling_rays():
    """33 rays: 30 of the synthetic camera + an origin inside the sphere (near clamps to 0), a ray that misses the sphere
    (near == far) and a camera behind the scene looking back (d.z < 0)."""
    rays = weightgen.make_rays(91, 33)
    rays[30, :6] = [0.1, -0.05, -0.2, 0.0, 0.0, 1.0]
    rays[31, :6] = [1.2, 0.0, -1.5, 0.0, 0.0, 1.0]
    rays[32, :6] = [0.05, 0.02, 1.5, 0.06, -0.08, -np.sqrt(1 - 0.06 ** 2 - 0.08 ** 2)]
    u = np.random.default_rng(92).uniform(size=(33, 1)).astype(np.float32)
    return torch.from_numpy(rays), torch.from_numpy(u)


def _qdiff(a, b, q):
    return float(np.quantile(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)), q))


def _sampling_oracle(use_deform, n, n_imp, steps):
    key = ("sampling", use_deform, n, n_imp, steps)
    if key not in _ORACLE:
        rays, u = _sampling_rays()
        net = _setup("trained", use_deform)[3]
        cfg = dict(RENDER_CFG, n_samples=n, n_importance=n_imp, up_sample_steps=steps)
        with torch.no_grad():
            t64 = O.OracleRenderer(net, cfg).sample_z(rays.double(), 0, u.double())[2]
            net32 = O.OracleNet({k: v.float() for k, v in net.p.items()}, use_deform)
            t32 = O.OracleRenderer(net32, cfg).sample_z(rays, 0, u)[2]
        _ORACLE[key] = ([a.numpy() for a in t64], [a.numpy() for a in t32])
    return _ORACLE[key]


def _check_trace(case, trace, t64, t32):
    assert len(trace) == len(t64)
    for i, zt in enumerate(trace):
        zt = zt.cpu().numpy()
        assert zt.shape == t64[i].shape, (i, zt.shape, t64[i].shape)
        assert np.isfinite(zt).all() and np.all(np.diff(zt, axis=1) >= 0), "z must stay finite and sorted"
        budget_q = 3 * _qdiff(t32[i], t64[i], 0.99) + 2e-6
        budget_max = 3 * np.max(np.abs(t32[i] - t64[i])) + 1e-4
        q, m = _qdiff(zt, t64[i], 0.99), float(np.max(np.abs(zt - t64[i])))
        _note(case, **{f"z{i}": [q, budget_q, m, budget_max]})
        assert q < budget_q and m < budget_max, (case, i, q, budget_q, m, budget_max)
        # the ray that misses the sphere (near == far): what the oracle's arithmetic gives -- all coarse z equal, zero-length sections
        spread64 = float(t64[i][31].max() - t64[i][31].min())
        if spread64 == 0.0:
            assert float(zt[31].max() - zt[31].min()) == 0.0


@pytest.mark.parametrize("use_deform", [True, False])
@pytest.mark.parametrize("n,n_imp,steps", [(64, 64, 4), (16, 16, 2), (32, 64, 1), (128, 128, 4), (128, 128, 2)])
def test_sampling_chain_settings(n, n_imp, steps, use_deform):
    """es_sample_z (one call) and the launch-by-launch chain against OracleRenderer.sample_z in fp64, with the oracle's own fp32 run as
    the budget (as test_sampling_trace): up to S = 256 samples (the per-ray kernels' limit) and 64 new samples per step (the up-sampling
    kernel's limit), one to four steps.  Both forms bit-equal."""
    eng, weff, packed, net = _setup("trained", use_deform)
    rays, u = _sampling_rays()
    rays_d, u_d = rays.cuda().contiguous(), u.cuda().reshape(-1).contiguous()
    t64, t32 = _sampling_oracle(use_deform, n, n_imp, steps)
    case = f"D_{int(use_deform)}_{n}_{n_imp}_{steps}"
    from endosurf_amd import _lib
    calls = _lib.calls
    z_one = eng.sample_z(rays_d, u_d, weff, packed, use_deform, n, n_imp, steps, True)
    assert _lib.calls - calls == 1, "the one-call form did not run"
    trace = []
    z_eager = eng.sample_z(rays_d, u_d, weff, packed, use_deform, n, n_imp, steps, True, trace=trace)
    torch.cuda.synchronize()
    assert tuple(z_one.shape) == (33, n + n_imp) and torch.equal(z_one, z_eager) and torch.equal(z_eager, trace[-1])
    assert t64[0][31].max() == t64[0][31].min() and np.isfinite(t64[-1]).all()          # (the missing ray is in the set)
    _check_trace(case, trace, t64, t32)
    near, far = eng.ray_setup(rays_d, None, n, 2.0 / n, 0, eng.empty(33, n), want_bounds=True)
    torch.cuda.synchronize()
    nr, fr = O.sphere_intersection(rays[:, :3].double(), rays[:, 3:6].double())
    assert float((near.cpu().double() - nr[:, 0]).abs().max()) < 1e-6 and float((far.cpu().double() - fr[:, 0]).abs().max()) < 1e-6
    assert float(nr[30]) == 0.0 and float(near[30]) == 0.0 and float(nr[31]) == float(fr[31]) and float(near[31]) == float(far[31])


@pytest.mark.parametrize("use_deform", [True, False])
def test_sampling_importance_not_a_multiple_of_the_steps(use_deform):
    """32 + 30 samples in 4 steps: the loop adds 4 x (30 // 4) = 28 samples (reference endosurf.py:95-110), so z has 60 columns -- the
    oracle's -- all of them written.  (Engine.sample_z used to return 62 columns, the last two uninitialised memory.)  The renderer itself
    refuses the configuration: every sample count it derives says 62, and the reference's render_rays raises on it as well."""
    eng, weff, packed, net = _setup("trained", use_deform)
    rays, u = _sampling_rays()
    rays_d, u_d = rays.cuda().contiguous(), u.cuda().reshape(-1).contiguous()
    t64, t32 = _sampling_oracle(use_deform, 32, 30, 4)
    assert t64[-1].shape == (33, 60)
    plain = eng.empty
    eng.empty = lambda *s, **k: plain(*s, **k).fill_(float("nan")) if k.get("dtype", torch.float32) == torch.float32 else plain(*s, **k)
    try:
        trace = []
        z = eng.sample_z(rays_d, u_d, weff, packed, use_deform, 32, 30, 4, True, trace=trace)
        z2 = eng.sample_z(rays_d, u_d, weff, packed, use_deform, 32, 30, 4, True)
        torch.cuda.synchronize()
    finally:
        del eng.empty
    assert tuple(z.shape) == (33, 60) and torch.equal(z, z2) and torch.equal(z, trace[-1])
    _check_trace(f"D_{int(use_deform)}_32_30_4", trace, t64, t32)
    with pytest.raises(ValueError):
        eng.sample_z(rays_d, u_d, weff, packed, use_deform, 32, 3, 4, True)          # 3 // 4 = 0 new samples per step
    from endosurf_amd import EndoSurfRenderer
    from gpu_util import net_cfg
    with pytest.raises(ValueError, match="multiple of up_sample_steps"):
        EndoSurfRenderer(dict(RENDER_CFG, n_importance=30), net_cfg(use_deform), device="cuda")


def test_upsample_step_rejects_sizes_before_launching():
    """ES_REQUIRE in front of the launch: n + n_imp > ld_out, n > 256 (the per-ray kernels' limit), n_imp > 64.  Status, no launch: the
    output buffers keep their sentinel."""
    eng = _setup("trained", True)[0]
    N = 4
    rays = torch.from_numpy(weightgen.make_rays(5, N)).cuda()
    big = lambda *s: torch.full(s, SENTINEL, device="cuda")
    z, sdf, z_new, z_out, src = big(N, 512), big(N, 512), big(N, 128), big(N, 512), torch.full((N, 512), -7, device="cuda", dtype=torch.int32)
    from endosurf_amd import _lib
    for n, n_imp, ld_out in ((32, 8, 39), (257, 8, 512), (64, 65, 512), (1, 8, 512), (32, 0, 512)):
        st = eng.lib.es_upsample_step(_lib.ptr(rays), _lib.ptr(z), 512, _lib.ptr(sdf), 512, N, n, n_imp, 64.0, _lib.ptr(z_new), _lib.ptr(z_out), ld_out,
                                      _lib.ptr(src), eng.st())
        assert st != 0, (n, n_imp, ld_out)
    torch.cuda.synchronize()
    assert bool((z_out == SENTINEL).all()) and bool((z_new == SENTINEL).all()) and bool((src == -7).all())
