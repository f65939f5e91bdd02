"""Every grouped problem of the weight-gradient GEMMs (csrc/wgrad.hip) against a plain fp64 contraction of the same operands.

es_point_backward_stages accepts the weight-gradient stage bits without ES_BWD_CHAINS and es_point_workspace_offset answers for every
buffer id, so a test can write each operand buffer of csrc/workspace.h itself and judge the contraction apart from the chains.

  A  EXACT on integers.  Operands are integers in {-3 .. 3} (wgrad_util.fill_integer; the padding follows the contract of workspace.h:
     zeros where it promises zeros, non-zero junk everywhere else).  Every partial sum is then an integer below 2^24 (9 x 206 k rows),
     exact in fp32 in any order, with atomics, and in split precision (small integers sit in the high bf16 plane): the library's result
     must EQUAL the fp64 reference.  Each case runs the three stage bits one by one (into a non-zero integer gradient: the call must add,
     and must leave every entry outside the stage's slices alone -- the reference knows that the last deformation layer rides with the
     SDF and colour launches) and all three at once from zero and once more on top, with fp32 atomics and in deterministic mode, on the
     fp32 and on the split-precision kernel.  Row counts: 1 and 128 (one row chunk); 800, 1024, 1100, 1400 (7 / 14, 8 / 16, 9 / 18,
     11 / 22 chunks of 128 rows: remainders 7 and 1 under the paired task numbering; 1400 is also the first size at which the split
     kernel's 256 slots push MC past 128); 1536 (the same for the fp32 kernel's 512 slots); 20 031; the fused training launch
     65 536 + 3 072 with a colour-less tail.  Flag combinations: with / without the deformation network x with / without colour, the
     colour-less tail with and without the deformation network.
  B  REAL operands.  A genuine forward + ES_BWD_CHAINS, the workspace copied to the host, then the weight-gradient stages; every entry
     against the fp64 contraction of the snapshot over the rows below M only (a non-zero pad row of an adjoint buffer is an error here):
         |out - exact| <= (T + 2) 2^-24 sum |dA| |X|,   T = rows accumulated into the entry over all problems that share it
     -- the a-priori bound of a length-T fp32 sum in any order.  The split kernel: the same bound, and its worst error relative to
     sum |dA| |X| per network within 1.5 x that of this test's own fp32 run + 2^-24 (the relation test_gpu_split_accuracy.py asserts).
     Two deterministic runs are bit-identical, and the three stages one by one equal es_point_backward_det bit for bit.

Measured on an MI355X (wgrad_problems_<case>.json in the log directory of test_gpu_split_accuracy.py):
  worst |error| / bound over the networks, fp32 deterministic | split:  M = 65: 0.104 | 0.101;  1 100: 2.8e-3 | 3.6e-3;  20 031: 1.5e-4 | 1.9e-4;
  65 536 + 3 072: 6.2e-5 | 5.5e-5 (fp32 atomics: 0.104, 3.3e-3, 1.8e-4, 4.5e-5).  In units of 2^-24 sum |dA| |X| the worst entry is 2.3 ... 8.3
  (fp32) and 1.8 ... 7.0 (split) at every size: the error does not grow with the row count, the bound does.  Part A: every case equal.
  Wall time of the module 33 s (part A 10 s, part B 23 s, of which the fp64 references of the two 68 608-row cases 17 s).
The reference of every comparison is wgrad_util.reference (fp64, host); nothing asks the library what it launched."""
import ctypes as C
import json
import os

import pytest
import torch

import wgrad_util as U
from gpu_util import renderer_for
from shapes_util import SEED, inputs as _inputs
from test_gpu_split_accuracy import LOG

pytestmark = pytest.mark.gpu
F_ALL = U.PF_DEFORM | U.PF_COLOR | U.PF_SAVE
RAN = set()          # kernel instantiations exercised by the exact cases
_ENG = {}


def _engine():
    if "eng" not in _ENG:
        from endosurf_amd.engine import Engine
        eng = Engine("cuda")
        eng.deterministic = True
        _ENG["eng"], _ENG["scratch"] = eng, eng.wg_scratch()
        eng.deterministic = False
    return _ENG["eng"], _ENG["scratch"]


def _library_layout(eng, M, flags):
    """wgrad_util's layout, every offset checked against es_point_workspace_offset."""
    lay = U.ws_layout(M, flags)
    assert int(eng.lib.es_point_workspace_floats(M, flags)) == lay.total
    for name, i in U.WS.items():
        assert int(eng.lib.es_point_workspace_offset(M, flags, i)) == lay.off[name], name
    assert int(eng.lib.es_point_workspace_offset(M, flags, U.WS_COUNT)) == -1
    woff, boff, total = U.weff_offsets()
    assert total == eng.n_weff
    for (net, l), o in woff.items():
        w, b = C.c_int64(), C.c_int64()
        assert eng.lib.es_weff_layout(net, l, C.byref(w), C.byref(b)) == 0 and (w.value, b.value) == (o, boff[net, l])
    return lay


class _Stages:
    """es_point_backward_stages on a given workspace: only the weight-gradient bits, so neither the points nor the weights are read."""

    def __init__(self, eng, scratch, M, ws, flags, m_color, d_sdf):
        from endosurf_amd import _lib
        self._lib, self.eng, self.scratch, self.ws, self.flags, self.m_color, self.d_sdf = _lib, eng, scratch, ws, flags, m_color, d_sdf
        z = lambda *s: torch.zeros(*s, device="cuda")
        self.pts = eng.points(x=z(M, 3), t=z(M), dirs=z(M, 3))
        self.packed, self.weff, self.d_go, self.d_rgb = z(eng.n_packed), z(eng.n_weff), z(M, 3), z(M, 3)

    def __call__(self, dweff, stages, det, x3):
        L = self._lib
        L.check(self.eng.lib.es_point_backward_stages(C.byref(self.pts), L.ptr(self.packed), L.ptr(self.weff), L.ptr(self.ws),
                                                      self.flags | (U.PF_X3 if x3 else 0), self.m_color, L.ptr(self.d_sdf), L.ptr(self.d_go),
                                                      L.ptr(self.d_rgb), L.ptr(dweff), L.ptr(self.scratch) if det else None, stages, self.eng.st()),
                "es_point_backward_stages")
        torch.cuda.synchronize()
        RAN.update(U.variants(self.flags, stages, det, x3))
        return dweff


def _first_bad(got, want):
    bad = (got != want).nonzero().flatten()
    return dict(count=int(bad.numel()), first=[(int(i), float(got[i]), float(want[i])) for i in bad[:6]])


def _exact_case(M, flags, m_color):
    eng, scratch = _engine()
    lay = _library_layout(eng, M, flags)
    gen = torch.Generator(device="cuda").manual_seed(1000 + M + flags)
    ws = torch.empty(lay.total, device="cuda")
    valid = U.fill_integer(ws, lay, M, flags, m_color, gen)
    d_sdf = torch.randint(-3, 4, (M,), generator=gen, device="cuda").float()
    snap, before = ws.cpu(), ws.clone()
    ref = U.reference(snap, lay, U.problems(flags), valid, d_sdf.cpu())
    del snap
    total = sum(ref.values())
    assert float(total.abs().max()) * 2 + 3 < 2 ** 24          # the premise: every partial sum (of two accumulated calls) is exact in fp32
    want = {s: v.float().cuda() for s, v in ref.items()}
    want_all = total.float().cuda()
    base = torch.randint(-3, 4, (eng.n_weff,), generator=gen, device="cuda").float()
    run = _Stages(eng, scratch, M, ws, flags, m_color, d_sdf)
    for x3 in (False, True):
        for det in (False, True):
            tag = (M, flags, m_color, "x3" if x3 else "fp32", "det" if det else "atomic")
            for stage in (U.STAGE_D, U.STAGE_S, U.STAGE_C):
                got = run(base.clone(), stage, det, x3)
                exp = base + want[stage] if stage in want else base          # (a stage whose network is absent launches nothing)
                assert torch.equal(got, exp), (tag, stage, _first_bad(got, exp))
            got = run(torch.zeros(eng.n_weff, device="cuda"), 14, det, x3)
            assert torch.equal(got, want_all), (tag, "all", _first_bad(got, want_all))
            got = run(got, 14, det, x3)
            assert torch.equal(got, 2 * want_all), (tag, "accumulate", _first_bad(got, 2 * want_all))
    assert torch.equal(ws, before), "the weight-gradient stages wrote to the workspace"


@pytest.mark.parametrize("M", [1, 128, 800, 1024, 1100, 1400, 1536])
def test_exact_row_counts(M):
    _exact_case(M, F_ALL, 0)


@pytest.mark.parametrize("name,M,flags,m_color", [
    ("no_deform", 1100, U.PF_COLOR | U.PF_SAVE, 0),
    ("no_deform_mc192", 2048, U.PF_COLOR | U.PF_SAVE, 0),          # first size at which the SDF launch's MC leaves 128 (fp32: 34 tasks per chunk)
    ("no_colour", 1100, U.PF_DEFORM | U.PF_SAVE, 0),                # the last deformation layer's tangent slice moves to the SDF launch
    ("sdf_only", 1100, U.PF_SAVE, 0),
    ("tail", 704, F_ALL, 640),
    ("tail_no_deform", 704, U.PF_COLOR | U.PF_SAVE, 640),
    ("colour_rows_not_128", 65, F_ALL, 0),                          # round_up64(M) = 128 = Mp; 129: Mc = 192 < Mp = 256
    ("colour_rows_below_mp", 129, F_ALL, 0),
])
def test_exact_flag_combinations(name, M, flags, m_color):
    _exact_case(M, flags, m_color)


def test_exact_20031():
    _exact_case(20031, F_ALL, 0)


def test_exact_training_launch_68608():
    """65 536 ray samples + 3 072 colour-less points: ~206 k rows into the deformation network's entries, every |entry| < 2^24."""
    _exact_case(65536 + 3072, F_ALL, 65536)


# ------------------------------------------------------------------------------------------------------------------------------
# B. real operands
# ------------------------------------------------------------------------------------------------------------------------------
_RENDERERS = {}
ULP = 2.0 ** -24


def _renderer(use_deform):
    if use_deform not in _RENDERERS:
        _RENDERERS[use_deform] = renderer_for(SEED, "trained", use_deform)
    r = _RENDERERS[use_deform]
    r.engine.deterministic, r.engine.split_precision = False, False
    return r


def _forward_and_chains(r, M, m_color, seed):
    """Engine.point_forward (fp32 family) + ES_BWD_CHAINS on shapes_util.inputs; returns (stage runner, context, full-backward closure)."""
    from endosurf_amd import _lib
    eng = r.engine
    weff, packed = r._weights()
    wd = weff.detach()
    flags = r._flags(weff) | _lib.PF_COLOR
    assert flags & _lib.PF_SAVE
    x, d, t, ws_, wg_, wc_ = _inputs(M, seed, r.use_deform, screen=[])
    dev = lambda a: a.cuda().contiguous()
    n_color = m_color if m_color else M
    pts = eng.points(x=dev(x), t=dev(t), dirs=dev(d))
    seeds = (dev(ws_), dev(wg_), dev(wc_[:n_color]))
    _, scratch = _engine()

    def call(ctx, dweff, stages, det, x3=False, whole=False):
        a = (C.byref(pts), _lib.ptr(packed), _lib.ptr(wd), _lib.ptr(ctx.ws), flags | (U.PF_X3 if x3 else 0), m_color, _lib.ptr(seeds[0]),
             _lib.ptr(seeds[1]), _lib.ptr(seeds[2]), _lib.ptr(dweff), _lib.ptr(scratch) if det else None)
        if whole == "plain":          # the entry without a scratch argument
            _lib.check(eng.lib.es_point_backward(*a[:-1], eng.st()), "es_point_backward")
        elif whole:
            _lib.check(eng.lib.es_point_backward_det(*a, eng.st()), "es_point_backward_det")
        else:
            _lib.check(eng.lib.es_point_backward_stages(*a, stages, eng.st()), "es_point_backward_stages")
        torch.cuda.synchronize()
        return dweff
    forward = lambda: eng.point_forward(pts, wd, packed, flags, m_color)
    return forward, call, flags, seeds


REAL = {"65": (65, 0), "1100": (1100, 0), "20031": (20031, 0), "train_68608": (65536 + 3072, 65536)}


@pytest.mark.parametrize("use_deform", [True, False])
@pytest.mark.parametrize("name", list(REAL))
def test_real_operands_against_fp64(name, use_deform):
    M, m_color = REAL[name]
    r = _renderer(use_deform)
    eng = r.engine
    forward, call, flags, seeds = _forward_and_chains(r, M, m_color, 7000 + M)
    zeros = lambda: torch.zeros(eng.n_weff, device="cuda")
    ctx = forward()
    call(ctx, zeros(), 1, False)          # ES_BWD_CHAINS alone
    lay = _library_layout(eng, M, flags)
    snap = ctx.ws.cpu()
    assert bool(torch.isfinite(snap[lay.off["WS_S_ACT"]:lay.off["WS_S_ACT"] + lay.size("WS_S_ACT")]).all())
    _, valid = U.row_counts(M, flags, m_color)
    ref, ab, cnt = U.reference(snap, lay, U.problems(flags), valid, seeds[0].cpu(), with_abs=True)
    exact = sum(ref.values())
    bound = (cnt + 2) * ULP * ab
    out = {"fp32_atomic": call(ctx, zeros(), 14, False), "fp32": call(ctx, zeros(), 14, True), "split": call(ctx, zeros(), 14, True, x3=True)}
    again = {"fp32": call(ctx, zeros(), 14, True), "split": call(ctx, zeros(), 14, True, x3=True)}
    one_by_one = zeros()
    for stage in (2, 4, 8):
        call(ctx, one_by_one, stage, True)
    whole = call(forward(), zeros(), 0, True, whole=True)          # a second forward + the whole deterministic backward in one call
    if M == 65:          # the two scratch-less whole backwards, each on a fresh forward of the same points: judged as fp32_atomic is
        out["plain"] = call(forward(), zeros(), 0, False, whole="plain")
        out["det_null_scratch"] = call(forward(), zeros(), 0, False, whole=True)
    report, fails = dict(case=name, use_deform=use_deform, M=M, m_color=m_color), []
    worst = {}
    for kind, got in out.items():
        err = (got.cpu().double() - exact).abs()
        assert bool(torch.isfinite(err).all()), kind
        for net, (b, e) in U.net_slices().items():
            live = ab[b:e] > 0
            if not bool(live.any()):
                assert not bool(got[b:e].any()), (kind, net)          # a network that is absent gets no gradient
                continue
            ratio = float((err[b:e][live] / bound[b:e][live]).max())
            rel = float((err[b:e][live] / ab[b:e][live]).max())
            worst[kind, net] = rel
            report[f"{kind}_net{net}"] = dict(worst_ratio_to_bound=ratio, worst_err_in_ulp_of_scale=rel / ULP)
            print(f"wgrad_problems {name} deform={use_deform} {kind} net{net}: |err|/bound {ratio:.3e}, |err|/(2^-24 sum|dA||X|) {rel / ULP:.3f}")
            if not ratio <= 1.0:
                fails.append((kind, net, ratio))
        dead = (ab == 0) & (got.cpu() != 0)
        assert not bool(dead.any()), (kind, "entries without any contribution are not zero", int(dead.sum()))
    os.makedirs(LOG, exist_ok=True)
    with open(os.path.join(LOG, f"wgrad_problems_{name}_{'deform' if use_deform else 'nodeform'}.json"), "w") as f:
        json.dump(report, f)
    assert not fails, fails
    for net in {n for _, n in worst}:
        assert worst["split", net] <= 1.5 * worst["fp32", net] + ULP, (net, worst["split", net], worst["fp32", net])
    assert torch.equal(out["fp32"], again["fp32"]) and torch.equal(out["split"], again["split"]), "deterministic runs differ"
    assert torch.equal(one_by_one, out["fp32"]), "three stages one by one differ from one call with all three"
    assert torch.equal(whole, out["fp32"]), _first_bad(whole, out["fp32"])


def test_zz_every_kernel_variant_ran():
    """All twelve k_wgrad / k_wgrad_x3 instantiations (network x deterministic) and k_wgrad_reduce were exercised by the exact cases."""
    if not RAN:          # run on its own: the smallest case of the full layout covers them all
        _exact_case(128, F_ALL, 0)
    assert RAN == U.ALL_VARIANTS, U.ALL_VARIANTS - RAN
