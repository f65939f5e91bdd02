"""The reference side of the weight-gradient tests (wgrad_util.py) checked on the host: its mirrors against the headers, its problem
table against the layer shapes, its fp64 contraction against autograd, and the premise of the exact GPU tests (integer operands keep
every fp32 partial sum exact, in any order)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import wgrad_util as U

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "endosurf_amd", "csrc")


def _text(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _layer_shapes():
    """(LAYER_K, LAYER_N, {(net, layer): (w_off, b_off)} or None): from es_weff_layout when the library loads here, else from arch.h."""
    LK, LN = U.parse_arch_table(_text("arch.h"), "LAYER_K"), U.parse_arch_table(_text("arch.h"), "LAYER_N")
    try:
        from endosurf_amd import _lib
        lib = _lib.load()
    except Exception:
        return LK, LN, None
    offs = {}
    for net in range(3):
        for l in range(9):
            w, b = C.c_int64(), C.c_int64()
            assert lib.es_weff_layout(net, l, C.byref(w), C.byref(b)) == 0
            offs[net, l] = (w.value, b.value)
    return LK, LN, offs


def test_buffer_ids_mirror_the_header():
    names = U.parse_wsbuf_enum(_text("workspace.h"))
    assert names[-1] == "WS_COUNT" and tuple(names[:-1]) == U.WSBUF_NAMES
    assert U.WS_COUNT == len(names) - 1 and set(U._SHAPES) == set(U.WSBUF_NAMES)
    assert (U.WS["WS_XCBAR"], U.WS["WS_CURV"], U.WS["WS_TBAR"], U.WS["WS_VBAR_C"]) == (27, 34, 35, 23)          # the header's static_assert


def test_layer_tables_mirror_the_header():
    LK, LN, offs = _layer_shapes()
    assert LK == U.LAYER_K and LN == U.LAYER_N
    woff, boff, total = U.weff_offsets()
    if offs is not None:
        assert all(offs[k] == (woff[k], boff[k]) for k in offs)
    assert total == sum(LN[n][l] * (LK[n][l] + 1) for n in range(3) for l in range(9))


def test_fragment_permutation():
    """A bijection of the tile that agrees with the formula in the comment above frag_off (written out here with its own loops)."""
    P = U.frag_index()
    assert P.shape == (64, 256) and sorted(P.reshape(-1).tolist()) == list(range(64 * 256))
    for w in range(4):
        for ri in range(2):
            for ni in range(2):
                for q in range(4):
                    for lane in (0, 1, 31, 32, 63):
                        hi, lo = lane >> 5, lane & 31
                        index = ((w * 16 + (ri * 2 + ni) * 4 + q) * 64 + lane) * 4
                        for e in range(4):          # the float4 = rows 32 ri + 8 q + 4 hi .. + 3 of column 64 w + 32 ni + lo
                            assert P[32 * ri + 8 * q + 4 * hi + e, 64 * w + 32 * ni + lo] == index + e
    t = torch.arange(128 * 256, dtype=torch.float32).reshape(128, 256)
    assert torch.equal(U.unpack_frag(U.pack_frag(t)), t)
    assert torch.equal(U.pack_frag(t).reshape(2, -1)[1, torch.from_numpy(P.reshape(-1))].reshape(64, 256), t[64:])


FLAG_CASES = {          # name: (flags, M, m_color)
    "deform_colour": (U.PF_DEFORM | U.PF_COLOR | U.PF_SAVE, 300, 0),
    "no_deform": (U.PF_COLOR | U.PF_SAVE, 300, 0),
    "no_colour": (U.PF_DEFORM | U.PF_SAVE, 300, 0),
    "colourless_tail": (U.PF_DEFORM | U.PF_COLOR | U.PF_SAVE, 300, 192),
}


@pytest.mark.parametrize("case", sorted(FLAG_CASES))
def test_problem_table_covers_every_entry_once_per_path(case):
    """Every weight and bias entry of every layer of the networks present is touched, nothing outside them is, and the blocks of one
    layer tile its [N][K] matrix: each entry gets exactly the value pass and (deformation, SDF) the second pass behind g_o / g_c."""
    flags, M, m_color = FLAG_CASES[case]
    LK, LN, offs = _layer_shapes()
    woff, boff, total = U.weff_offsets(LK, LN)
    if offs is not None:
        woff, boff = {k: v[0] for k, v in offs.items()}, {k: v[1] for k, v in offs.items()}
    hits = np.zeros(total, np.int64)
    lay = U.ws_layout(M, flags)
    launched, valid = U.row_counts(M, flags, m_color)
    for p in U.problems(flags, LK, LN):
        Kl, Nl = LK[p.net][p.layer], LN[p.net][p.layer]
        assert p.row0 + p.N <= Nl and p.col0 + p.K <= Kl, p
        hits[woff[p.net, p.layer]:woff[p.net, p.layer] + Nl * Kl].reshape(Nl, Kl)[p.row0:p.row0 + p.N, p.col0:p.col0 + p.K] += 1
        if p.bias:
            hits[boff[p.net, p.layer] + p.row0:boff[p.net, p.layer] + p.row0 + p.N] += 100
        for ref, width in ((p.x, p.K), (p.da, p.N)):          # the operands exist in this layout and are wide and long enough
            if isinstance(ref, tuple):
                layers, R, ld = lay.shape[ref[0]]
                assert ref[1] < layers and width <= ld and launched[p.rows] <= R, (p, lay.shape[ref[0]])
        assert valid[p.rows] <= launched[p.rows] and (p.small or launched[p.rows] % 64 == 0)
        assert not p.small or (p.K == 256 and p.N <= 4)
    present = {U.NET_S} | ({U.NET_D} if flags & U.PF_DEFORM else set()) | ({U.NET_C} if flags & U.PF_COLOR else set())
    for net, (b, e) in U.net_slices(LK, LN).items():
        if net not in present:
            assert not hits[b:e].any(), net
            continue
        for l in range(9):
            Kl, Nl = LK[net][l], LN[net][l]
            w = hits[woff[net, l]:woff[net, l] + Nl * Kl].reshape(Nl, Kl)
            bias = hits[boff[net, l]:boff[net, l] + Nl]
            if net == U.NET_S and l == 8:          # row 0: sdf (d_sdf + seed row of the reverse sweep); rows 1..256: the feature, with colour only
                assert (w[0] == 2).all() and bias[0] == 100
                assert (w[1:] == (1 if flags & U.PF_COLOR else 0)).all() and (bias[1:] == (100 if flags & U.PF_COLOR else 0)).all()
            else:
                assert (w == (1 if net == U.NET_C else 2)).all() and (bias == 100).all(), (net, l)


def test_workspace_layout_mirror_is_consistent():
    for flags in (7, 6, 5, 4, 3, 0):
        lay = U.ws_layout(1100, flags)
        assert lay.Mp == 1152 and lay.total % 64 == 0
        ends = [lay.off[n] + lay.size(n) for n in U.WSBUF_NAMES]
        assert all(e <= o for e, o in zip(ends, [lay.off[n] for n in U.WSBUF_NAMES[1:]] + [lay.total]))
    assert U.ws_layout(100, 7).off["WS_SDF"] == 128 * 6          # as tests/test_abi.py asks of the library


def test_chunk_rule_of_the_chosen_row_counts():
    """The row counts of the GPU module hit the launch geometries they are there for (MC rule of launch_group's comment)."""
    F = U.PF_DEFORM | U.PF_COLOR | U.PF_SAVE
    P = U.problems(F)

    def geo(M, stage, x3, m_color=0):
        return U.launch_geometry(P, stage, U.row_counts(M, F, m_color)[0], x3)
    for M in (1, 128):
        assert {c for _, c in geo(M, U.STAGE_D, False)[1]} == {1, 2} and geo(M, U.STAGE_S, False)[1][0][1] == 1
    for M, c in ((1024, 8), (1100, 9), (1400, 11), (800, 7)):          # 8 / 16, 9 / 18, 11 / 22; remainders 1 and 7 under the paired numbering
        MC, g = geo(M, U.STAGE_D, False)
        assert MC == 128 and {n for _, n in g} == {c, 2 * c} and any(k == 2 for k, _ in g)
    assert 1100 // 128 + 1 == 9 and 9 % 8 == 1 and 7 % 8 == 7
    # the first sizes at which MC leaves 128: fp32 kernel (512 slots) Mp = 1536 in the deformation launch; split kernel (256 slots) Mp = 1408
    assert geo(1408, U.STAGE_D, False)[0] == 128 and geo(1409, U.STAGE_D, False)[0] == 192
    assert geo(1280, U.STAGE_D, True)[0] == 128 and geo(1281, U.STAGE_D, True)[0] == 192 and geo(1400, U.STAGE_D, True)[0] == 192
    for x3, slots in ((False, 512), (True, 256)):
        for stage in (U.STAGE_D, U.STAGE_S, U.STAGE_C):
            for M, mc in ((1536, 0), (20031, 0), (68608, 65536)):
                MC, g = geo(M, stage, x3, mc)
                assert MC % 64 == 0 and sum(k * c for k, c in g) <= slots
                assert MC == 128 or sum(k * -(-U.row_counts(M, F, mc)[0][p.rows] // (MC - 64)) for (k, _), p in
                                        zip(g, [p for p in P if p.stage == stage and not p.small])) > slots


def _toy():
    """A two-layer net y = W1 softplus(W0 x + b0) + b1 (39 -> 256 -> 3) on 100 points in a 128-row toy workspace: the input row-major in
    a 64-wide buffer, the hidden activation and its adjoint in fragment order, the output adjoint in a [..][4] buffer."""
    g = torch.Generator().manual_seed(3)
    M, Mp = 100, 128
    LK, LN = ((39, 256),), ((256, 3),)
    W0 = torch.randn(256, 39, generator=g, dtype=torch.float64, requires_grad=True)
    b0 = torch.randn(256, generator=g, dtype=torch.float64, requires_grad=True)
    W1 = torch.randn(3, 256, generator=g, dtype=torch.float64, requires_grad=True)
    b1 = torch.randn(3, generator=g, dtype=torch.float64, requires_grad=True)
    x = torch.randn(M, 39, generator=g).double()
    seed = torch.randn(M, 3, generator=g).double()
    z = x @ W0.t() + b0
    h = torch.nn.functional.softplus(z)
    z.retain_grad()
    ((h @ W1.t() + b1) * seed).sum().backward()
    lay = U.Layout({"X0": 0, "H": Mp * 64, "A0": Mp * 64 + Mp * 256, "A1": Mp * 64 + 2 * Mp * 256},
                   {"X0": (1, Mp, 64), "H": (1, Mp, 256), "A0": (1, Mp, 256), "A1": (1, Mp, 4)}, Mp * (64 + 512 + 4), Mp)
    snap = torch.full((lay.total,), 7.0)          # junk wherever nothing is written: pad rows, columns 39.., the fourth lane
    lay.view(snap, "X0")[:M, :39] = x.float()
    for name, val in (("H", h.detach()), ("A0", z.grad)):
        full = torch.full((Mp, 256), 7.0)
        full[:M] = val.float()
        lay.view(snap, name).copy_(U.pack_frag(full))
    lay.view(snap, "A1")[:M, :3] = seed.float()
    probs = [U.Prob(U.STAGE_S, False, ("X0", 0, False), ("A0", 0, True), "Mp", 39, 256, 0, 0, 0, 0, True, 1),
             U.Prob(U.STAGE_S, True, ("H", 0, True), ("A1", 0, False), "Mp", 256, 3, 0, 1, 0, 0, True, 1)]
    return lay, snap, probs, {"Mp": M}, LK, LN, (W0, b0, W1, b1)


def test_reference_against_autograd_of_a_two_layer_toy():
    lay, snap, probs, valid, LK, LN, (W0, b0, W1, b1) = _toy()
    out, ab, cnt = U.reference(snap, lay, probs, valid, LK=LK, LN=LN, with_abs=True)
    got = out[U.STAGE_S]
    want = torch.cat([W0.grad.reshape(-1), b0.grad, W1.grad.reshape(-1), b1.grad])
    # the snapshot holds the operands rounded to fp32: 100-term sums of O(1) products
    assert float((got - want).abs().max()) < 1e-4 * float(want.abs().max())
    assert float(cnt.min()) == 100 and float(cnt.max()) == 100 and bool((ab >= got.abs() - 1e-12).all())
    x32, a32 = lay.view(snap, "X0")[:100, :39].double(), U.unpack_frag(lay.view(snap, "A0"))[:100].double()
    assert torch.equal(got[:256 * 39].view(256, 39), a32.t() @ x32)          # and exactly the contraction of what the snapshot holds


def test_reference_bias_stride_and_shared_outputs():
    """bias_stride = 2 takes rows 0, 2, 4 ...; two problems into one block add up; ``ones`` and ``d_sdf`` operands."""
    lay = U.Layout({"X": 0, "A": 64 * 256}, {"X": (1, 64, 256), "A": (1, 64, 256)}, 2 * 64 * 256, 64)
    g = torch.Generator().manual_seed(5)
    snap = torch.randint(-3, 4, (lay.total,), generator=g).float()
    d_sdf = torch.randint(-3, 4, (10,), generator=g).float()
    LK, LN = ((256,),), ((256,),)
    X, A = lay.view(snap, "X").double(), lay.view(snap, "A").double()
    P = [U.Prob(2, False, ("X", 0, False), ("A", 0, False), "r", 256, 256, 0, 0, 0, 0, True, 2),
         U.Prob(2, True, ("X", 0, False), "ones", "r", 256, 1, 0, 0, 0, 0, False, 1),
         U.Prob(2, True, ("X", 0, False), "d_sdf", "s", 256, 1, 0, 0, 0, 0, True, 1)]
    out = U.reference(snap, lay, P, {"r": 50, "s": 10}, d_sdf, LK=LK, LN=LN)[2]
    W = (A[:50].t() @ X[:50])
    W[0] += X[:50].sum(0) + d_sdf.double() @ X[:10]
    b = A[0:50:2].sum(0)
    b[0] += d_sdf.double().sum()
    assert torch.equal(out[:65536].view(256, 256), W) and torch.equal(out[65536:], b)


@pytest.mark.parametrize("M,m_color", [(1100, 0), (704, 640)])
def test_integer_fill_keeps_the_contract_and_fp32_sums_exact(M, m_color):
    """The fill obeys the padding contract (zeros / non-zero junk where wgrad_util says), the reference over the real rows equals the
    reference over every row the kernels run over (so one member of every pair is zero on the pad rows), and a float32 accumulation
    in a shuffled row order reproduces it exactly.  (The same check at 68 608 rows was run once by hand: see the GPU module.)"""
    flags = U.PF_DEFORM | U.PF_COLOR | U.PF_SAVE
    lay = U.ws_layout(M, flags)
    gen = torch.Generator().manual_seed(M)
    ws = torch.empty(lay.total)
    valid = U.fill_integer(ws, lay, M, flags, m_color, gen)
    launched, _ = U.row_counts(M, flags, m_color)
    assert bool((ws == ws.round()).all()) and float(ws.abs().max()) == 3.0
    da = lay.view(ws, "WS_D_A", 3)
    assert not da[2 * M:].any() and bool((da[:2 * M, 204:] != 0).all()) and bool((da[1:2 * M:2, :204] != 0).any())
    assert bool((lay.view(ws, "WS_D_R", 0)[M:] != 0).all()) and not lay.view(ws, "WS_D_T", 7)[M:].any()
    assert bool((lay.view(ws, "WS_GC")[M:] != 0).all()) and bool((lay.view(ws, "WS_C_IN")[:, 93:] != 0).all())
    assert not U.unpack_frag(lay.view(ws, "WS_S_TAU", 7))[M:].any() and bool((U.unpack_frag(lay.view(ws, "WS_S_RHO", 2))[M:] != 0).all())
    assert bool((lay.view(ws, "WS_C_Y8")[:M, 3] != 0).all()) and not lay.view(ws, "WS_C_Y", 1)[M:].any()
    if m_color:
        assert bool((lay.view(ws, "WS_C_Y", 1)[m_color:M] != 0).all()) and bool((lay.view(ws, "WS_C_H", 1)[m_color:M] != 0).all())
    d_sdf = torch.randint(-3, 4, (M,), generator=gen).float()
    probs = U.problems(flags)
    ref = U.reference(ws, lay, probs, valid, d_sdf)
    full = U.reference(ws, lay, probs, dict(launched), d_sdf)
    tot = sum(ref.values())
    assert all(torch.equal(ref[s], full[s]) for s in ref) and float(tot.abs().max()) < 2 ** 24
    assert float(tot.abs().max()) > 100          # (not vacuous)
    assert torch.equal(shuffled_fp32(ws, lay, probs, valid, d_sdf, seed=1), tot.float())


def shuffled_fp32(ws, lay, probs, valid, d_sdf, seed):
    """The contractions accumulated in float32 by numpy, rows in a random order, 4096 rows at a time."""
    woff, boff, total = U.weff_offsets()
    out = np.zeros(total, np.float32)
    rng = np.random.default_rng(seed)
    for p in probs:
        rows = valid[p.rows]
        X = U._operand(ws, lay, p.x, rows, p.K, d_sdf).float().numpy()
        A = U._operand(ws, lay, p.da, rows, p.N, d_sdf).float().numpy()
        Kl, Nl = U.LAYER_K[p.net][p.layer], U.LAYER_N[p.net][p.layer]
        W = out[woff[p.net, p.layer]:woff[p.net, p.layer] + Nl * Kl].reshape(Nl, Kl)[p.row0:p.row0 + p.N, p.col0:p.col0 + p.K]
        order = rng.permutation(rows)
        for i in range(0, rows, 4096):
            sel = order[i:i + 4096]
            W += A[sel].T @ X[sel]
            if p.bias:
                out[boff[p.net, p.layer] + p.row0:boff[p.net, p.layer] + p.row0 + p.N] += A[sel[sel % p.bias_stride == 0]].sum(0, dtype=np.float32)
    return torch.from_numpy(out)
