"""Reference side of the weight-gradient tests (test_wgrad_host.py, test_gpu_wgrad_problems.py): numpy / torch-CPU fp64 only.

The backward pass ends in  dW[n][k] += sum_m dA[m][n] X[m][k]  for every layer, from (layer input X, pre-activation adjoint dA) pairs
that the chains leave in the point workspace (csrc/workspace.h).  This module restates, from the maths of the backward and NOT from
what csrc/wgrad.hip launches:

  * the buffer ids and shapes of the workspace (mirror of WsBuf / ws_layout),
  * the accumulator-fragment order of the SDF kernels' [64 x 256] tiles (chain_common.h frag_off),
  * the table of contractions (which pair feeds which rows / columns of which layer, and which of them feed a bias),
  * the fp64 result of that table on a host snapshot of a workspace, in es_weff_layout order,
  * an integer fill of a workspace on which the fp32 result must equal the fp64 one bit for bit.

Which member of a pair is zero on the rows past M (the kernels have no row guards, so one of them has to be):
  (u_l, abar_l) D_U0/D_U x D_A, (u_8, abar_8) D_U x D_A8 ......... dA: an adjoint buffer
  (tau_l, r_l)  D_T0/D_T x D_R, (tau_8, g_c) D_T x GC ............ X: the backward's tangent sweep is seeded with d_go = 0 on those rows;
                                                                   D_R and GC are FORWARD buffers (junk)
  (s_l, zbar_l) S_S0/S_ACT x S_ZB, (s_8, featbar) S_ACT x FEATBAR  dA: adjoint buffers
  (tau_l, rho_l) S_TAU0/S_TAU x S_RHO, column sums of tau_8 ...... X: tangent of the zero seed; S_RHO is a FORWARD buffer (junk)
  (s_8, d_sdf) ................................................... neither: the problem has the M real rows only
  colour pairs C_IN/FEAT/C_H x C_Y, C_H x C_Y8 ................... dA: adjoint buffers
csrc/workspace.h promises exactly this (its tangent-buffer sentence was added with these tests)."""
import re
from collections import namedtuple

import numpy as np
import torch

PF_DEFORM, PF_COLOR, PF_SAVE, PF_X3 = 1, 2, 4, 8
STAGE_D, STAGE_S, STAGE_C = 2, 4, 8          # ES_BWD_WGRAD_DEFORM / _SDF / _COLOR
NET_D, NET_S, NET_C = 0, 1, 2
LAYERS = 9
LAYER_K = ((52, 256, 256, 256, 256, 256, 256, 256, 256), (39, 256, 256, 256, 295, 256, 256, 256, 256), (349, 256, 256, 256, 605, 256, 256, 256, 256))
LAYER_N = ((256, 256, 256, 204, 256, 256, 256, 256, 3), (256, 256, 256, 256, 256, 256, 256, 256, 257), (256, 256, 256, 256, 256, 256, 256, 256, 3))

WSBUF_NAMES = ("WS_XC", "WS_V", "WS_SDF", "WS_FEAT", "WS_GC", "WS_GO", "WS_RGB", "WS_S_ACT", "WS_D_U0", "WS_D_U", "WS_D_MASK", "WS_D_R",
               "WS_S_S0", "WS_S_RHO", "WS_S_ADJEPS", "WS_C_IN", "WS_C_H", "WS_C_MASK", "WS_C_Y", "WS_C_Y8", "WS_FEATBAR", "WS_XCBAR_C",
               "WS_GCBAR_C", "WS_VBAR_C", "WS_S_TAU0", "WS_S_TAU", "WS_S_ZB", "WS_XCBAR", "WS_JU", "WS_D_T0", "WS_D_T", "WS_D_A", "WS_D_A8",
               "WS_C_SBAR", "WS_CURV", "WS_TBAR")
WS = {n: i for i, n in enumerate(WSBUF_NAMES)}
WS_COUNT = len(WSBUF_NAMES)


def parse_wsbuf_enum(text):
    """Enumerator names of ``enum WsBuf`` in the text of csrc/workspace.h, in order (WS_COUNT included)."""
    body = re.search(r"enum\s+WsBuf\s*:\s*int\s*\{(.*?)\};", text, re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    return [t.strip() for t in body.split(",") if t.strip()]


def parse_arch_table(text, name):
    """LAYER_K / LAYER_N of csrc/arch.h as a tuple of tuples."""
    body = re.search(name + r"\[NETS\]\[LAYERS\]\s*=\s*\{(.*?)\};", text, re.S).group(1)
    return tuple(tuple(int(v) for v in row.split(",")) for row in re.findall(r"\{([^{}]*)\}", body))


# ---- effective-weight layout (arch.h: for net, for layer: W[N][K] row-major, b[N]) ------------------------------------------------
def weff_offsets(LK=LAYER_K, LN=LAYER_N):
    """({(net, layer): w_off}, {(net, layer): b_off}, total)"""
    w, b, off = {}, {}, 0
    for net in range(len(LK)):
        for l in range(len(LK[net])):
            w[net, l] = off
            b[net, l] = off + LN[net][l] * LK[net][l]
            off += LN[net][l] * (LK[net][l] + 1)
    return w, b, off


# ---- workspace layout ------------------------------------------------------------------------------------------------------------
# name: (condition, layers, rows = Mp * num // den, leading dimension)
_SHAPES = {
    "WS_XC": ("", 1, 1, 1, 3), "WS_V": ("", 1, 1, 1, 3), "WS_SDF": ("", 1, 1, 1, 1), "WS_GC": ("", 1, 1, 1, 3), "WS_GO": ("", 1, 1, 1, 3),
    "WS_D_MASK": ("d", 8, 1, 32, 256), "WS_CURV": ("d", 1, 1, 1, 3), "WS_TBAR": ("d", 1, 1, 1, 1),
    "WS_FEAT": ("c", 1, 1, 1, 256), "WS_RGB": ("c", 1, 1, 1, 3), "WS_C_IN": ("c", 1, 1, 1, 128), "WS_S_ACT": ("", 8, 1, 1, 256),
    "WS_D_U0": ("sd", 1, 2, 1, 64), "WS_D_U": ("sd", 8, 2, 1, 256), "WS_D_A": ("sd", 8, 2, 1, 256), "WS_D_A8": ("sd", 1, 2, 1, 4),
    "WS_D_R": ("sd", 8, 1, 1, 256), "WS_JU": ("sd", 1, 1, 1, 3), "WS_D_T0": ("sd", 1, 1, 1, 64), "WS_D_T": ("sd", 8, 1, 1, 256),
    "WS_S_S0": ("s", 1, 1, 1, 64), "WS_S_RHO": ("s", 8, 1, 1, 256), "WS_S_ADJEPS": ("s", 1, 1, 1, 64), "WS_S_TAU0": ("s", 1, 1, 1, 64),
    "WS_S_TAU": ("s", 8, 1, 1, 256), "WS_S_ZB": ("s", 8, 1, 1, 256), "WS_XCBAR": ("s", 1, 1, 1, 3),
    "WS_C_SBAR": ("sc", 1, 1, 1, 128), "WS_C_H": ("sc", 8, 1, 1, 256), "WS_C_MASK": ("sc", 8, 1, 64, 512), "WS_C_Y": ("sc", 8, 1, 1, 256),
    "WS_C_Y8": ("sc", 1, 1, 1, 4), "WS_FEATBAR": ("sc", 1, 1, 1, 256), "WS_XCBAR_C": ("sc", 1, 1, 1, 3), "WS_GCBAR_C": ("sc", 1, 1, 1, 3),
    "WS_VBAR_C": ("sc", 1, 1, 1, 3),
}
FRAG_BUFFERS = ("WS_S_ACT", "WS_S_RHO", "WS_S_TAU", "WS_S_ZB")


class Layout:
    """Offsets and logical shapes (layers, rows, ld) of named buffers inside one flat fp32 workspace."""

    def __init__(self, off, shape, total, Mp):
        self.off, self.shape, self.total, self.Mp = off, shape, total, Mp

    def size(self, name):
        l, r, ld = self.shape[name]
        return l * r * ld

    def view(self, ws, name, layer=0):
        """Layer ``layer`` of buffer ``name`` as stored: [rows, ld] (fragment-ordered buffers: see unpack_frag)."""
        l, r, ld = self.shape[name]
        o = self.off[name] + layer * r * ld
        return ws[o:o + r * ld].view(r, ld)


def round_up(m, q):
    return (m + q - 1) // q * q


def ws_layout(M, flags):
    """Mirror of csrc/workspace.h ws_layout: every buffer padded to a multiple of 64 floats, rows padded to a multiple of 128."""
    Mp = round_up(M, 128)
    have = {"": True, "d": bool(flags & PF_DEFORM), "c": bool(flags & PF_COLOR), "s": bool(flags & PF_SAVE)}
    off, shape, o = {}, {}, 0
    for name in WSBUF_NAMES:
        cond, layers, num, den, ld = _SHAPES[name]
        on = all(have[c] for c in cond)
        shape[name] = (layers, Mp * num // den, ld) if on else (0, 0, ld)
        off[name] = o
        o += round_up(shape[name][0] * shape[name][1] * ld, 64)
    return Layout(off, shape, o, Mp)


# ---- fragment order ---------------------------------------------------------------------------------------------------------------
def frag_index():
    """P[row, col] = position of element (row, col) of a [64 x 256] tile in accumulator-fragment order: the float4 of a quad (rows
    32 ri + 8 q + 4 hi .. + 3 of column 64 w + 32 ni + lo) sits at ((w * 16 + (ri * 2 + ni) * 4 + q) * 64 + hi * 32 + lo) * 4."""
    row, col = np.meshgrid(np.arange(64), np.arange(256), indexing="ij")
    ri, q, hi, e = row >> 5, (row >> 3) & 3, (row >> 2) & 1, row & 3
    w, ni, lo = col >> 6, (col >> 5) & 1, col & 31
    return (((w * 16 + (ri * 2 + ni) * 4 + q) * 64 + hi * 32 + lo) * 4 + e).astype(np.int64)


_FRAG = {}


def _frag(device):
    key = str(device)
    if key not in _FRAG:
        _FRAG[key] = torch.from_numpy(frag_index().reshape(-1)).to(device)
    return _FRAG[key]


def pack_frag(rows):
    """Row-major [R, 256] (R a multiple of 64) -> the same storage with every 64-row tile in fragment order."""
    R = rows.shape[0]
    tiles = rows.reshape(R // 64, 64 * 256)
    out = torch.empty_like(tiles)
    out[:, _frag(rows.device)] = tiles
    return out.reshape(R, 256)


def unpack_frag(stored):
    R = stored.shape[0]
    return stored.reshape(R // 64, 64 * 256)[:, _frag(stored.device)].reshape(R, 256)


# ---- the contractions -------------------------------------------------------------------------------------------------------------
# x / da: (buffer, layer inside the stack, fragment-ordered); da may also be "ones" (dA = 1: column sums of X) or "d_sdf" (the caller's
# [M] vector).  rows: "2Mp" (value + J d rows of every point), "Mp" (one row per point), "Mc" (rows that went through the colour
# network), "M" (real rows only).  The block lands at rows row0 .. row0 + N, columns col0 .. col0 + K of W[net][layer]; bias: the column
# sums of dA over the rows r with r % bias_stride == 0 go to b[net][layer][row0 ..].  small: one of the <= 4-output problems that the
# library slices over the GEMM tasks of the launch ``stage``.
Prob = namedtuple("Prob", "stage small x da rows K N net layer row0 col0 bias bias_stride")


def problems(flags, LK=LAYER_K, LN=LAYER_N):
    """Every contraction of the weight gradient of one point evaluation, from the structure of the backward pass:
    deformation network: the reverse sweep of (value row, J d row) pairs inputs u_l with adjoints abar_l (bias: value rows only -- the
      tangent J d does not see the bias), and g_o = J^T g_c is linear in every W_l: the VJP sweep's r_l pairs with the tangent tau_l;
    SDF network: value pass (s_l, zbar_l) and the reverse sweep behind g_c (tau_l, rho_l); the skip layer's input is [s_4 | enc];
      the last layer's row 0 is the SDF (adjoint d_sdf, plus the seed row of the reverse sweep: column sums of tau_8), rows 1..256 the
      colour network's geometry feature;
    colour network: inputs [small (93) | feature (256)] at layers 0 and 4 (behind the 256 hidden columns there), adjoints y_l."""
    deform, color = bool(flags & PF_DEFORM), bool(flags & PF_COLOR)
    P = []
    if deform:
        for l in range(8):
            u = ("WS_D_U0", 0, False) if l == 0 else ("WS_D_U", l - 1, False)
            tau = ("WS_D_T0", 0, False) if l == 0 else ("WS_D_T", l - 1, False)
            K, N = LK[NET_D][l], LN[NET_D][l]
            P.append(Prob(STAGE_D, False, u, ("WS_D_A", l, False), "2Mp", K, N, NET_D, l, 0, 0, True, 2))
            P.append(Prob(STAGE_D, False, tau, ("WS_D_R", l, False), "Mp", K, N, NET_D, l, 0, 0, False, 1))
        # the last layer (3 outputs) rides with the shorter launches: the value / J d pair with the SDF launch, the tangent pair with
        # the colour launch (the SDF launch when there is none)
        P.append(Prob(STAGE_S, True, ("WS_D_U", 7, False), ("WS_D_A8", 0, False), "2Mp", 256, 3, NET_D, 8, 0, 0, True, 2))
        P.append(Prob(STAGE_C if color else STAGE_S, True, ("WS_D_T", 7, False), ("WS_GC", 0, False), "Mp", 256, 3, NET_D, 8, 0, 0, False, 1))
    for l in range(8):
        s = ("WS_S_S0", 0, False) if l == 0 else ("WS_S_ACT", l - 1, True)
        tau = ("WS_S_TAU0", 0, False) if l == 0 else ("WS_S_TAU", l - 1, True)
        K = 39 if l == 0 else 256
        P.append(Prob(STAGE_S, False, s, ("WS_S_ZB", l, True), "Mp", K, 256, NET_S, l, 0, 0, True, 1))
        P.append(Prob(STAGE_S, False, tau, ("WS_S_RHO", l, True), "Mp", K, 256, NET_S, l, 0, 0, False, 1))
        if l == 4:
            P.append(Prob(STAGE_S, False, ("WS_S_S0", 0, False), ("WS_S_ZB", 4, True), "Mp", 39, 256, NET_S, 4, 0, 256, False, 1))
            P.append(Prob(STAGE_S, False, ("WS_S_TAU0", 0, False), ("WS_S_RHO", 4, True), "Mp", 39, 256, NET_S, 4, 0, 256, False, 1))
    if color:
        P.append(Prob(STAGE_S, False, ("WS_S_ACT", 7, True), ("WS_FEATBAR", 0, False), "Mc", 256, 256, NET_S, 8, 1, 0, True, 1))
    P.append(Prob(STAGE_S, True, ("WS_S_ACT", 7, True), "d_sdf", "M", 256, 1, NET_S, 8, 0, 0, True, 1))
    P.append(Prob(STAGE_S, True, ("WS_S_TAU", 7, True), "ones", "Mp", 256, 1, NET_S, 8, 0, 0, False, 1))
    if color:
        for l in range(8):
            if l == 0:
                P.append(Prob(STAGE_C, False, ("WS_C_IN", 0, False), ("WS_C_Y", 0, False), "Mc", 93, 256, NET_C, 0, 0, 0, True, 1))
                P.append(Prob(STAGE_C, False, ("WS_FEAT", 0, False), ("WS_C_Y", 0, False), "Mc", 256, 256, NET_C, 0, 0, 93, False, 1))
                continue
            P.append(Prob(STAGE_C, False, ("WS_C_H", l - 1, False), ("WS_C_Y", l, False), "Mc", 256, 256, NET_C, l, 0, 0, True, 1))
            if l == 4:
                P.append(Prob(STAGE_C, False, ("WS_C_IN", 0, False), ("WS_C_Y", 4, False), "Mc", 93, 256, NET_C, 4, 0, 256, False, 1))
                P.append(Prob(STAGE_C, False, ("WS_FEAT", 0, False), ("WS_C_Y", 4, False), "Mc", 256, 256, NET_C, 4, 0, 349, False, 1))
        P.append(Prob(STAGE_C, True, ("WS_C_H", 7, False), ("WS_C_Y8", 0, False), "Mc", 256, 3, NET_C, 8, 0, 0, True, 1))
    return P


def row_counts(M, flags, m_color=0):
    """(rows a problem runs over, rows of it that belong to real points), per row kind."""
    Mp = round_up(M, 128)
    n_color = (m_color if 0 < m_color < M else M) if flags & PF_COLOR else 0
    Mc = round_up(n_color, 64)
    return {"2Mp": 2 * Mp, "Mp": Mp, "Mc": Mc, "M": M}, {"2Mp": 2 * M, "Mp": M, "Mc": n_color, "M": M}


def launch_geometry(probs, stage, launched, x3):
    """The row-chunk rule of launch_group for the GEMM problems of ``stage``: a task is (problem, block of 128 input features -- all 256
    in split precision, row chunk of MC rows); MC is the smallest 128 + 64 j for which the group fits one round of 512 (split: 256)
    workgroup slots.  Returns (MC, [(k blocks, row chunks) per problem])."""
    kw, slots = (256, 256) if x3 else (128, 512)
    g = [p for p in probs if p.stage == stage and not p.small]
    MC = 128
    count = lambda mc: sum(-(-p.K // kw) * -(-launched[p.rows] // mc) for p in g)
    while MC < 65536 and count(MC) > slots:
        MC += 64
    return MC, [(-(-p.K // kw), -(-launched[p.rows] // MC)) for p in g]


def variants(flags, stages, det, x3):
    """Kernel instantiations that a call with these stage bits runs: (kernel, network of the launch, deterministic)."""
    v = set()
    for bit, net, need in ((STAGE_D, 0, PF_DEFORM), (STAGE_S, 1, 0), (STAGE_C, 2, PF_COLOR)):
        if stages & bit and (flags & need) == need:
            v.add(("k_wgrad_x3" if x3 else "k_wgrad", net, bool(det)))
            if det:
                v.add(("k_wgrad_reduce",))
    return v


ALL_VARIANTS = {(k, n, d) for k in ("k_wgrad", "k_wgrad_x3") for n in range(3) for d in (False, True)} | {("k_wgrad_reduce",)}


# ---- reference --------------------------------------------------------------------------------------------------------------------
def _operand(snap, lay, ref, rows, cols, d_sdf):
    if ref == "ones":
        return torch.ones(rows, 1, dtype=torch.float64)
    if ref == "d_sdf":
        return d_sdf.reshape(-1, 1)[:rows].double()
    name, layer, frag = ref
    v = lay.view(snap, name, layer)
    if frag:
        v = unpack_frag(v[:round_up(rows, 64)])
    return v[:rows, :cols].double()


def reference(snap, lay, probs, valid, d_sdf=None, LK=LAYER_K, LN=LAYER_N, with_abs=False):
    """fp64 gradient of the effective weights, per launch stage: {stage: dweff}, from the host snapshot ``snap`` of a workspace, over the
    rows of real points only (``valid``: row kind -> count).  With ``with_abs`` also sum |dA| |X| and the number of rows accumulated
    into every entry (over all problems that share it), both over all stages."""
    woff, boff, total = weff_offsets(LK, LN)
    out = {}
    ab = torch.zeros(total, dtype=torch.float64) if with_abs else None
    cnt = torch.zeros(total, dtype=torch.float64) if with_abs else None
    for p in probs:
        rows = valid[p.rows]
        if rows == 0:
            continue
        o = out.setdefault(p.stage, torch.zeros(total, dtype=torch.float64))
        X = _operand(snap, lay, p.x, rows, p.K, d_sdf)
        A = _operand(snap, lay, p.da, rows, p.N, d_sdf)
        Kl, Nl = LK[p.net][p.layer], LN[p.net][p.layer]
        blk = lambda t: t[woff[p.net, p.layer]:woff[p.net, p.layer] + Nl * Kl].view(Nl, Kl)[p.row0:p.row0 + p.N, p.col0:p.col0 + p.K]
        bia = lambda t: t[boff[p.net, p.layer] + p.row0:boff[p.net, p.layer] + p.row0 + p.N]
        blk(o).add_(A.t() @ X)
        if p.bias:
            bia(o).add_(A[::p.bias_stride].sum(0))
        if with_abs:
            blk(ab).add_(A.abs().t() @ X.abs())
            blk(cnt).add_(rows)
            if p.bias:
                bia(ab).add_(A[::p.bias_stride].abs().sum(0))
                bia(cnt).add_(-(-rows // p.bias_stride))
    return (out, ab, cnt) if with_abs else out


def net_slices(LK=LAYER_K, LN=LAYER_N):
    """{net: (begin, end)} of the networks' parts of the effective-weight buffer."""
    woff, _, total = weff_offsets(LK, LN)
    begins = [woff[n, 0] for n in range(len(LK))] + [total]
    return {n: (begins[n], begins[n + 1]) for n in range(len(LK))}


# ---- integer fill -----------------------------------------------------------------------------------------------------------------
# operand buffer: (kind, row kind of its valid rows, valid columns per layer).  kind "adj": rows of no real point are exact zeros (the
# promise of workspace.h for adjoint and tangent buffers); "fwd": they are junk.
_N_D = lambda l: LAYER_N[NET_D][l]
OPERANDS = {
    "WS_D_U0": ("fwd", "2Mp", lambda l: 52), "WS_D_U": ("fwd", "2Mp", lambda l: 256), "WS_D_A": ("adj", "2Mp", _N_D), "WS_D_A8": ("adj", "2Mp", lambda l: 3),
    "WS_D_R": ("fwd", "Mp", _N_D), "WS_D_T0": ("adj", "Mp", lambda l: 52), "WS_D_T": ("adj", "Mp", lambda l: 256), "WS_GC": ("fwd", "Mp", lambda l: 3),
    "WS_S_S0": ("fwd", "Mp", lambda l: 39), "WS_S_ACT": ("fwd", "Mp", lambda l: 256), "WS_S_ZB": ("adj", "Mp", lambda l: 256),
    "WS_S_RHO": ("fwd", "Mp", lambda l: 256), "WS_S_TAU0": ("adj", "Mp", lambda l: 39), "WS_S_TAU": ("adj", "Mp", lambda l: 256),
    "WS_FEATBAR": ("adj", "Mc", lambda l: 256), "WS_FEAT": ("fwd", "Mc", lambda l: 256), "WS_C_IN": ("fwd", "Mc", lambda l: 93),
    "WS_C_H": ("fwd", "Mc", lambda l: 256), "WS_C_Y": ("adj", "Mc", lambda l: 256), "WS_C_Y8": ("adj", "Mc", lambda l: 3),
}


def _junk(shape, gen, device):
    """Non-zero integers in {-3 .. 3}: wherever nothing is promised."""
    mag = torch.randint(1, 4, shape, generator=gen, device=device, dtype=torch.int8)
    sgn = torch.randint(0, 2, shape, generator=gen, device=device, dtype=torch.int8) * 2 - 1
    return (mag * sgn).float()


def fill_integer(ws, lay, M, flags, m_color, gen):
    """Fills the workspace ``ws`` (any device) for the exact tests: uniform integers in {-3 .. 3} on the rows and columns of every operand
    buffer that belong to real points, and padding by the contract of workspace.h -- exact zeros on the rows >= M (2 M) of adjoint and
    tangent buffers, non-zero integer junk everywhere else: rows >= M of forward buffers, columns past the valid width (K of the 64- and
    128-wide inputs, N = 204 of the deformation network's layer 3, the fourth lane of the [..][4] buffers) on EVERY row, the rows
    [m_color, M) of the colour network's buffers (both members of a pair), and every buffer the weight gradients do not read."""
    dev = ws.device
    _, valid = row_counts(M, flags, m_color)
    step = 1 << 26
    for o in range(0, ws.numel(), step):
        n = min(step, ws.numel() - o)
        ws[o:o + n] = _junk((n,), gen, dev)
    for name, (kind, rk, cols) in OPERANDS.items():
        layers, R, ld = lay.shape[name]
        if layers == 0:
            continue
        v = valid[rk]
        zero_from = {"2Mp": 2 * M, "Mp": M, "Mc": M}[rk]
        for l in range(layers):
            stored = lay.view(ws, name, l)
            buf = _junk((R, ld), gen, dev)
            c = cols(l)
            buf[:v, :c] = torch.randint(-3, 4, (v, c), generator=gen, device=dev, dtype=torch.int8).float()
            if kind == "adj":
                buf[zero_from:] = 0.0
            stored.copy_(pack_frag(buf) if name in FRAG_BUFFERS else buf)
    return valid
