"""Host model of weight-norm and of the three weight packings (csrc/pack.hip, k_pack_x3r of csrc/query_x3.hip), written from the layouts as
the headers DOCUMENT them -- the comment above SegDesc and the one above P16_SEGS in csrc/arch.h, the chunk comment of k_pack_x3r and
xr_kperm of csrc/x3r_core.h -- not from the kernels' loops: the decoders below are gathers (where does B[k][n] live?), the kernels and the
encoders of test_pack_host.py are scatters (what does thread / lane / element hold?).  Plain numpy; fp64 wherever something is computed.

The tables (LAYER_K, LAYER_N, SEGS, P16_SEGS, XR_SEGS, INV_SQRT2, XR_PAD_CHUNKS) are parsed from the headers' text, so a changed table
changes the model with it; test_pack_host.py cross-checks the totals derived here against the library's layout queries.

The comparison functions at the end (check_weff, check_packed, check_packed_x3, check_wn_backward) are shared by the host tests, which
show that each of them REJECTS a subtly wrong buffer, and by test_gpu_pack.py, which applies them to what the kernels wrote."""
import ctypes as C
import os
import re
from collections import namedtuple

import numpy as np

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "endosurf_amd", "csrc")
U = 2.0 ** -24          # unit roundoff of fp32: one correctly rounded operation has relative error <= U, one "1 ulp" operation <= 2 U
NETS, LAYERS = 3, 9
SPLIT_MIN, SPLIT_MAX = 2.0 ** -100, 2.0 ** 100          # the range on which split3 is asserted exact (see split3)

Seg = namedtuple("Seg", "name net layer dir row0 col0 kreal nreal skip")


# ---- the tables, from the headers' text --------------------------------------------------------------------------------------------
def _text(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _no_comments(s):
    return re.sub(r"//[^\n]*", "", s)


def _layer_table(text, name):
    body = re.search(name + r"\[NETS\]\[LAYERS\]\s*=\s*\{(.*?)\};", text, re.S).group(1)
    return tuple(tuple(int(v) for v in row.split(",")) for row in re.findall(r"\{([^{}]*)\}", body))


def _name_list(text, pattern):
    body = _no_comments(re.search(pattern, text, re.S).group(1))
    return [n.strip() for n in body.split(",") if n.strip()]


def parse_tables():
    arch, x3 = _text("arch.h"), _text("x3r_core.h")
    names = _name_list(arch, r"enum Seg\s*:\s*int\s*\{(.*?)\};")
    assert names[-1] == "SEG_COUNT"
    names = names[:-1]
    segs = []
    for line in re.search(r"SegDesc SEGS\[SEG_COUNT\]\s*=\s*\{\n(.*?)\n\};", arch, re.S).group(1).split("\n"):
        m = re.match(r"\s*\{([^{}]*)\},?\s*//\s*(\w+)", line)
        if m is None:
            continue          # the column legend
        vals = [int(v) for v in m.group(1).split(",")]
        assert len(vals) == 8 and m.group(2) == names[len(segs)], line          # the row's own comment names the enum entry it fills
        segs.append(Seg(m.group(2), *vals))
    assert len(segs) == len(names)
    idx = {n: i for i, n in enumerate(names)}
    return dict(LAYER_K=_layer_table(arch, "LAYER_K"), LAYER_N=_layer_table(arch, "LAYER_N"), SEGS=tuple(segs),
                P16=tuple(idx[n] for n in _name_list(arch, r"P16_SEGS\[\]\s*=\s*\{(.*?)\};")),
                XR=tuple(idx[n] for n in _name_list(x3, r"XR_SEGS\[\]\s*=\s*\{(.*?)\};")),
                INV_SQRT2=float(re.search(r"INV_SQRT2\s*=\s*([0-9.eE+-]+)f\s*;", arch).group(1)),
                XR_PAD_CHUNKS=int(re.search(r"XR_PAD_CHUNKS\s*=\s*(\d+)\s*;", x3).group(1)))


_T = parse_tables()
LAYER_K, LAYER_N, SEGS, P16_SEGS, XR_SEGS = _T["LAYER_K"], _T["LAYER_N"], _T["SEGS"], _T["P16"], _T["XR"]
INV_SQRT2 = np.float32(_T["INV_SQRT2"])          # the fp32 constant the pack folds into skip-layer weights and k_weightnorm_bwd applies
XR_PAD_CHUNKS = _T["XR_PAD_CHUNKS"]
SEG_ID = {s.name: i for i, s in enumerate(SEGS)}
NET_NAMES = ("deform_network", "sdf_network", "color_network")


def cdiv(a, b):
    return -(-a // b)


# ---- flat parameter buffer and effective-weight buffer (arch.h: "for net, for layer: bias[N], weight_g[N], weight_v[N*K]; then variance",
# "for net, for layer: W[N*K] (row-major), b[N]") ------------------------------------------------------------------------------------
def param_layout():
    """({(net, layer): (bias_off, g_off, v_off, N, K)}, total floats including the variance slot)"""
    out, off = {}, 0
    for net in range(NETS):
        for l in range(LAYERS):
            N, K = LAYER_N[net][l], LAYER_K[net][l]
            out[net, l] = (off, off + N, off + 2 * N, N, K)
            off += N * (2 + K)
    return out, off + 1


def weff_layout():
    """({(net, layer): (w_off, b_off, N, K)}, total floats)"""
    out, off = {}, 0
    for net in range(NETS):
        for l in range(LAYERS):
            N, K = LAYER_N[net][l], LAYER_K[net][l]
            out[net, l] = (off, off + N * K, N, K)
            off += N * (K + 1)
    return out, off


PARAM, PARAM_FLOATS = param_layout()
WEFF, WEFF_FLOATS = weff_layout()
LAYER_IDS = tuple((net, l) for net in range(NETS) for l in range(LAYERS))          # index 9 * network + layer of es_weightnorm_backward_layers


def check_library_layout(lib):
    """The layouts derived above against the library's own queries (es_param_layout, es_weff_layout and the four totals)."""
    assert lib.es_param_floats() == PARAM_FLOATS and lib.es_weff_floats() == WEFF_FLOATS
    assert lib.es_packed_floats() == PACKED_TOTAL_FLOATS and lib.es_packed_x3_bytes() == PACKED_X3_BYTES
    assert lib.es_param_variance_off() == PARAM_FLOATS - 1
    for (net, l), (b, g, v, N, K) in PARAM.items():
        ob, og, ov, w, wb, n, k = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_int(), C.c_int()
        assert lib.es_param_layout(net, l, C.byref(ob), C.byref(og), C.byref(ov), C.byref(n), C.byref(k)) == 0
        assert lib.es_weff_layout(net, l, C.byref(w), C.byref(wb)) == 0
        assert (ob.value, og.value, ov.value, n.value, k.value) == (b, g, v, N, K) and (w.value, wb.value, N, K) == WEFF[net, l]


def flatten_state(state):
    """weightgen.make_state's dictionary -> the flat fp32 parameter buffer; missing (deformation) keys stay zero."""
    flat = np.zeros(PARAM_FLOATS, np.float32)
    for (net, l), (b, g, v, N, K) in PARAM.items():
        pre = f"{NET_NAMES[net]}.net.{l}."
        if pre + "bias" in state:
            flat[b:b + N] = state[pre + "bias"].reshape(-1)
            flat[g:g + N] = state[pre + "weight_g"].reshape(-1)
            flat[v:v + N * K] = state[pre + "weight_v"].reshape(-1)
    flat[-1] = state["deviation_network.variance"]
    return flat


def layers_of(use_deform):
    return [k for k in LAYER_IDS if use_deform or k[0] != 0]


# ---- weight-norm in fp64 -----------------------------------------------------------------------------------------------------------------
def _bgv(flat, key):
    b, g, v, N, K = PARAM[key]
    return (flat[b:b + N].astype(np.float64), flat[g:g + N].astype(np.float64), flat[v:v + N * K].astype(np.float64).reshape(N, K))


def weightnorm_fp64(flat, layers=LAYER_IDS):
    """{(net, layer): (W [N][K], b [N])}: W = g v / ||v|| per row."""
    out = {}
    for key in layers:
        b, g, v = _bgv(flat, key)
        out[key] = (g[:, None] * v / np.sqrt((v * v).sum(1))[:, None], b)
    return out


def weff_buffer(flat, layers=LAYER_IDS, fill=0.0):
    """weightnorm_fp64 rounded to fp32 in the effective-weight buffer's layout: what a correct k_weff writes, up to its rounding."""
    w = np.full(WEFF_FLOATS, fill, np.float32)
    for key, (W, b) in weightnorm_fp64(flat, layers).items():
        wo, bo, N, K = WEFF[key]
        w[wo:wo + N * K] = W.reshape(-1)
        w[bo:bo + N] = b
    return w


def weightnorm_bwd_fp64(flat, dweff, layers=LAYER_IDS):
    """{(net, layer): (db [N], dg [N], dv [N][K])}.  dweff of layer 4 of every
    network is the gradient with respect to the weight the kernels USE, W / sqrt(2) (k_weightnorm_bwd, csrc/pack.hip): dW = s dweff with
    s = the library's fp32 constant INV_SQRT2 there, 1 elsewhere; dg = <dW, v> / ||v||, dv = g / ||v|| (dW - dg v / ||v||)."""
    out = {}
    for key in layers:
        b, g, v = _bgv(flat, key)
        wo, bo, N, K = WEFF[key]
        dW = dweff[wo:wo + N * K].astype(np.float64).reshape(N, K) * (float(INV_SQRT2) if key[1] == 4 else 1.0)
        nv = np.sqrt((v * v).sum(1))
        dg = (dW * v).sum(1) / nv
        dv = (g / nv)[:, None] * (dW - dg[:, None] * v / nv[:, None])
        out[key] = (dweff[bo:bo + N].copy(), dg, dv)
    return out


# ---- the split ---------------------------------------------------------------------------------------------------------------------------
def bf16_rne(x):
    """fp32 -> the nearest bf16 (ties to even), returned as fp32 with 16 zero low bits.  Finite inputs."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    r = (b + (np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1)))) & np.uint32(0xFFFF0000)
    return r.view(np.float32)


def split3(x):
    """(h, m, l) = (bf16(x), bf16(x - h), bf16(x - h - m)) with the subtractions in fp32, as split_pair (csrc/x3r_core.h) forms them.
    h + m + l == x exactly for x = 0 and for SPLIT_MIN <= |x| <= SPLIT_MAX: three 8-bit significands cover the 24 bits of x as long as no
    residual underflows (|x| >= 2^-100 keeps x - h - m >= 2^-124 normal) and h does not overflow.  Outside that range nothing is asserted."""
    x = np.ascontiguousarray(x, np.float32)
    h = bf16_rne(x)
    r = x - h
    m = bf16_rne(r)
    l = bf16_rne(r - m)
    return h, m, l


def in_split_range(x):
    a = np.abs(np.asarray(x, np.float64))
    return bool(((a == 0) | ((a >= SPLIT_MIN) & (a <= SPLIT_MAX))).all())


def xr_kperm(hi, j):
    """csrc/x3r_core.h: position j (0..7) of lane half hi -> k offset inside the 16-wide k-step."""
    return 4 * hi + j if j < 4 else 8 + 4 * hi + (j - 4)


# ---- where the three packings keep B[k][n] -----------------------------------------------------------------------------------------------
def seg32_layout():
    """([(float offset, kg, nt)] per segment, PACKED_FLOATS): "[nt][g][lane]" float4 tiles, kg = ceil(kreal / 8), nt = ceil(nreal / 32)."""
    out, off = [], 0
    for s in SEGS:
        kg, nt = cdiv(s.kreal, 8), cdiv(s.nreal, 32)
        out.append((off, kg, nt))
        off += kg * nt * 64 * 4
    return out, off


def seg16_layout():
    """([(float offset, kg)] per entry of P16_SEGS, PACKED_TOTAL_FLOATS): "[nt16][g][lane]" float4 tiles behind the 32-packing,
    kg = ceil(kreal / 16), always 16 column tiles."""
    out, off = [], seg32_layout()[1]
    for i in P16_SEGS:
        kg = cdiv(SEGS[i].kreal, 16)
        out.append((off, kg))
        off += kg * 16 * 64 * 4
    return out, off


X3_UNIT = 64 * 16                    # bytes of one (feature block, plane) unit: 64 lanes x 16 B
X3_CHUNK_BYTES = 8 * 3 * X3_UNIT     # one k-step: [8 feature blocks][3 planes][64 lanes] x 16 B


def x3_layout():
    """([(first k-step, k-steps)] per entry of XR_SEGS, XR_CHUNKS): 2 * ceil(kreal / 32) k-steps of 16 k each (the stream works in pairs)."""
    out, c = [], 0
    for i in XR_SEGS:
        kg = 2 * cdiv(SEGS[i].kreal, 32)
        out.append((c, kg))
        c += kg
    return out, c


SEG32, PACKED_FLOATS = seg32_layout()
SEG16, PACKED_TOTAL_FLOATS = seg16_layout()
X3, XR_CHUNKS = x3_layout()
PACKED_X3_BYTES = (XR_CHUNKS + XR_PAD_CHUNKS) * X3_CHUNK_BYTES


def index32(seg):
    """float index of B[k][n] of 32-segment ``seg``, [8 kg][32 nt]: "element j of the float4 of lane l is B[8g + 2j + (l>>5)][32nt + (l&31)]"."""
    off, kg, nt = SEG32[seg]
    k, n = np.arange(8 * kg)[:, None], np.arange(32 * nt)[None, :]
    lane = 32 * (k % 2) + n % 32
    return off + (((n // 32) * kg + k // 8) * 64 + lane) * 4 + (k % 8) // 2


def index16(i):
    """float index of B[k][n] of the i-th 16-segment, [16 kg][256]: "element j of lane l = B[16g + 4j + (l>>4)][16 nt16 + (l&15)]"."""
    off, kg = SEG16[i]
    k, n = np.arange(16 * kg)[:, None], np.arange(256)[None, :]
    lane = 16 * (k % 4) + n % 16
    return off + (((n // 16) * kg + k // 16) * 64 + lane) * 4 + (k % 16) // 4


def index_x3(i, plane):
    """index, in 16-bit words, of plane ``plane`` of B[k][n] of the i-th split segment, [16 k-steps][256]: k-step c = first + k / 16 holds
    [8 feature blocks][3 planes][64 lanes] x 16 B; lane (n % 32, half hi) of feature block n / 32 holds the 8 bf16 of positions j = 0..7,
    position j <-> k offset xr_kperm(hi, j); the two bf16 of a 32-bit word are (low half, high half) = positions (2i, 2i + 1)."""
    c0, kg = X3[i]
    kk = np.arange(16)
    hi_of, j_of = np.zeros(16, np.int64), np.zeros(16, np.int64)
    for hi in range(2):
        for j in range(8):
            hi_of[xr_kperm(hi, j)], j_of[xr_kperm(hi, j)] = hi, j
    assert sorted(xr_kperm(hi, j) for hi in range(2) for j in range(8)) == list(kk)
    k, n = np.arange(16 * kg)[:, None], np.arange(256)[None, :]
    lane = 32 * hi_of[k % 16] + n % 32
    unit = ((c0 + k // 16) * 8 + n // 32) * 3 + plane
    return (unit * 64 + lane) * 8 + j_of[k % 16]


def decode32(packed, seg):
    return packed[index32(seg)]


def decode16(packed, i):
    return packed[index16(i)]


def bf16_words_to_f32(w):
    return (w.astype(np.uint32) << np.uint32(16)).view(np.float32)


def decode_x3(raw, i):
    """(B_h, B_m, B_l) as fp32 over [k-steps x 16][256] from the byte buffer of es_pack_x3 (a bf16 is an fp32 with 16 zero low bits)."""
    w = np.ascontiguousarray(raw).view(np.uint16)
    return tuple(bf16_words_to_f32(w[index_x3(i, p)]) for p in range(3))


def expected_B(weff, seg, kpad, npad):
    """B[k][n] of a segment with its pads, from an effective-weight buffer: fp32(scale * W[...]) on the real extent (ONE fp32 multiply:
    nothing to contract), +0.0 elsewhere.  dir F: B[k][n] = W[row0 + n][col0 + k]; dir R: B[k][n] = W[row0 + k][col0 + n]."""
    s = SEGS[seg]
    wo, bo, N, K = WEFF[s.net, s.layer]
    W = weff[wo:wo + N * K].reshape(N, K)
    B = np.zeros((kpad, npad), np.float32)
    sc = INV_SQRT2 if s.skip else np.float32(1.0)
    if s.dir == 0:
        B[:s.kreal, :s.nreal] = sc * W[s.row0:s.row0 + s.nreal, s.col0:s.col0 + s.kreal].T
    else:
        B[:s.kreal, :s.nreal] = sc * W[s.row0:s.row0 + s.kreal, s.col0:s.col0 + s.nreal]
    return B


# ---- the comparisons ---------------------------------------------------------------------------------------------------------------------
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def assert_bits(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = g != w
    if bad.any():
        at = tuple(int(i) for i in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ by bits, first at {at}: got {got[at]!r} ({int(g[at]):#x}), "
                             f"expected {want[at]!r} ({int(w[at]):#x})")


def _written(seg, use_deform):
    return use_deform or SEGS[seg].net != 0


def check_packed(packed, weff, use_deform, prefill=None):
    """Both fragment packings against the effective weights they were packed from: every real element bit-equal to fp32(scale * weff),
    every pad +0.0 by bits; with use_deform = 0 the deformation segments must hold ``prefill`` (a 32-bit pattern) if one is given."""
    assert packed.shape == (PACKED_TOTAL_FLOATS,) and packed.dtype == np.float32
    for what, ids, dec in (("32x32x2", range(len(SEGS)), decode32), ("16x16x4", range(len(P16_SEGS)), decode16)):
        for i in ids:
            seg = i if what == "32x32x2" else P16_SEGS[i]
            got = dec(packed, i)
            if _written(seg, use_deform):
                assert_bits(got, expected_B(weff, seg, *got.shape), f"{what} packing of {SEGS[seg].name} [k][n]")
            elif prefill is not None:
                assert (bits(got) == np.uint32(prefill)).all(), f"{what} packing of {SEGS[seg].name}: written although use_deform = 0"


def check_packed_x3(raw, weff, use_deform, prefill=None):
    """The split-precision packing against the numpy split of the effective weights it was packed from: each plane bit-equal to split3,
    h + m + l == scale * weff exactly (asserted on the DECODED planes, after checking the values are inside the exactness range), pads
    zero in all three planes, the pad k-steps behind the last segment zero; untouched segments as in check_packed (16-bit pattern)."""
    assert raw.shape == (PACKED_X3_BYTES,) and raw.dtype == np.uint8
    for i, seg in enumerate(XR_SEGS):
        s = SEGS[seg]
        planes = decode_x3(raw, i)
        if not _written(seg, use_deform):
            if prefill is not None:
                for p in planes:
                    assert (bits(p) >> np.uint32(16) == np.uint32(prefill)).all(), f"split packing of {s.name}: written although use_deform = 0"
            continue
        B = expected_B(weff, seg, *planes[0].shape)
        assert in_split_range(B), f"{s.name}: a weight outside the exactness range of the split"
        for name, got, want in zip("hml", planes, split3(B)):
            assert_bits(got, want, f"split packing of {s.name}, plane {name} [k][n]")
        total = planes[0].astype(np.float64) + planes[1].astype(np.float64) + planes[2].astype(np.float64)
        assert np.array_equal(total, B.astype(np.float64)), f"split packing of {s.name}: h + m + l != scale * weff"
        pad = np.ones(B.shape, bool)
        pad[:s.kreal, :s.nreal] = False
        for name, got in zip("hml", planes):
            assert not bits(got)[pad].any(), f"split packing of {s.name}, plane {name}: a pad element is not +0"
    assert not raw[XR_CHUNKS * X3_CHUNK_BYTES:].any(), "the pad k-steps behind the last segment must be zero"


def weff_bound(K):
    """Relative error bound of one element of k_weff's W = (g / sqrtf(ss)) * v, ss = sum v^2, in units of U (see test_gpu_pack.py::test_weff):
    ss: T = ceil(K / 64) fused multiply-adds per lane, then 6 shuffle adds, all terms >= 0: (T + 6) U relative, halved by the square root;
    sqrtf <= 1 ulp = 2 U, the division <= 1 ulp = 2 U, the multiply U."""
    return (cdiv(K, 64) + 6) / 2.0 + 5.0


def _gamma(c):
    return c * U / (1.0 - c * U)          # (1 + U)^c - 1 <= c U / (1 - c U): the first-order count with its higher-order terms


def check_weff(weff, flat, layers):
    """Effective weights against fp64, element by element, relative, no absolute term (the forward has no cancellation); biases
    bit-equal.  Returns the largest error in units of U over all elements."""
    worst = 0.0
    for key, (W, b) in weightnorm_fp64(flat, layers).items():
        wo, bo, N, K = WEFF[key]
        got = weff[wo:wo + N * K].astype(np.float64).reshape(N, K)
        err, ref = np.abs(got - W), np.abs(W)
        assert np.isfinite(got).all(), key
        bad = err > _gamma(weff_bound(K)) * ref
        if bad.any():
            r, c = (int(i) for i in np.argwhere(bad)[0])
            raise AssertionError(f"weff of layer {key}: {int(bad.sum())} elements beyond {weff_bound(K)} U relative, first at row {r} column {c}: "
                                 f"got {got[r, c]!r}, fp64 {W[r, c]!r} ({err[r, c] / ref[r, c] / U:.2f} U)")
        nz = ref > 0
        if nz.any():
            worst = max(worst, float((err[nz] / ref[nz]).max() / U))
        assert_bits(weff[bo:bo + N], b.astype(np.float32), f"bias of layer {key}")
    return worst


def wn_bwd_constants(key):
    """(c_dg, c_dv, c_prop) in units of U for k_weightnorm_bwd (derivation in test_gpu_pack.py::test_weightnorm_backward)."""
    T, s = cdiv(LAYER_K[key[0]][key[1]], 64), 1 if key[1] == 4 else 0
    return 1.5 * (T + 6) + 5 + s, T + 19 + s, T + 6 + s


def check_wn_backward(dparams, flat, dweff, layers):
    """(db, dg, dv) of es_weightnorm_backward against fp64.  db: a bit-equal copy.  dg: |error| <= c_dg U A / ||v||, A = sum |dW v| (the
    sum without its cancellation).  dv, elementwise, with n_k = |g| / ||v|| (|dW_k| + |dg| |v_k| / ||v||):
      * against the fp64 formula evaluated at the DEVICE's dg (the stage on its own input):  |error| <= c_dv U n_k;
      * against fp64 throughout: the error of dg enters as well, |error| <= c_dv U n_k + c_prop U |g| / ||v|| (A / ||v||) |v_k| / ||v||.
    Returns the largest (dg error / (A / ||v||), dv error / n_k at the device's dg) in units of U."""
    worst_g = worst_v = 0.0
    for key, (db, dg, dv) in weightnorm_bwd_fp64(flat, dweff, layers).items():
        b, g, v = _bgv(flat, key)
        bo_p, go_p, vo_p, N, K = PARAM[key]
        wo, bo, _, _ = WEFF[key]
        c_dg, c_dv, c_prop = wn_bwd_constants(key)
        assert_bits(dparams[bo_p:bo_p + N], db, f"db of layer {key}")
        dW = dweff[wo:wo + N * K].astype(np.float64).reshape(N, K) * (float(INV_SQRT2) if key[1] == 4 else 1.0)
        nv = np.sqrt((v * v).sum(1))
        A = np.abs(dW * v).sum(1) / nv
        got_g = dparams[go_p:go_p + N].astype(np.float64)
        got_v = dparams[vo_p:vo_p + N * K].astype(np.float64).reshape(N, K)
        assert np.isfinite(got_g).all() and np.isfinite(got_v).all(), key
        eg = np.abs(got_g - dg)
        bad = eg > _gamma(c_dg) * A
        if bad.any():
            r = int(np.argwhere(bad)[0][0])
            raise AssertionError(f"dg of layer {key}: {int(bad.sum())} rows beyond {c_dg} U of sum |dW v| / ||v||, first row {r}: got {got_g[r]!r}, "
                                 f"fp64 {dg[r]!r} ({eg[r] / A[r] / U:.1f} U)")
        if (A > 0).any():
            worst_g = max(worst_g, float((eg[A > 0] / A[A > 0]).max() / U))
        gs, vn = (np.abs(g) / nv)[:, None], np.abs(v) / nv[:, None]
        dv_own = (g / nv)[:, None] * (dW - got_g[:, None] * v / nv[:, None])          # the fp64 formula at the device's dg
        n_own = gs * (np.abs(dW) + np.abs(got_g)[:, None] * vn)
        n_ref = gs * (np.abs(dW) + np.abs(dg)[:, None] * vn)
        for what, err, lim in (("at the device's dg", np.abs(got_v - dv_own), _gamma(c_dv) * n_own),
                               ("in fp64 throughout", np.abs(got_v - dv), _gamma(c_dv) * n_ref + _gamma(c_prop) * gs * A[:, None] * vn)):
            bad = err > lim
            if bad.any():
                r, c = (int(i) for i in np.argwhere(bad)[0])
                raise AssertionError(f"dv of layer {key} against the formula {what}: {int(bad.sum())} elements beyond the bound, first at row {r} "
                                     f"column {c}: got {got_v[r, c]!r}, error {err[r, c]!r}, bound {lim[r, c]!r}")
        e_own = np.abs(got_v - dv_own)
        if (n_own > 0).any():
            worst_v = max(worst_v, float((e_own[n_own > 0] / n_own[n_own > 0]).max() / U))
    return worst_g, worst_v


# ---- inputs shared by the host and the GPU tests -----------------------------------------------------------------------------------------
def synthetic_flat(seed=7):
    """A flat parameter buffer whose rows stress the row reduction, on top of a "trained" state.  Row r of every layer, by r % 6:
    0: v normal with ||v|| = 10^U(-3, 3), g = +-10^U(-3, 3);  1: g = 0;  2: v with a single non-zero entry;  3: v = +-1 alternating;
    4: g negated;  5: as generated."""
    import weightgen
    flat = flatten_state(weightgen.make_state(seed, "trained", True))
    rng = np.random.default_rng(seed)
    for (net, l), (bo, go, vo, N, K) in PARAM.items():
        g, v = flat[go:go + N], flat[vo:vo + N * K].reshape(N, K)          # views
        for r in range(N):
            kind = r % 6
            if kind == 0:
                row = rng.normal(size=K)
                v[r] = row * (10.0 ** rng.uniform(-3, 3) / np.linalg.norm(row))
                g[r] = rng.choice([-1.0, 1.0]) * 10.0 ** rng.uniform(-3, 3)
            elif kind == 1:
                g[r] = 0.0
            elif kind == 2:
                v[r] = 0.0
                v[r, rng.integers(K)] = rng.choice([-1.0, 1.0]) * 10.0 ** rng.uniform(-3, 3)
            elif kind == 3:
                v[r] = rng.choice([-1.0, 1.0]) * (1.0 - 2.0 * (np.arange(K) % 2))
            elif kind == 4:
                g[r] = -g[r]
    return flat


def make_dweff(flat, kind, seed=3):
    """An effective-weight gradient: "normal" (standard normal), "parallel" (every row a multiple of its v: dv cancels to ~0),
    "single" (one non-zero per row).  Bias gradients standard normal."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=WEFF_FLOATS).astype(np.float32)
    if kind == "normal":
        return d
    for key, (wo, bo, N, K) in WEFF.items():
        v = flat[PARAM[key][2]:PARAM[key][2] + N * K].reshape(N, K)
        D = d[wo:wo + N * K].reshape(N, K)
        if kind == "parallel":
            D[:] = rng.normal(size=(N, 1)).astype(np.float32) * v
        elif kind == "single":
            keep = rng.integers(K, size=N)
            val = D[np.arange(N), keep].copy()
            D[:] = 0.0
            D[np.arange(N), keep] = val
        else:
            raise ValueError(kind)
    return d


def synthetic_weff(seed=5):
    """An effective-weight buffer of values inside the exactness range of the split that exercise its rounding: +-0, powers of two from
    2^-100 to 2^100, their nextafter neighbours (carries in the rounding), values whose m and l planes (bf16-exact) or whose l plane
    (16-bit significands) are exactly zero, and random significands at random exponents.  Layer 4 of every network is packed times
    1/sqrt(2): its values stay >= 2^-99 so that the product is in range too."""
    rng = np.random.default_rng(seed)
    e = np.arange(-100, 101)
    p2 = np.ldexp(1.0, e).astype(np.float32)
    up, down = np.nextafter(p2, np.float32(np.inf)), np.nextafter(p2[1:], np.float32(0))
    sig8 = np.ldexp(rng.integers(128, 256, size=4096).astype(np.float64), rng.integers(-107, 93, size=4096)).astype(np.float32)
    sig16 = np.ldexp(rng.integers(1 << 15, 1 << 16, size=4096).astype(np.float64), rng.integers(-115, 85, size=4096)).astype(np.float32)
    pool = np.concatenate([np.zeros(2, np.float32), p2, up, down, sig8, sig16])
    pool = np.concatenate([pool, -pool])
    w = np.ldexp(rng.uniform(1.0, 2.0, size=WEFF_FLOATS), rng.integers(-100, 100, size=WEFF_FLOATS)).astype(np.float32)
    w *= rng.choice([-1.0, 1.0], size=WEFF_FLOATS).astype(np.float32)
    at = rng.random(WEFF_FLOATS) < 0.5
    w[at] = pool[rng.integers(pool.size, size=int(at.sum()))]
    w = np.where(np.abs(w) > np.float32(SPLIT_MAX), np.float32(SPLIT_MAX), w).astype(np.float32)          # 2^100 (1 + ...) from the random part
    for (net, l), (wo, bo, N, K) in WEFF.items():
        if l == 4:
            seg = w[wo:wo + N * K]
            small = (seg != 0) & (np.abs(seg) < np.float32(2.0 ** -99))
            seg[small] *= np.float32(2.0)
            big = np.abs(seg) >= np.float32(2.0 ** 100)          # (the product of 2^100 and the constant rounds inside the range anyway)
            seg[big] *= np.float32(0.5)
    assert in_split_range(w)
    return w
