"""The host model of weight-norm and of the weight packings (pack_util.py) checked on the host: its tables against the headers and the
library's layout queries, its decoders (gathers) against encoders written the other way round (scatters, below), the tiling of the three
buffers, the exactness of the split on the values the GPU tests use -- and, the point of the file, that the comparison functions
test_gpu_pack.py applies to the kernels' output REJECT each of nine subtly wrong buffers."""
import math

import numpy as np
import pytest

import pack_util as P
import weightgen


# ---- encoders: what does (tile, k group, lane, element) hold?  Scatters, the kernels' direction ------------------------------------------
def encode32(buf, seg, B):
    off, kg, nt = P.SEG32[seg]
    t, g, lane, j = np.meshgrid(np.arange(nt), np.arange(kg), np.arange(64), np.arange(4), indexing="ij")
    buf[off + ((t * kg + g) * 64 + lane) * 4 + j] = B[8 * g + 2 * j + (lane >> 5), 32 * t + (lane & 31)]


def encode16(buf, i, B):
    off, kg = P.SEG16[i]
    t, g, lane, j = np.meshgrid(np.arange(16), np.arange(kg), np.arange(64), np.arange(4), indexing="ij")
    buf[off + ((t * kg + g) * 64 + lane) * 4 + j] = B[16 * g + 4 * j + (lane >> 4), 16 * t + (lane & 15)]


def encode_x3(words, i, planes, kperm=P.xr_kperm, order=(0, 1, 2)):
    """``words``: the buffer as 16-bit words.  planes = (B_h, B_m, B_l) as fp32 with 16 zero low bits; ``order[p]`` = the slot plane p is
    stored in."""
    c0, kg = P.X3[i]
    perm = np.array([[kperm(hi, j) for j in range(8)] for hi in range(2)])
    g, fb, lane, j = np.meshgrid(np.arange(kg), np.arange(8), np.arange(64), np.arange(8), indexing="ij")
    k, n = 16 * g + perm[lane >> 5, j], 32 * fb + (lane & 31)
    for p, B in enumerate(planes):
        w = (P.bits(B) >> np.uint32(16)).astype(np.uint16)
        words[((((c0 + g) * 8 + fb) * 3 + order[p]) * 64 + lane) * 8 + j] = w[k, n]


def pack_all(weff, use_deform=True, prefill=0, B_of=P.expected_B, skip16=()):
    packed = np.full(P.PACKED_TOTAL_FLOATS, prefill, np.uint32).view(np.float32)
    for seg, (off, kg, nt) in enumerate(P.SEG32):
        if use_deform or P.SEGS[seg].net != 0:
            encode32(packed, seg, B_of(weff, seg, 8 * kg, 32 * nt))
    for i, (off, kg) in enumerate(P.SEG16):
        if (use_deform or P.SEGS[P.P16_SEGS[i]].net != 0) and i not in skip16:
            encode16(packed, i, B_of(weff, P.P16_SEGS[i], 16 * kg, 256))
    return packed


def pack_all_x3(weff, use_deform=True, prefill=0, **kw):
    raw = np.full(P.PACKED_X3_BYTES // 2, prefill, np.uint16)
    for i, (c0, kg) in enumerate(P.X3):
        if use_deform or P.SEGS[P.XR_SEGS[i]].net != 0:
            encode_x3(raw, i, P.split3(P.expected_B(weff, P.XR_SEGS[i], 16 * kg, 256)), **kw)
    raw[P.XR_CHUNKS * P.X3_CHUNK_BYTES // 2:] = 0
    return raw.view(np.uint8)


@pytest.fixture(scope="module")
def flat():
    return P.flatten_state(weightgen.make_state(11, "trained", True))


@pytest.fixture(scope="module")
def weff(flat):
    return P.weff_buffer(flat)


# ---- tables --------------------------------------------------------------------------------------------------------------------------------
def test_tables_mirror_the_headers_and_the_library():
    assert len(P.SEGS) == 58 and len(P.P16_SEGS) == 17 and len(P.XR_SEGS) == 57 and sorted(P.XR_SEGS) != list(range(57))
    assert set(s.kreal for s in P.SEGS) >= {39, 52, 93, 204, 256} and set(s.nreal for s in P.SEGS) >= {39, 52, 93, 204, 256}
    assert sorted(set(k for row in P.LAYER_K for k in row)) == [39, 52, 256, 295, 349, 605]
    assert sorted(set(n for row in P.LAYER_N for n in row)) == [3, 204, 256, 257]
    assert abs(float(P.INV_SQRT2) - math.sqrt(0.5)) <= 2.0 ** -25 * math.sqrt(0.5)          # the nearest fp32 to 1 / sqrt(2)
    for s in P.SEGS:          # every window lies inside its layer's matrix
        N, K = P.LAYER_N[s.net][s.layer], P.LAYER_K[s.net][s.layer]
        rows, cols = (s.nreal, s.kreal) if s.dir == 0 else (s.kreal, s.nreal)
        assert s.row0 + rows <= N and s.col0 + cols <= K and s.skip == (1 if s.layer == 4 else 0), s
    try:
        from endosurf_amd import _lib
        lib = _lib.load()
    except Exception:
        return          # the totals against the library wherever it loads (test_gpu_pack.py repeats this on the GPU machine)
    P.check_library_layout(lib)


def test_flatten_matches_the_package(flat):
    try:
        from endosurf_amd import params
        ref = params.flatten_state(weightgen.make_state(11, "trained", True))
    except Exception:
        return          # (the library does not load here)
    assert np.array_equal(ref, flat)


# ---- round trips and tiling ----------------------------------------------------------------------------------------------------------------
def test_decoders_invert_the_encoders_on_every_segment():
    rng = np.random.default_rng(0)
    packed = np.full(P.PACKED_TOTAL_FLOATS, np.nan, np.float32)
    mats32, mats16 = [], []
    for seg, (off, kg, nt) in enumerate(P.SEG32):
        mats32.append(rng.normal(size=(8 * kg, 32 * nt)).astype(np.float32))
        encode32(packed, seg, mats32[-1])
    for i, (off, kg) in enumerate(P.SEG16):
        mats16.append(rng.normal(size=(16 * kg, 256)).astype(np.float32))
        encode16(packed, i, mats16[-1])
    assert not np.isnan(packed).any()          # the encoders covered the buffer
    for seg, B in enumerate(mats32):
        assert np.array_equal(P.decode32(packed, seg), B), P.SEGS[seg].name
    for i, B in enumerate(mats16):
        assert np.array_equal(P.decode16(packed, i), B), P.SEGS[P.P16_SEGS[i]].name
    shapes = {(s.kreal, s.nreal) for s in P.SEGS}
    assert shapes >= {(39, 256), (256, 39), (52, 256), (256, 52), (93, 256), (256, 93), (204, 256), (256, 204)}          # the ragged ones
    words = np.full(P.PACKED_X3_BYTES // 2, 0xFFFF, np.uint16)
    mats = []
    for i, (c0, kg) in enumerate(P.X3):
        mats.append(tuple(P.bf16_rne(rng.normal(size=(16 * kg, 256)).astype(np.float32)) for _ in range(3)))
        encode_x3(words, i, mats[-1])
    assert not (words[:P.XR_CHUNKS * P.X3_CHUNK_BYTES // 2] == 0xFFFF).any()
    for i, want in enumerate(mats):
        for got, w in zip(P.decode_x3(words.view(np.uint8), i), want):
            assert np.array_equal(got, w), P.SEGS[P.XR_SEGS[i]].name


def test_segments_tile_their_buffers():
    """Byte ranges of all 32-segments, all 16-segments, all split k-steps and the pad k-steps: disjoint, and their union is the buffer --
    by extent (consecutive ranges) and by index (every decoder index hit exactly once)."""
    ranges = [(4 * off, 4 * (off + kg * nt * 256)) for off, kg, nt in P.SEG32] + [(4 * off, 4 * (off + kg * 16 * 256)) for off, kg in P.SEG16]
    assert ranges[0][0] == 0 and ranges[-1][1] == 4 * P.PACKED_TOTAL_FLOATS and ranges[len(P.SEGS)][0] == 4 * P.PACKED_FLOATS
    assert all(a[1] == b[0] and a[0] < a[1] for a, b in zip(ranges, ranges[1:]))
    hits = np.zeros(P.PACKED_TOTAL_FLOATS, np.int32)
    for seg in range(len(P.SEGS)):
        np.add.at(hits, P.index32(seg).reshape(-1), 1)
    for i in range(len(P.P16_SEGS)):
        np.add.at(hits, P.index16(i).reshape(-1), 1)
    assert (hits == 1).all()
    x3 = [(c0 * P.X3_CHUNK_BYTES, (c0 + kg) * P.X3_CHUNK_BYTES) for c0, kg in P.X3]
    x3.append((P.XR_CHUNKS * P.X3_CHUNK_BYTES, (P.XR_CHUNKS + P.XR_PAD_CHUNKS) * P.X3_CHUNK_BYTES))
    assert x3[0][0] == 0 and x3[-1][1] == P.PACKED_X3_BYTES and all(a[1] == b[0] and a[0] < a[1] for a, b in zip(x3, x3[1:]))
    hits = np.zeros(P.PACKED_X3_BYTES // 2, np.int32)
    for i in range(len(P.XR_SEGS)):
        for p in range(3):
            np.add.at(hits, P.index_x3(i, p).reshape(-1), 1)
    n = P.XR_CHUNKS * P.X3_CHUNK_BYTES // 2
    assert (hits[:n] == 1).all() and (hits[n:] == 0).all() and hits.size - n == P.XR_PAD_CHUNKS * P.X3_CHUNK_BYTES // 2


# ---- the split -----------------------------------------------------------------------------------------------------------------------------
def test_bf16_rounds_to_nearest_even():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -23, -(1.0 + 2.0 ** -8), 0.0, -0.0], np.float32)
    want = np.array([1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -1.0, 0.0, -0.0], np.float32)
    assert np.array_equal(P.bits(P.bf16_rne(x)), P.bits(want))


def _exact(x):
    h, m, l = P.split3(x)
    assert not ((P.bits(h) | P.bits(m) | P.bits(l)) & np.uint32(0xFFFF)).any()          # three bf16
    return np.array_equal(h.astype(np.float64) + m.astype(np.float64) + l.astype(np.float64), x.astype(np.float64))


@pytest.mark.parametrize("name", ["init", "trained", "synthetic"])
def test_split_is_exact_on_the_values_the_gpu_tests_use(name):
    """The condition: x = 0 or 2^-100 <= |x| <= 2^100.  Outside it nothing is asserted exact anywhere (the last line shows why)."""
    flat_ = P.synthetic_flat() if name == "synthetic" else P.flatten_state(weightgen.make_state(11, name, True))
    w = P.weff_buffer(flat_)
    for x in (w, P.INV_SQRT2 * w):
        assert P.in_split_range(x) and _exact(x)
    sw = P.synthetic_weff()
    assert P.in_split_range(sw) and _exact(sw)
    for key, (wo, bo, N, K) in P.WEFF.items():
        if key[1] == 4:
            x = P.INV_SQRT2 * sw[wo:wo + N * K]
            assert P.in_split_range(x) and _exact(x)
    edge = np.array([2.0 ** -100, 2.0 ** 100, -2.0 ** -100, np.nextafter(np.float32(2.0 ** -100), np.float32(1)),
                     np.nextafter(np.float32(2.0 ** 100), np.float32(1))], np.float32)
    assert P.in_split_range(edge) and _exact(edge)
    h, m, l = P.split3(sw)
    assert (m == 0).any() and ((l == 0) & (m != 0)).any() and (l != 0).any()          # the cases the synthetic buffer promises
    assert not _exact(np.array([np.nextafter(np.float32(2.0 ** -126), np.float32(1))], np.float32))          # a residual below the normal range


# ---- the comparisons are alive -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_deform", [True, False])
def test_comparisons_accept_correct_buffers(flat, weff, use_deform):
    pre32, pre16 = 0x7FC12345, 0x7FC1
    P.check_packed(pack_all(weff, use_deform, pre32), weff, use_deform, pre32)
    P.check_packed_x3(pack_all_x3(weff, use_deform, pre16), weff, use_deform, pre16)
    assert P.check_weff(weff, flat, P.layers_of(use_deform)) <= 1.0          # fp64 rounded once to fp32: at most U


def _rejects(fn, *a):
    with pytest.raises(AssertionError):
        fn(*a)


def test_rejects_planes_m_and_l_exchanged(weff):
    _rejects(P.check_packed_x3, pack_all_x3(weff, order=(0, 2, 1)), weff, True)


def test_rejects_l_zeroed(weff):
    raw = pack_all_x3(weff).copy()
    raw.view(np.uint16)[P.index_x3(12, 2)] = 0          # one segment's low plane
    _rejects(P.check_packed_x3, raw, weff, True)


def test_rejects_identity_kperm(weff):
    _rejects(P.check_packed_x3, pack_all_x3(weff, kperm=lambda hi, j: 8 * hi + j), weff, True)


@pytest.mark.parametrize("where", ["32", "16", "x3", "x3_pad_chunk"])
def test_rejects_one_nonzero_pad_element(weff, where):
    packed, raw = pack_all(weff), pack_all_x3(weff).copy()
    tiny = np.float32(1e-30)
    if where == "32":          # SF4A: rows 39 (the one pad row of its 5 k groups)
        packed[P.index32(P.SEG_ID["SF4A"])[39, 7]] = tiny
    elif where == "16":          # DF3: column 204
        packed[P.index16(P.P16_SEGS.index(P.SEG_ID["DF3"]))[100, 204]] = tiny
    elif where == "x3":          # SF4A: k = 39 .. 63 of its four k-steps
        raw.view(np.uint16)[P.index_x3(P.XR_SEGS.index(P.SEG_ID["SF4A"]), 2)[63, 255]] = P.bits(P.bf16_rne(np.array([tiny])))[0] >> 16
    else:
        raw[-1] = 1
    if where in ("32", "16"):
        _rejects(P.check_packed, packed, weff, True)
    else:
        _rejects(P.check_packed_x3, raw, weff, True)


def _flipped(name):
    """expected_B with the F and R rules exchanged on one segment (same window origin, flat addressing as a kernel would do it)."""
    def B_of(weff, seg, kpad, npad):
        s = P.SEGS[seg]
        if s.name != name:
            return P.expected_B(weff, seg, kpad, npad)
        wo, bo, N, K = P.WEFF[s.net, s.layer]
        k, n = np.arange(s.kreal)[:, None], np.arange(s.nreal)[None, :]
        idx = (s.row0 + k) * K + s.col0 + n if s.dir == 0 else (s.row0 + n) * K + s.col0 + k
        B = np.zeros((kpad, npad), np.float32)
        B[:s.kreal, :s.nreal] = P.INV_SQRT2 * weff[wo + idx]
        return B
    return B_of


@pytest.mark.parametrize("name", ["SF4A", "SR4A"])
def test_rejects_exchanged_orientation(weff, name):
    _rejects(P.check_packed, pack_all(weff, B_of=_flipped(name)), weff, True)


def test_rejects_missing_skip_scale(weff):
    def B_of(w, seg, kpad, npad):
        B = P.expected_B(w, seg, kpad, npad)
        return B if P.SEGS[seg].name != "CF4S" else (B.astype(np.float64) / float(P.INV_SQRT2)).astype(np.float32)
    _rejects(P.check_packed, pack_all(weff, B_of=B_of), weff, True)


def test_rejects_a_16_packing_written_by_the_32_rule(weff):
    i = P.P16_SEGS.index(P.SEG_ID["SF1"])
    packed = pack_all(weff, skip16=(i,))
    off, kg = P.SEG16[i]
    B = P.expected_B(weff, P.SEG_ID["SF1"], 256, 256)
    t, g, lane, j = np.meshgrid(np.arange(8), np.arange(32), np.arange(64), np.arange(4), indexing="ij")          # the same 65 536 floats
    packed[off + ((t * 32 + g) * 64 + lane) * 4 + j] = B[8 * g + 2 * j + (lane >> 5), 32 * t + (lane & 31)]
    _rejects(P.check_packed, packed, weff, True)


def test_rejects_a_weff_row_off_by_2_to_the_minus_20(flat, weff):
    w = weff.copy()
    wo, bo, N, K = P.WEFF[2, 4]          # the longest rows: the widest bound, 13 U
    w[wo + 7 * K:wo + 8 * K] *= np.float32(1 + 2.0 ** -20)          # 16 U
    _rejects(P.check_weff, w, flat, P.LAYER_IDS)
    w = weff.copy()
    w[bo + 3] = np.nextafter(w[bo + 3], np.float32(np.inf))          # a bias one ulp off
    _rejects(P.check_weff, w, flat, P.LAYER_IDS)


def _dparams(flat, dweff):
    d = np.zeros(P.PARAM_FLOATS, np.float32)
    for key, (db, dg, dv) in P.weightnorm_bwd_fp64(flat, dweff).items():
        b, g, v, N, K = P.PARAM[key]
        d[b:b + N], d[g:g + N], d[v:v + N * K] = db, dg, dv.reshape(-1)
    return d


@pytest.mark.parametrize("kind", ["normal", "parallel", "single"])
def test_rejects_dg_without_the_skip_scale(flat, kind):
    dweff = P.make_dweff(flat, kind)
    d = _dparams(flat, dweff)
    worst_g, worst_v = P.check_wn_backward(d, flat, dweff, P.LAYER_IDS)
    assert worst_g <= 1.0 and worst_v <= 2.0          # fp64 rounded once to fp32: U; dv is measured at the ROUNDED dg, another U
    g_off = P.PARAM[1, 4][1]
    d[g_off + 5] = np.float32(float(d[g_off + 5]) / float(P.INV_SQRT2))          # one row of one layer 4
    _rejects(P.check_wn_backward, d, flat, dweff, P.LAYER_IDS)


def test_backward_model_is_the_derivative_of_the_forward_model(flat):
    """weightnorm_bwd_fp64 against a central difference of weightnorm_fp64 along one random direction (layer 4 without its factor)."""
    rng = np.random.default_rng(2)
    key = (1, 3)
    b, g, v, N, K = P.PARAM[key]
    wo, bo, _, _ = P.WEFF[key]
    dweff = rng.normal(size=P.WEFF_FLOATS).astype(np.float32)
    db, dg, dv = P.weightnorm_bwd_fp64(flat, dweff, [key])[key]
    direction = np.zeros(P.PARAM_FLOATS)
    direction[g:g + N * (K + 1)] = rng.normal(size=N * (K + 1))
    f = lambda p: float((P.weightnorm_fp64(p, [key])[key][0] * dweff[wo:wo + N * K].reshape(N, K)).sum())
    eps = 1e-6
    num = (f(flat.astype(np.float64) + eps * direction) - f(flat.astype(np.float64) - eps * direction)) / (2 * eps)
    ana = float((dg * direction[g:g + N]).sum() + (dv.reshape(-1) * direction[v:v + N * K]).sum())
    assert abs(num - ana) <= 1e-7 * max(abs(ana), 1.0)
