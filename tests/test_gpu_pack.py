"""Weight-norm, the three weight packings and the weight-norm backward, every element checked: k_weff, k_pack, k_pack16 and
k_weightnorm_bwd of csrc/pack.hip and k_pack_x3r of csrc/query_x3.hip against the host model of pack_util.py (fp64 where something is
computed, bits where something is only moved), on buffers prefilled with a recognisable NaN between guard words, so that what a call
leaves unwritten is asserted as well.  The comparison functions are pack_util's; test_pack_host.py shows that each of them rejects a
subtly wrong buffer.  Every test is a handful of single launches on the architecture's own sizes plus vectorised numpy.

u = 2^-24 below is the unit roundoff of fp32: a correctly rounded operation has relative error <= u; an operation the HIP
documentation gives as "1 ulp" (sqrtf, the fp32 division) <= 2 u."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import pack_util as P
import weightgen

pytestmark = pytest.mark.gpu

PRE32, PRE16 = 0x7FC12345, 0x7FC1          # prefills: a NaN no kernel computes, as fp32 and as bf16
GUARD = 64                                 # guard words on either side of a buffer (keeps the 16-byte alignment of the float4 stores)


def _L():
    from endosurf_amd import _lib
    lib = _lib.load()
    _lib.check(lib.es_init(), "es_init")
    return lib, _lib


class Guarded:
    """A device buffer of ``n`` words (int32 or int16) prefilled with ``pattern`` between two runs of guard words."""
    def __init__(self, n, pattern, dtype=torch.int32):
        self.full = torch.full((n + 2 * GUARD,), pattern, dtype=dtype, device="cuda")
        self.view, self.n, self.pattern = self.full[GUARD:GUARD + n], n, pattern

    def host(self):
        torch.cuda.synchronize()
        a = self.full.cpu().numpy()
        assert (a[:GUARD] == self.pattern).all() and (a[GUARD + self.n:] == self.pattern).all(), "a guard word was overwritten"
        return a[GUARD:GUARD + self.n]


def _flat(name, use_deform=True):
    if name == "synthetic":
        return P.synthetic_flat()
    return P.flatten_state(weightgen.make_state(11, name, use_deform))


@functools.lru_cache(maxsize=None)
def _packed(name, use_deform):
    """(flat, weff, packed, packed_x3 bytes) of one parameter set: es_weightnorm_pack and es_pack_x3 through the raw ABI, once."""
    lib, _lib = _L()
    flat = _flat(name, use_deform)
    dflat = torch.from_numpy(flat).cuda()
    weff, packed = Guarded(P.WEFF_FLOATS, PRE32), Guarded(P.PACKED_TOTAL_FLOATS, PRE32)
    x3 = Guarded(P.PACKED_X3_BYTES // 2, PRE16, torch.int16)
    _lib.check(lib.es_weightnorm_pack(_lib.ptr(dflat), _lib.ptr(weff.view), _lib.ptr(packed.view), int(use_deform), _lib.stream_ptr()), "es_weightnorm_pack")
    _lib.check(lib.es_pack_x3(_lib.ptr(weff.view), _lib.ptr(x3.view), int(use_deform), _lib.stream_ptr()), "es_pack_x3")
    out = (flat, weff.host().view(np.float32), packed.host().view(np.float32), x3.host().view(np.uint8))
    for a in out:
        a.setflags(write=False)
    return out


SETS = [(n, d) for n in ("init", "trained", "synthetic") for d in (True, False)]


def test_layout_queries_match_the_host_model():
    P.check_library_layout(_L()[0])


@pytest.mark.parametrize("name,use_deform", SETS)
def test_weff(name, use_deform):
    """k_weff against fp64, element by element, RELATIVE, no absolute term (W = g v / ||v|| has no cancellation); biases bit-equal.

    The bound, from the kernel's operation count (one wavefront per row of K entries, T = ceil(K / 64)):
      ss = sum v^2: T fused multiply-adds per lane (one rounding each), then 6 shuffle adds; every term is >= 0, so the relative error of
           ss is <= (T + 6) u and that of its square root <= (T + 6) / 2 u;
      sqrtf: 1 ulp <= 2 u;  g / sqrt: 1 ulp <= 2 u;  scale * v: one correctly rounded multiply, u.
    Total: ((T + 6) / 2 + 5) u, between 8.5 u (K = 39) and 13 u (K = 605) -- asserted as c u / (1 - c u), the count with its higher-order
    terms.  Condition: no underflow in v^2 that matters to ss (rows here have ||v|| >= 1e-3).  Measured on gfx950: DESIGN.md section 3.
    With use_deform = 0 the deformation layers' part of the NaN-prefilled buffer keeps its prefill; guard words around weff and packed
    keep theirs (Guarded.host)."""
    flat, weff, packed, raw = _packed(name, use_deform)
    worst = P.check_weff(weff, flat, P.layers_of(use_deform))
    print(f"weff[{name}, use_deform={use_deform}]: largest relative error {worst:.3f} u")
    first_written = 0 if use_deform else P.WEFF[1, 0][0]
    assert (P.bits(weff[:first_written]) == PRE32).all(), "use_deform = 0 must leave the deformation layers' part of weff untouched"
    assert not (P.bits(weff[first_written:]) == PRE32).any()


@pytest.mark.parametrize("name,use_deform", SETS)
def test_fragment_packings(name, use_deform):
    """k_pack and k_pack16 on the device's own weff: real elements bit-equal to fp32(scale * weff) (one multiply: nothing to contract),
    pads +0.0 by bits, no prefill left with use_deform = 1, exactly the deformation segments left with use_deform = 0."""
    flat, weff, packed, raw = _packed(name, use_deform)
    P.check_packed(packed, weff, use_deform, PRE32)
    kept = P.bits(packed) == PRE32
    want = np.zeros(P.PACKED_TOTAL_FLOATS, bool)
    if not use_deform:
        for seg, s in enumerate(P.SEGS):
            if s.net == 0:
                want[P.index32(seg).reshape(-1)] = True
        for i, seg in enumerate(P.P16_SEGS):
            if P.SEGS[seg].net == 0:
                want[P.index16(i).reshape(-1)] = True
    assert np.array_equal(kept, want)


@pytest.mark.parametrize("name,use_deform", SETS)
def test_split_packing(name, use_deform):
    """k_pack_x3r on the device's own weff: planes h, m, l bit-equal to the numpy split, h + m + l == scale * weff exactly on every
    element, pads and the four pad k-steps zero, written and untouched regions as for the fragment packings."""
    flat, weff, packed, raw = _packed(name, use_deform)
    P.check_packed_x3(raw, weff, use_deform, PRE16)
    kept = raw.view(np.uint16) == PRE16
    want = np.zeros(P.PACKED_X3_BYTES // 2, bool)
    if not use_deform:
        for i, seg in enumerate(P.XR_SEGS):
            if P.SEGS[seg].net == 0:
                for p in range(3):
                    want[P.index_x3(i, p).reshape(-1)] = True
    assert np.array_equal(kept, want)


def test_split_packing_of_values_that_exercise_the_rounding():
    """es_pack_x3 alone on a synthetic weff inside the exactness range: +-0, 2^-100 .. 2^100, nextafter neighbours of powers of two,
    values whose m or l plane is exactly zero (pack_util.synthetic_weff)."""
    lib, _lib = _L()
    w = P.synthetic_weff()
    x3 = Guarded(P.PACKED_X3_BYTES // 2, PRE16, torch.int16)
    dw = torch.from_numpy(w).cuda()
    _lib.check(lib.es_pack_x3(_lib.ptr(dw), _lib.ptr(x3.view), 1, _lib.stream_ptr()), "es_pack_x3")
    raw = x3.host().view(np.uint8)
    P.check_packed_x3(raw, w, True, PRE16)
    assert not (raw.view(np.uint16) == PRE16).any()


def _backward(flat, dweff, use_deform):
    lib, _lib = _L()
    d = Guarded(P.PARAM_FLOATS, PRE32)
    a, b = torch.from_numpy(flat).cuda(), torch.from_numpy(dweff).cuda()
    _lib.check(lib.es_weightnorm_backward(_lib.ptr(a), _lib.ptr(b), _lib.ptr(d.view), int(use_deform), _lib.stream_ptr()), "es_weightnorm_backward")
    return d.host().view(np.float32)


@pytest.mark.parametrize("name,kind,use_deform", [(n, k, True) for n in ("trained", "synthetic") for k in ("normal", "parallel", "single")]
                         + [("trained", "normal", False), ("synthetic", "parallel", False)])
def test_weightnorm_backward(name, kind, use_deform):
    """k_weightnorm_bwd against fp64 for three kinds of dweff (standard normal; every row parallel to v, so that dv cancels to ~0; one
    non-zero per row), with measures that do not hide the cancellation.  db is a bit-equal copy.

    One wavefront per row, T = ceil(K / 64), s = 1 for layer 4 of a network (dW = fl(dweff * INV_SQRT2): one more rounding) else 0,
    A = sum_k |dW_k v_k|, n = ||v||.  ss = sum v^2 as in test_weff: relative error (T + 6) u;  inv = 1 / sqrtf(ss): (T + 6) / 2 u from
    ss, 2 u sqrtf, 2 u division =: E u with E = (T + 6) / 2 + 4.
      dg = dot * inv: dot is T fused multiply-adds and 6 adds of SIGNED terms (+ s): |error| <= (T + 6 + s) u A; times inv (E u) and
           one multiply (u), with |dg| <= A / n:      |dg error| <= (1.5 (T + 6) + 5 + s) u A / n          [c_dg: 15.5 .. 30 u]
      dv_k = gs (dW_k - c v_k), gs = fl(g inv) [(E + 1) u], c = fl(dg inv) [(E + 1) u at the device's dg], the product c v_k and the
           difference one rounding each (or one, fused), the last multiply u.  With n_k = |g| / n (|dW_k| + |dg| |v_k| / n), the sum of
           the magnitudes of the two terms that cancel:
             against the fp64 formula at the DEVICE's dg:   |error| <= (2 E + 5 + s) u n_k = (T + 19 + s) u n_k   [c_dv: 20 .. 30 u]
             against fp64 throughout, dg's own error (bounded by A / n, not by |dg|) enters times |g| / n |v_k| / n:
                                                            |error| <= c_dv u n_k + (T + 6 + s) u |g| / n (A / n) |v_k| / n
    All three are asserted (pack_util.check_wn_backward), as c u / (1 - c u).  Measured on gfx950: DESIGN.md section 3.
    The variance slot and, with use_deform = 0, the deformation slices of the NaN-prefilled dparams stay untouched."""
    flat = _flat(name)
    dweff = P.make_dweff(flat, kind)
    d = _backward(flat, dweff, use_deform)
    worst_g, worst_v = P.check_wn_backward(d, flat, dweff, P.layers_of(use_deform))
    print(f"weightnorm_backward[{name}, {kind}, use_deform={use_deform}]: dg {worst_g:.3f} u of sum |dW v| / ||v||, dv {worst_v:.3f} u of n_k")
    first_written = 0 if use_deform else P.PARAM[1, 0][0]
    assert (P.bits(d[:first_written]) == PRE32).all() and P.bits(d)[-1] == PRE32
    assert not (P.bits(d[first_written:-1]) == PRE32).any()


PARTITIONS = {
    "one_run": [(0, 27)],
    "single_layers": [(i, 1) for i in range(27)],
    "networks": [(0, 9), (9, 9), (18, 9)],
    "uneven_with_empty_pieces": [(0, 0), (0, 5), (5, 0), (5, 1), (6, 13), (13, 0), (19, 8), (27, 0)],
}


@functools.lru_cache(maxsize=None)
def _layers_case():
    flat = _flat("trained")
    dweff = P.make_dweff(flat, "normal", seed=9)
    return flat, dweff, _backward(flat, dweff, True)


def _layer_calls(pieces):
    lib, _lib = _L()
    flat, dweff, whole = _layers_case()
    d = Guarded(P.PARAM_FLOATS, PRE32)
    a, b = torch.from_numpy(flat).cuda(), torch.from_numpy(dweff).cuda()
    for first, n in pieces:
        _lib.check(lib.es_weightnorm_backward_layers(_lib.ptr(a), _lib.ptr(b), _lib.ptr(d.view), first, n, _lib.stream_ptr()), "es_weightnorm_backward_layers")
    return d.host().view(np.float32), whole


@pytest.mark.parametrize("name", sorted(PARTITIONS))
def test_weightnorm_backward_layers_partitions(name):
    """Every partition of [0, 27), its pieces called in shuffled order on a NaN-prefilled dparams, gives the bits of the whole call
    (the variance slot's prefill included)."""
    pieces = list(PARTITIONS[name])
    assert sum(n for _, n in pieces) == 27
    np.random.default_rng(len(pieces)).shuffle(pieces)
    got, whole = _layer_calls([tuple(int(v) for v in p) for p in pieces])
    P.assert_bits(got, whole, f"partition {name}")


def test_weightnorm_backward_layers_writes_only_its_slices():
    got, whole = _layer_calls([(13, 2)])          # sdf layers 4 and 5
    lo, hi = P.PARAM[1, 4][0], P.PARAM[1, 6][0]
    P.assert_bits(got[lo:hi], whole[lo:hi], "the slices of layers 13 and 14")
    assert (P.bits(got[:lo]) == PRE32).all() and (P.bits(got[hi:]) == PRE32).all()


@pytest.mark.parametrize("case", ["negative_first", "past_the_end", "null_params", "null_dweff", "null_dparams"])
def test_weightnorm_backward_layers_refusals(case):
    """Status 1 with a message, nothing launched: the poisoned output stays poisoned."""
    lib, _lib = _L()
    flat, dweff, _ = _layers_case()
    d = Guarded(P.PARAM_FLOATS, PRE32)
    a, b = torch.from_numpy(flat).cuda(), torch.from_numpy(dweff).cuda()
    pa, pb, pd, first, n = _lib.ptr(a), _lib.ptr(b), _lib.ptr(d.view), 3, 2
    if case == "negative_first":
        first = -1
    elif case == "past_the_end":
        first, n = 20, 8
    elif case == "null_params":
        pa = None
    elif case == "null_dweff":
        pb = None
    else:
        pd = None
    assert lib.es_weightnorm_backward_layers(pa, pb, pd, first, n, _lib.stream_ptr()) == 1
    assert lib.es_last_error()
    assert (P.bits(d.host()) == PRE32).all()


# ---- consumers do not read what the pack leaves unwritten ------------------------------------------------------------------------------
def _consumers(fill):
    """Every consumer of the three buffers through the raw ABI with use_deform = 0, on buffers prefilled with the byte ``fill`` before
    es_weightnorm_pack / es_pack_x3 (use_deform = 0) wrote their part.  {name: host tensor}."""
    lib, _lib = _L()
    st = _lib.stream_ptr
    flat = torch.from_numpy(_flat("trained", False)).cuda()
    byte_buf = lambda nbytes: torch.full((nbytes,), fill, dtype=torch.uint8, device="cuda")
    weff, packed, px3 = byte_buf(4 * P.WEFF_FLOATS), byte_buf(4 * P.PACKED_TOTAL_FLOATS), byte_buf(P.PACKED_X3_BYTES)
    _lib.check(lib.es_weightnorm_pack(_lib.ptr(flat), _lib.ptr(weff), _lib.ptr(packed), 0, st()), "es_weightnorm_pack")
    _lib.check(lib.es_pack_x3(_lib.ptr(weff), _lib.ptr(px3), 0, st()), "es_pack_x3")
    flags = _lib.PF_COLOR | _lib.PF_SAVE
    wg = torch.empty(int(lib.es_wgrad_scratch_floats()), device="cuda")
    out = {}
    for family, M in (("fp32", 200), ("split", 130)):          # a ragged last tile | two 128-point blocks
        rng = np.random.default_rng(M)
        x = torch.from_numpy(rng.uniform(-0.8, 0.8, size=(M, 3)).astype(np.float32)).cuda()
        t = torch.from_numpy(rng.uniform(size=(M,)).astype(np.float32)).cuda()
        dirs = rng.normal(size=(M, 3))
        dirs = torch.from_numpy((dirs / np.linalg.norm(dirs, axis=-1, keepdims=True)).astype(np.float32)).cuda()
        adj = {k: torch.from_numpy(rng.normal(size=s).astype(np.float32)).cuda() for k, s in (("sdf", (M,)), ("go", (M, 3)), ("rgb", (M, 3)))}
        pts = _lib.es_points()
        pts.x, pts.t, pts.dirs, pts.mode, pts.t_scalar, pts.n_per_ray, pts.ldz, pts.M = _lib.ptr(x), _lib.ptr(t), _lib.ptr(dirs), 0, 0, 1, 1, M
        ws = torch.zeros(int(lib.es_point_workspace_floats(M, flags)), device="cuda")
        dweff = torch.zeros(P.WEFF_FLOATS, device="cuda")
        if family == "fp32":
            for tp in (16, 32, 64):
                q = torch.full((M,), float("nan"), device="cuda")
                _lib.check(lib.es_query_sdf_tiles(C.byref(pts), _lib.ptr(packed), _lib.ptr(weff), _lib.ptr(q), 0, tp, st()), "es_query_sdf_tiles")
                out[f"query_{tp}"] = q
            _lib.check(lib.es_point_forward(C.byref(pts), _lib.ptr(packed), _lib.ptr(weff), _lib.ptr(ws), flags, 0, st()), "es_point_forward")
        else:
            q = torch.full((M,), float("nan"), device="cuda")
            _lib.check(lib.es_query_sdf_x3(C.byref(pts), _lib.ptr(px3), _lib.ptr(weff), _lib.ptr(q), 0, None, 0, st()), "es_query_sdf_x3")
            out["query_x3"] = q
            _lib.check(lib.es_point_forward_x3(C.byref(pts), _lib.ptr(packed), _lib.ptr(px3), _lib.ptr(weff), _lib.ptr(ws), flags, 0, st()),
                       "es_point_forward_x3")
        torch.cuda.synchronize()
        for name, buf, width in (("xc", _lib.WS_XC, 3), ("sdf", _lib.WS_SDF, 1), ("feat", _lib.WS_FEAT, 256), ("gc", _lib.WS_GC, 3),
                                 ("go", _lib.WS_GO, 3), ("rgb", _lib.WS_RGB, 3)):
            off = int(lib.es_point_workspace_offset(M, flags, buf))
            out[f"{family}_{name}"] = ws[off:off + M * width].clone()
        if family == "fp32":
            _lib.check(lib.es_point_backward_det(C.byref(pts), _lib.ptr(packed), _lib.ptr(weff), _lib.ptr(ws), flags, 0, _lib.ptr(adj["sdf"]),
                                                 _lib.ptr(adj["go"]), _lib.ptr(adj["rgb"]), _lib.ptr(dweff), _lib.ptr(wg), st()), "es_point_backward_det")
        else:
            _lib.check(lib.es_point_backward_x3(C.byref(pts), _lib.ptr(packed), _lib.ptr(px3), _lib.ptr(weff), _lib.ptr(ws), flags, 0,
                                                _lib.ptr(adj["sdf"]), _lib.ptr(adj["go"]), _lib.ptr(adj["rgb"]), _lib.ptr(dweff), _lib.ptr(wg), st()),
                       "es_point_backward_x3")
        out[f"{family}_dweff"] = dweff
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def test_consumers_do_not_read_what_the_pack_leaves_unwritten():
    """use_deform = 0 through the raw ABI: the packs leave the deformation network's part of weff, packed and packed_x3 as the caller
    allocated it.  Whatever is there -- zero bytes or 0xFF bytes (NaN as fp32 and as bf16) -- the queries (16-, 32-, 64-point tiles,
    split precision), the point forward and the deterministic backward of both families give the same bits, all finite.  (Reading a
    NaN cannot fault; this only compares results.)"""
    zero, ones = _consumers(0x00), _consumers(0xFF)
    assert sorted(zero) == sorted(ones) and len(zero) == 4 + 2 * 7
    for k in sorted(zero):
        assert bool(torch.isfinite(ones[k]).all()) and bool(torch.isfinite(zero[k]).all()), f"{k}: not finite"
        assert torch.equal(zero[k].view(torch.int32), ones[k].view(torch.int32)), f"{k} depends on what the pack left unwritten"
        assert bool((zero[k] != 0).any()), f"{k}: nothing was computed"
