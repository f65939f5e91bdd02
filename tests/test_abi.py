"""CPU: the C-ABI library loads and exports every symbol include/endosurf_hip.h declares (no compute calls without a GPU)."""
import ctypes as C
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "endosurf_hip.h")


def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(es_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib():
    from endosurf_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_header_and_prototypes_agree(lib):
    from endosurf_amd import _lib
    decl = declared_functions()
    assert decl, "no declarations parsed"
    assert sorted(_lib.PROTOTYPES) == decl


def test_every_declared_symbol_is_exported(lib):
    for name in declared_functions():
        assert getattr(lib, name) is not None, name
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(REPO, "endosurf_amd", "lib", "libendosurf_hip.so")],
                         capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (es_[a-z0-9_]+)", out))
    assert set(declared_functions()) <= exported


def test_layout_queries_match_reference_shapes(lib):
    from endosurf_amd import _lib, params
    import weightgen
    assert lib.es_abi_version() == _lib.ABI_VERSION
    assert lib.es_param_floats() == 1654951            # reference parameter count
    lay = params.layout()
    state = weightgen.make_state(1, "init", True)
    assert set(lay) == set(state)
    end = 0
    for key, (off, shape) in sorted(lay.items(), key=lambda kv: kv[1][0]):
        assert off == end, key
        assert tuple(shape) == tuple(state[key].shape), key
        n = 1
        for s in shape:
            n *= s
        end = off + n
    assert end == lib.es_param_floats()
    flat = params.flatten_state(state)
    off, shape = lay["sdf_network.net.4.weight_v"]
    assert (flat[off:off + 256 * 295].reshape(256, 295) == state["sdf_network.net.4.weight_v"]).all()


def test_struct_sizes_match_header(lib):
    from endosurf_amd import _lib
    assert C.sizeof(_lib.es_points) == 5 * 8 + 6 * 4          # 5 pointers, 6 ints
    assert C.sizeof(_lib.es_composite_args) % 8 == 0
    assert lib.es_point_workspace_floats(0, 7) == 0
    n = lib.es_point_workspace_floats(100, 7)
    assert n > 128 * 20000 and lib.es_point_workspace_offset(100, 7, 2) >= 128 * 6      # x_c (3) and v = J d (3) precede the sdf buffer
    assert lib.es_kernel_name(0) == b"k_query_sdf"


def test_bad_arguments_return_error_codes(lib):
    from endosurf_amd import _lib
    assert lib.es_param_layout(7, 0, None, None, None, None, None) == 1
    assert b"out of range" in lib.es_last_error()
    p = _lib.es_points()
    p.M, p.mode = 4, 0
    assert lib.es_query_sdf(C.byref(p), None, None, None, 1, None) == 1      # null x/t
    p.mode = 3
    assert lib.es_query_sdf(C.byref(p), None, None, None, 1, None) == 1
    # es_query_sdf_tiles (ABI v6): the tile height is 0 (by batch size), 16, 32 or 64 -- checked before anything is launched
    import numpy as np
    buf = np.zeros(64, np.float32)
    q = _lib.es_points()
    q.M, q.mode, q.t_scalar = 4, 0, 1
    q.x, q.t = buf.ctypes.data, buf.ctypes.data          # (host addresses: never dereferenced, the call fails on its argument check)
    assert lib.es_query_sdf_tiles(C.byref(q), buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, 1, 24, None) == 1
    assert b"tile_points" in lib.es_last_error()


# ---- the header against endosurf_amd/_lib.py, type by type -----------------------------------------------------------------------------
STRUCTS = ("es_points", "es_composite_args", "es_render_args", "es_loss_args")
SCALARS = {"int": C.c_int, "float": C.c_float, "double": C.c_double, "long long": C.c_longlong, "unsigned long long": C.c_ulonglong,
           "int64_t": C.c_int64, "int32_t": C.c_int32, "unsigned char": C.c_ubyte, "char": C.c_char}


def header_text():
    return re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)


def split_decl(decl):
    """'const float* rays' -> ('float*', 'rays'); 'unsigned long long seed' -> ('unsigned long long', 'seed')."""
    m = re.fullmatch(r"\s*(.*?)\s*\b(\w+)\s*", decl, flags=re.S)
    ctype = re.sub(r"\bconst\b", " ", m.group(1))
    return re.sub(r"\s*\*\s*", "*", " ".join(ctype.split())), m.group(2)


def type_matches(ctype, ct, _lib, is_return=False):
    """Does the ctypes type ``ct`` of _lib.py carry the header's C type ``ctype``?"""
    if ctype.endswith("*"):
        base = ctype[:-1]
        if base in STRUCTS:
            return ct is C.POINTER(getattr(_lib, base))
        if base == "char" and is_return:
            return ct is C.c_char_p
        if ct is C.c_void_p:
            return True
        return base in SCALARS and hasattr(ct, "_type_") and ct is C.POINTER(ct._type_) and C.sizeof(ct._type_) == C.sizeof(SCALARS[base])
    if ctype in STRUCTS:
        return ct is getattr(_lib, ctype)
    return ct is SCALARS[ctype]


def header_structs():
    out = {}
    for body, name in re.findall(r"typedef\s+struct\s+\w+\s*\{(.*?)\}\s*(\w+)\s*;", header_text(), flags=re.S):
        fields = []
        for decl in filter(str.strip, body.split(";")):
            first, *more = decl.split(",")
            ctype, fname = split_decl(first)
            assert "*" not in "".join(more), decl      # 'int a, b' only for scalars
            fields += [(fname, ctype)] + [(n.strip(), ctype) for n in more]
        out[name] = fields
    return out


def header_prototypes():
    src = re.sub(r"typedef\s+struct\s+\w+\s*\{.*?\}\s*\w+\s*;", " ", header_text(), flags=re.S)
    src = re.sub(r"enum\s*\{.*?\}\s*;", " ", src, flags=re.S)
    src = re.sub(r"^\s*#.*$", " ", src, flags=re.M).replace('extern "C" {', " ").replace("}", " ")
    out = {}
    for decl in filter(str.strip, src.split(";")):
        m = re.fullmatch(r"\s*(.*?)\b(es_\w+)\s*\((.*)\)\s*", decl, flags=re.S)
        assert m, decl
        ret, _ = split_decl(m.group(1) + " _")
        args = [] if m.group(3).strip() == "void" else [split_decl(a)[0] for a in m.group(3).split(",")]
        out[m.group(2)] = (ret, args)
    return out


def header_constants():
    src = header_text()
    vals = {n: int(v) for n, v in re.findall(r"^\s*#define\s+(ES_\w+)\s+(-?\d+)\s*$", src, flags=re.M)}
    for body in re.findall(r"enum\s*\{(.*?)\}\s*;", src, flags=re.S):
        for item in filter(str.strip, body.split(",")):
            n, v = item.split("=")      # every enumerator of the header states its value
            vals[n.strip()] = int(v)
    return vals


def test_prototype_types_match_header(lib):
    from endosurf_amd import _lib
    protos = header_prototypes()
    assert sorted(protos) == sorted(_lib.PROTOTYPES)
    for name, (ret, args) in protos.items():
        res, argtypes = _lib.PROTOTYPES[name]
        assert type_matches(ret, res, _lib, is_return=True), (name, "return", ret, res)
        assert len(args) == len(argtypes), (name, "arity", len(args), len(argtypes))
        for i, (a, ct) in enumerate(zip(args, argtypes)):
            assert type_matches(a, ct, _lib), (name, i, a, ct)


def test_struct_fields_match_header(lib):
    from endosurf_amd import _lib
    structs = header_structs()
    assert sorted(structs) == sorted(STRUCTS)
    for sname, fields in structs.items():
        mirror = getattr(_lib, sname)._fields_
        assert [f for f, _ in fields] == [f for f, _ in mirror], sname
        for (fname, ctype), (_, ct) in zip(fields, mirror):
            assert type_matches(ctype, ct, _lib), (sname, fname, ctype, ct)


def test_constants_match_header(lib):
    from endosurf_amd import _lib
    consts = header_constants()
    assert _lib.ABI_VERSION == consts["ES_ABI_VERSION"] == lib.es_abi_version()
    assert _lib.QUERY_TILE_RACING == consts["ES_QUERY_TILE_RACING"]
    mirrored = [n for n in vars(_lib) if re.fullmatch(r"(PF|WS|BWD)_[A-Z0-9_]+", n)]
    assert {"PF_DEFORM", "PF_COLOR", "PF_SAVE", "PF_X3", "WS_XC", "WS_RGB", "WS_XCBAR", "WS_CURV", "WS_TBAR", "WS_VBAR",
            "BWD_CHAINS", "BWD_WGRAD_DEFORM", "BWD_WGRAD_SDF", "BWD_WGRAD_COLOR"} <= set(mirrored)
    for n in mirrored:
        assert getattr(_lib, n) == consts["ES_" + n], n


# ---- scratch sizes of the whole-stage calls: the formulas of ABI v14, restated -----------------------------------------------------------
def up64(n):
    return (n + 63) // 64 * 64


@pytest.mark.parametrize("N,n_samples,n_importance,steps", [(0, 32, 32, 4), (1, 2, 0, 0), (1, 32, 32, 4), (7, 33, 12, 3), (1024, 32, 32, 4)])
def test_sample_scratch_floats(lib, N, n_samples, n_importance, steps):
    want = 0
    if N > 0 and n_samples > 0:
        S = n_samples + max(n_importance, 0)
        n_imp = n_importance // steps if steps > 0 and n_importance > 0 else 0
        want = up64(N * S) * 4 + up64(N * n_samples) + 2 * up64(N * n_imp)
    assert lib.es_sample_scratch_floats(N, n_samples, n_importance, steps) == want


@pytest.mark.parametrize("N,n_steps", [(0, 128), (1, 2), (1000, 129), (1024, 128)])
def test_march_scratch_floats(lib, N, n_steps):
    want = 2 * up64(N * n_steps) + up64(N * 4) + 5 * up64(N) + up64(N * 3) if N > 0 and n_steps > 0 else 0
    assert lib.es_march_scratch_floats(N, n_steps) == want


@pytest.mark.parametrize("N,S", [(0, 4), (1, 1), (333, 17), (1024, 64)])
def test_render_scratch_floats(lib, N, S):
    want = up64(N * S) + up64(N * S) + 2 * up64(3 * N * S) if N > 0 and S > 0 else 0
    assert lib.es_render_scratch_floats(N, S) == want


# ---- refusals of the point-backward and ray-query entries (host addresses: never dereferenced, nothing launches) -------------------------
BACKWARD_ENTRIES = ("es_point_backward", "es_point_backward_det", "es_point_backward_stages", "es_point_backward_x3")


def backward_call(lib, entry, pts, flags, m_color=0, d_rgb=True, dweff=True, stages=15):
    import numpy as np
    buf = np.zeros(64, np.float32)
    b = buf.ctypes.data
    tail = {"es_point_backward": [], "es_point_backward_det": [b], "es_point_backward_stages": [b, stages], "es_point_backward_x3": [b]}[entry]
    head = [C.byref(pts), b] + ([b] if entry == "es_point_backward_x3" else [])      # packed (, packed_x3)
    return getattr(lib, entry)(*head, b, b, flags, m_color, b, b, b if d_rgb else None, b if dweff else None, *tail, None)


@pytest.fixture()
def host_points():
    import numpy as np
    from endosurf_amd import _lib
    buf = np.zeros(64, np.float32)
    p = _lib.es_points()
    p.M, p.mode, p.t_scalar = 256, 0, 1
    p.x, p.t, p.dirs = buf.ctypes.data, buf.ctypes.data, buf.ctypes.data
    p._keep = buf
    return p


@pytest.mark.parametrize("entry", BACKWARD_ENTRIES)
def test_backward_entries_refuse_bad_arguments(lib, host_points, entry):
    from endosurf_amd import _lib
    save = _lib.PF_DEFORM | _lib.PF_SAVE
    assert backward_call(lib, entry, host_points, _lib.PF_DEFORM) == 1                                   # no ES_PF_SAVE
    assert b"ES_PF_SAVE" in lib.es_last_error()
    assert backward_call(lib, entry, host_points, save, dweff=False) == 1                                # null dweff
    assert b"null buffer" in lib.es_last_error()
    assert backward_call(lib, entry, host_points, save | _lib.PF_COLOR, d_rgb=False) == 1                # colour without its adjoint
    assert b"colour adjoint" in lib.es_last_error()
    assert backward_call(lib, entry, host_points, save | _lib.PF_COLOR, m_color=100) == 1                # m_color not a multiple of 64
    assert b"m_color" in lib.es_last_error()


def test_staged_backward_refuses_bad_stages(lib, host_points):
    from endosurf_amd import _lib
    save = _lib.PF_DEFORM | _lib.PF_SAVE
    x3_chain = header_constants()["ES_PF_X3_CHAIN"]
    assert backward_call(lib, "es_point_backward_stages", host_points, save | x3_chain) == 1
    assert b"fp32 family" in lib.es_last_error()
    for stages in (0, 16):
        assert backward_call(lib, "es_point_backward_stages", host_points, save, stages=stages) == 1
        assert b"stages" in lib.es_last_error()


def test_query_sdf_rays_refuses_bad_arguments(lib, host_points):
    from endosurf_amd import _lib
    b = host_points._keep.ctypes.data
    assert lib.es_query_sdf_rays(C.byref(host_points), b, b, b, 64, None, 1, None) == 1                  # explicit points (mode 0)
    assert b"mode 1" in lib.es_last_error()
    r = _lib.es_points()
    r.M, r.mode, r.n_per_ray, r.ldz, r.rays, r.z = 256, 1, 32, 32, b, b
    assert lib.es_query_sdf_rays(C.byref(r), b, b, b, 31, None, 1, None) == 1                            # ld_out < n_per_ray
    assert b"ld_out" in lib.es_last_error()
