"""CPU: the numpy twins of the mesh export (endosurf_amd.meshing mesh_clean / cluster_vertices, endosurf_amd.data ply_body / write_ply /
read_ply) on hand-made inputs with the answers written out, and the argument checks of the new C entry points (nothing is launched).
tests/test_gpu_mesh_export.py compares the device against these twins and imports the hand-made cases below."""
import ctypes as C
import os

import numpy as np
import pytest

from endosurf_amd import data as D
from endosurf_amd import meshing as M

I64 = np.int64


def _verts(V, seed=0):
    return np.random.default_rng(seed).normal(size=(V, 3)).astype(np.float32)


# name -> (V, triangles, kept triangle ids, degenerate, duplicates)
CLEAN_CASES = {
    "twelve": (10, [[0, 1, 2], [2, 3, 3], [1, 2, 3], [4, 4, 4], [2, 0, 1], [3, 4, 5], [2, 1, 0], [5, 4, 3], [4, 5, 6], [3, 2, 1], [5, 6, 7],
                    [6, 7, 5]], [0, 2, 5, 8, 10], 2, 5),
    "first_and_last": (7, [[1, 2, 3], [4, 5, 6], [0, 1, 2], [2, 3, 1], [6, 5, 4]], [0, 1, 2], 0, 2),
    "rotated_first": (7, [[2, 3, 1], [0, 1, 2], [1, 2, 3], [3, 2, 1]], [0, 1], 0, 2),
    "none": (4, np.zeros((0, 3), I64), [], 0, 0),
    "one": (4, [[3, 1, 2]], [0], 0, 0),
    "one_degenerate": (4, [[3, 1, 3]], [], 1, 0),
    "all_the_same": (3, [[0, 1, 2], [1, 2, 0], [2, 0, 1], [0, 2, 1], [2, 1, 0]], [0], 0, 4),
}


def clean_case(name):
    V, tris, kept, n_deg, n_dup = CLEAN_CASES[name]
    return _verts(V, len(name)), np.asarray(tris, I64).reshape(-1, 3), kept, n_deg, n_dup


@pytest.mark.parametrize("name", list(CLEAN_CASES))
def test_mesh_clean_on_hand_made_meshes(name):
    v, f, kept, n_deg, n_dup = clean_case(name)
    cv, cf, vmap, st = M.mesh_clean(v, f)
    assert cf.dtype == np.int32 and vmap.dtype == np.int64 and cf.shape == (len(kept), 3)
    assert np.array_equal(cf, f[kept]) and np.array_equal(cv, v) and np.array_equal(vmap, np.arange(len(v)))
    assert st == {"degenerate": n_deg, "duplicates": n_dup, "kept_triangles": len(kept)}
    kv, kf, kmap, kst = M.mesh_clean(v, f, compact=True)
    used = np.unique(f[kept])
    assert kst == st and np.array_equal(kmap, used) and np.array_equal(kv, v[used])
    assert np.array_equal(kmap[kf], f[kept])                                  # the same triangles under the new names


def test_mesh_clean_written_out():
    v, f, _, _, _ = clean_case("twelve")
    kv, kf, kmap, st = M.mesh_clean(v, f, compact=True)
    assert kf.tolist() == [[0, 1, 2], [1, 2, 3], [3, 4, 5], [4, 5, 6], [5, 6, 7]]
    assert kmap.tolist() == [0, 1, 2, 3, 4, 5, 6, 7] and kv.shape == (8, 3)          # vertices 8 and 9 are used by nothing
    assert st == {"degenerate": 2, "duplicates": 5, "kept_triangles": 5}
    v, f, _, _, _ = clean_case("first_and_last")
    assert M.mesh_clean(v, f, compact=True)[1].tolist() == [[1, 2, 3], [4, 5, 6], [0, 1, 2]]


def test_mesh_clean_keeps_large_indices_apart():
    """Indices that agree in their low 21 bits are different vertices."""
    big = (1 << 21) + 1
    f = np.array([[0, 1, 2], [0, 1, big + 1], [big, 1, 2], [2, 1, big], [0, 1, 2]], I64)
    _, cf, _, st = M.mesh_clean(np.zeros((big + 2, 3), np.float32), f)
    assert cf.tolist() == f[:3].tolist() and st == {"degenerate": 0, "duplicates": 2, "kept_triangles": 3}
    with pytest.raises(ValueError):
        M.mesh_clean(np.zeros((3, 3), np.float32), [[0, 1, 3]])
    with pytest.raises(ValueError):
        M.mesh_clean(np.zeros((3, 2), np.float32), [[0, 1, 2]])


# ---- clustering ------------------------------------------------------------------------------------------------------------------------
CLUSTER_V = np.array([[-0.5, 0.2, 0.2], [-1.0, 0.2, 0.2], [0.0, 0.0, 0.0], [0.999, 0.5, 0.5], [1.0, 0.0, 0.0], [-1.5, 0.0, 0.0]], np.float32)
CLUSTER_F = np.array([[0, 2, 4], [1, 3, 4], [0, 1, 2], [5, 0, 2], [4, 2, 0]], I64)


def test_cluster_written_out():
    """Cell 1 from the origin: floor, not truncation (-0.5 and -1.0 share cell -1, -1.5 is in -2), and a vertex exactly on a boundary
    (1.0, -1.0) belongs to the cell that starts there."""
    att = np.arange(12, dtype=np.float32).reshape(6, 2)
    v, f, a, vc, st = M.cluster_vertices(CLUSTER_V, CLUSTER_F, 1.0, attributes=att)
    assert vc.dtype == np.int32 and vc.tolist() == [1, 1, 2, 2, 3, 0]
    f32 = np.float32
    want = np.array([[-1.5, 0, 0], [-0.75, f32(0.2), f32(0.2)], [(0.0 + float(f32(0.999))) / 2, 0.25, 0.25], [1, 0, 0]], np.float64).astype(f32)
    assert v.dtype == f32 and np.array_equal(v, want)
    assert np.array_equal(a, np.array([[10, 11], [1, 2], [5, 6], [8, 9]], f32))
    assert f.dtype == np.int32 and f.tolist() == [[1, 2, 3], [0, 1, 2]]
    assert st == {"cells": 4, "largest_cell": 2, "degenerate": 1, "duplicates": 2, "kept_triangles": 2}
    v2, f2, a2, vc2, st2 = M.cluster_vertices(CLUSTER_V, CLUSTER_F, 1.0)
    assert a2 is None and np.array_equal(v2, v) and np.array_equal(f2, f) and st2 == st
    # an origin moves the boundaries: with origin 0.5 the cells are [-1.5, -0.5), [-0.5, 0.5), [0.5, 1.5)
    _, _, _, vc3, st3 = M.cluster_vertices(CLUSTER_V, CLUSTER_F, 1.0, origin=(0.5, 0.0, 0.0))
    assert vc3.tolist() == [1, 0, 1, 2, 2, 0] and st3["cells"] == 3


def test_cluster_collapse_and_renumber():
    rng = np.random.default_rng(3)
    v = rng.uniform(-1, 1, size=(40, 3)).astype(np.float32)
    f = rng.integers(0, 40, size=(60, 3))
    cv, cf, _, vc, st = M.cluster_vertices(v, f, 100.0, origin=(-50.0, -50.0, -50.0))          # everything in one cell
    assert cv.shape == (1, 3) and cf.shape == (0, 3) and (vc == 0).all()
    seq = np.zeros(3)
    for row in v.astype(np.float64):
        seq += row
    assert np.array_equal(cv[0], (seq / 40).astype(np.float32))                                # the sum in index order
    assert st == {"cells": 1, "largest_cell": 40, "degenerate": 60, "duplicates": 0, "kept_triangles": 0}
    cv, cf, _, vc, st = M.cluster_vertices(v, f, 1e-5)                                          # every vertex its own cell
    order = np.lexsort((v[:, 2], v[:, 1], v[:, 0]))                                              # distinct cells along x already
    assert st["cells"] == 40 and st["largest_cell"] == 1 and np.array_equal(cv, v[order]) and np.array_equal(vc[order], np.arange(40))
    _, ef, _, est = M.mesh_clean(v, f)
    assert np.array_equal(cf, vc[ef]) and {k: st[k] for k in est} == est


def test_cluster_range_and_arguments():
    f = np.zeros((0, 3), I64)
    half = float(1 << 20)
    ok = np.array([[-half * 0.5, 0, 0], [half * 0.5 - 0.25, 0, 0]], np.float32)               # cells -2^20 and 2^20 - 1
    assert M.cluster_vertices(ok, f, 0.5)[4]["cells"] == 2
    for bad in ([half * 0.5, 0, 0], [0, -half * 0.5 - 0.5, 0], [0, 0, 1e9], [np.nan, 0, 0], [0, np.inf, 0]):
        with pytest.raises(ValueError, match="2\\^20"):
            M.cluster_vertices(np.array([bad], np.float32), f, 0.5)
    for cell in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="cell"):
            M.cluster_vertices(ok, f, cell)
    with pytest.raises(ValueError, match="attributes"):
        M.cluster_vertices(ok, f, 1.0, attributes=np.zeros((2, 9), np.float32))
    with pytest.raises(ValueError, match="attributes"):
        M.cluster_vertices(ok, f, 1.0, attributes=np.zeros((3, 2), np.float32))
    v, t, a, vc, st = M.cluster_vertices(np.zeros((0, 3), np.float32), f, 1.0)
    assert v.shape == (0, 3) and t.shape == (0, 3) and vc.shape == (0,) and st["cells"] == 0 and st["largest_cell"] == 0


# ---- PLY -----------------------------------------------------------------------------------------------------------------------------------
def ply_inputs(V, T, seed=0):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(V, 3)).astype(np.float32)
    f = rng.integers(0, max(V, 1), size=(T, 3)).astype(np.int32)
    c = rng.uniform(-0.1, 1.1, size=(V, 3)).astype(np.float32)
    n = rng.normal(size=(V, 3)).astype(np.float32)
    return v, f, c, n


PLY_COMBOS = [(False, False), (True, False), (False, True), (True, True)]


@pytest.mark.parametrize("faces", [True, False])
@pytest.mark.parametrize("with_colors,with_normals", PLY_COMBOS)
def test_ply_round_trip(tmp_path, faces, with_colors, with_normals):
    v, f, c, n = ply_inputs(7, 5, seed=1)
    path = str(tmp_path / "m.ply")
    D.write_ply(path, v, f if faces else None, c if with_colors else None, n if with_normals else None)
    got = D.read_ply(path)
    want = {"vertices": v}
    if faces:
        want["triangles"] = f
    if with_colors:
        want["colors"] = D.to8b(c)
    if with_normals:
        want["normals"] = n
    assert set(got) == set(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    vb = 12 + (12 if with_normals else 0) + (3 if with_colors else 0)
    assert os.path.getsize(path) == len(D.ply_header(7, 5 if faces else None, with_colors, with_normals)) + 7 * vb + (13 * 5 if faces else 0)


def test_ply_header_and_length_literally(tmp_path):
    v = np.array([[1.0, 2.0, 3.0], [-1.0, 0.5, 0.25]], np.float32)
    path = str(tmp_path / "lit.ply")
    D.write_ply(path, v, np.array([[0, 1, 1]]), colors=np.array([[0.0, 0.5, 1.0], [2.0, -1.0, 0.2]]), normals=v[::-1], comment="frame 3")
    header = (b"ply\nformat binary_little_endian 1.0\ncomment frame 3\nelement vertex 2\nproperty float x\nproperty float y\n"
              b"property float z\nproperty float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\n"
              b"property uchar blue\nelement face 1\nproperty list uchar int vertex_indices\nend_header\n")
    raw = open(path, "rb").read()
    assert raw[:len(header)] == header and len(raw) == len(header) + 2 * 27 + 13
    body = raw[len(header):]
    assert body[:12] == np.array([1, 2, 3], "<f4").tobytes() and body[12:24] == np.array([-1, 0.5, 0.25], "<f4").tobytes()
    assert body[24:27] == bytes([0, 127, 255]) and body[27 + 24:54] == bytes([255, 0, 51])
    assert body[54:] == bytes([3]) + np.array([0, 1, 1], "<i4").tobytes()
    got = D.read_ply(path)
    assert got["comments"] == ["frame 3"] and got["triangles"].tolist() == [[0, 1, 1]]
    cloud = str(tmp_path / "cloud.ply")
    D.write_ply(cloud, v)
    assert open(cloud, "rb").read() == (b"ply\nformat binary_little_endian 1.0\nelement vertex 2\nproperty float x\nproperty float y\n"
                                        b"property float z\nend_header\n" + v.tobytes())


def quantisation_probes():
    """0, 1, 0.5, every k / 255 with its two fp32 neighbours, values below 0 and above 1."""
    k = (np.arange(256, dtype=np.float64) / 255).astype(np.float32)
    x = np.concatenate([[0.0, 1.0, 0.5, -0.0, -1e-8, -3.0, 1.0000001, 7.5, -np.inf, np.inf], k, np.nextafter(k, np.float32(-1)),
                        np.nextafter(k, np.float32(2))]).astype(np.float32)
    return np.resize(x, (-(-len(x) // 3) * 3,)).reshape(-1, 3)


def test_ply_colour_quantisation_is_to8b():
    c = quantisation_probes()
    body = D.ply_body(np.zeros_like(c), colors=c).reshape(-1, 15)
    assert np.array_equal(body[:, 12:], D.to8b(c))
    assert D.to8b(np.float32([0.0, 1.0, 0.5, -3.0, 7.5])).tolist() == [0, 255, 127, 0, 255]
    nan = D.ply_body(np.zeros((1, 3), np.float32), colors=np.array([[np.nan, 0.5, 1.0]], np.float32))
    assert nan[12:].tolist() == [0, 127, 255]


def test_read_ply_refuses_other_files(tmp_path):
    v, f, c, n = ply_inputs(3, 1)
    good = D.ply_header(3, 1, True, True) + D.ply_body(v, f, c, n).tobytes()

    def refuses(raw, match):
        p = str(tmp_path / "bad.ply")
        with open(p, "wb") as fh:
            fh.write(raw)
        with pytest.raises(ValueError, match=match):
            D.read_ply(p)

    refuses(good.replace(b"binary_little_endian", b"ascii"), "binary_little_endian")
    refuses(good.replace(b"binary_little_endian", b"binary_big_endian"), "binary_little_endian")
    refuses(good.replace(b"property float x", b"property double x"), "properties")
    refuses(good.replace(b"property uchar blue\n", b"property uchar blue\nproperty uchar alpha\n"), "properties")
    refuses(good.replace(b"property float nx\nproperty float ny\n", b"property float ny\nproperty float nx\n"), "properties")
    refuses(good.replace(b"uchar int vertex_indices", b"uchar uint vertex_indices"), "element face")
    refuses(good.replace(b"element face 1\n", b"element edge 1\n"), "element face")
    refuses(good[:-1], "bytes")
    refuses(good + b"\0", "bytes")
    refuses(b"PLY\n" + good[4:], "not a PLY")
    refuses(good.replace(b"end_header\n", b""), "not a PLY")
    quad = bytearray(good)
    quad[len(D.ply_header(3, 1, True, True)) + 3 * 27] = 4
    refuses(bytes(quad), "triangle")
    with pytest.raises(ValueError):
        D.ply_body(v, f, colors=c[:2])
    with pytest.raises(ValueError):
        D.ply_body(v, f.astype(np.float32))


# ---- the library's argument checks (no GPU: every call must fail before it launches) -------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from endosurf_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_new_entry_points_check_their_arguments(lib):
    assert lib.es_abi_version() == 14
    buf = np.zeros(256, np.float64)
    p = C.c_void_p(buf.ctypes.data // 16 * 16 + 16)          # (a host address: never dereferenced)
    odd = C.c_void_p(p.value + 4)

    def fails(status, word):
        assert status == 1 and word in lib.es_last_error(), (status, lib.es_last_error())

    fails(lib.es_mesh_clean_keys(None, 4, 2, p, p, None), b"tris")
    fails(lib.es_mesh_clean_keys(p, 4, 2, None, p, None), b"key_hi")
    fails(lib.es_mesh_clean_keys(p, 4, 2, p, None, None), b"key_lo")
    fails(lib.es_mesh_clean_keys(p, -4, 2, p, p, None), b"negative")
    fails(lib.es_mesh_clean_keys(p, 4, 1 << 31, p, p, None), b"2^31")
    fails(lib.es_mesh_clean_count(None, 4, 2, p, 1, p, p, None), b"tris")
    fails(lib.es_mesh_clean_count(p, 4, 2, None, 1, p, p, None), b"order")
    fails(lib.es_mesh_clean_count(p, 4, 2, p, 1, None, p, None), b"scratch")
    fails(lib.es_mesh_clean_count(p, 4, 2, p, 1, odd, p, None), b"aligned")
    fails(lib.es_mesh_clean_count(p, 4, 2, p, 1, p, None, None), b"totals")
    fails(lib.es_mesh_clean_count(p, 4, -2, p, 1, p, p, None), b"negative")
    assert lib.es_vn_scratch_bytes(10) > 0 and lib.es_vn_scratch_bytes(-1) == -1 and b"negative" in lib.es_last_error()
    assert lib.es_vn_scratch_bytes(1 << 31) == -1 and b"2^31" in lib.es_last_error()
    fails(lib.es_vn_count(None, 4, 2, p, p, None), b"tris")
    fails(lib.es_vn_count(p, 4, 2, None, p, None), b"corner_vertex")
    fails(lib.es_vn_count(p, 4, 2, p, None, None), b"scratch")
    fails(lib.es_vn_count(p, -4, 2, p, p, None), b"negative")
    fails(lib.es_vn_gather(None, p, 4, 2, p, p, p, None), b"verts")
    fails(lib.es_vn_gather(p, None, 4, 2, p, p, p, None), b"tris")
    fails(lib.es_vn_gather(p, p, 4, 2, None, p, p, None), b"order")
    fails(lib.es_vn_gather(p, p, 4, 2, p, None, p, None), b"scratch")
    fails(lib.es_vn_gather(p, p, 4, 2, p, p, None, None), b"normals")
    fails(lib.es_vn_gather(p, p, 4, -2, p, p, p, None), b"negative")
    assert lib.es_cluster_scratch_bytes(10) > 0 and lib.es_cluster_scratch_bytes(-1) == -1 and b"negative" in lib.es_last_error()
    fails(lib.es_cluster_keys(None, 4, 1.0, 0.0, 0.0, 0.0, p, None), b"verts")
    fails(lib.es_cluster_keys(p, 4, 1.0, 0.0, 0.0, 0.0, None, None), b"key")
    fails(lib.es_cluster_keys(p, -4, 1.0, 0.0, 0.0, 0.0, p, None), b"negative")
    for cell in (0.0, -1.0, float("nan"), float("inf")):
        fails(lib.es_cluster_keys(p, 4, cell, 0.0, 0.0, 0.0, p, None), b"cell")
    fails(lib.es_cluster_keys(p, 4, 1.0, float("nan"), 0.0, 0.0, p, None), b"origin")
    fails(lib.es_cluster_count(None, 4, p, p, None), b"sorted_key")
    fails(lib.es_cluster_count(p, 4, None, p, None), b"scratch")
    fails(lib.es_cluster_count(p, 4, p, None, None), b"totals")
    fails(lib.es_cluster_count(p, -4, p, p, None), b"negative")
    fails(lib.es_cluster_emit(p, p, 9, 4, p, p, 2, 0, p, p, p, None), b"8 attribute channels")
    fails(lib.es_cluster_emit(p, p, -1, 4, p, p, 2, 0, p, p, p, None), b"8 attribute channels")
    fails(lib.es_cluster_emit(p, p, 2, 4, p, p, 2, 1, p, p, p, None), b"2^20")
    fails(lib.es_cluster_emit(p, p, 2, 4, p, p, 5, 0, p, p, p, None), b"cell count")
    fails(lib.es_cluster_emit(p, p, 2, 4, p, p, 0, 0, p, p, p, None), b"cell count")
    fails(lib.es_cluster_emit(p, p, 2, -4, p, p, 2, 0, p, p, p, None), b"negative")
    fails(lib.es_cluster_emit(None, p, 2, 4, p, p, 2, 0, p, p, p, None), b"verts")
    fails(lib.es_cluster_emit(p, None, 2, 4, p, p, 2, 0, p, p, p, None), b"attrs")
    fails(lib.es_cluster_emit(p, p, 2, 4, None, p, 2, 0, p, p, p, None), b"order")
    fails(lib.es_cluster_emit(p, p, 2, 4, p, None, 2, 0, p, p, p, None), b"scratch")
    fails(lib.es_cluster_emit(p, p, 2, 4, p, p, 2, 0, None, p, p, None), b"verts_out")
    fails(lib.es_cluster_emit(p, p, 2, 4, p, p, 2, 0, p, None, p, None), b"attrs_out")
    fails(lib.es_cluster_emit(p, p, 2, 4, p, p, 2, 0, p, p, None, None), b"vertex_cluster")
    fails(lib.es_cluster_remap(None, 4, 2, p, p, None), b"tris")
    fails(lib.es_cluster_remap(p, 4, 2, None, p, None), b"vertex_cluster")
    fails(lib.es_cluster_remap(p, 4, 2, p, None, None), b"tris_out")
    fails(lib.es_cluster_remap(p, 4, -2, p, p, None), b"negative")
    assert lib.es_ply_body_bytes(3, 2, 1, 1) == 3 * 27 + 26 and lib.es_ply_body_bytes(3, 2, 0, 1) == 3 * 15 + 26
    assert lib.es_ply_body_bytes(3, 0, 1, 0) == 3 * 24 and lib.es_ply_body_bytes(1, 0, 0, 0) == 12
    assert lib.es_ply_body_bytes(-3, 2, 0, 0) == -1 and b"negative" in lib.es_last_error()
    fails(lib.es_ply_pack(None, p, p, p, 4, 2, p, None), b"verts")
    fails(lib.es_ply_pack(p, p, p, None, 4, 2, p, None), b"tris")
    fails(lib.es_ply_pack(p, p, p, p, 4, 2, None, None), b"out")
    fails(lib.es_ply_pack(p, p, p, p, -4, 2, p, None), b"negative")
    fails(lib.es_ply_pack(p, p, p, p, 4, 1 << 31, p, None), b"2^31")
    # nothing to do is no error, with or without pointers
    assert lib.es_mesh_clean_keys(None, 4, 0, None, None, None) == 0 and lib.es_vn_gather(None, None, 0, 0, None, None, None, None) == 0
    assert lib.es_cluster_remap(None, 4, 0, None, None, None) == 0 and lib.es_ply_pack(None, None, None, None, 0, 0, None, None) == 0
    assert lib.es_cluster_keys(None, 0, 1.0, 0.0, 0.0, 0.0, None, None) == 0
