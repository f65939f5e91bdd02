"""Mesh export on the device (csrc/export.hip and the clean-up of csrc/mesh.hip: Engine.mesh_clean / vertex_normals / cluster_vertices /
ply_pack, the ``clean`` and ``simplify`` keywords of EndoSurfRenderer.extract_observation_mesh, EndoSurfRenderer.export_observation_mesh)
against the numpy twins in endosurf_amd.meshing and endosurf_amd.data, which tests/test_mesh_export_host.py checks on written-out cases.
Everything is compared bit for bit."""
import os
import re

import numpy as np
import pytest
import torch

from endosurf_amd import data as D
from endosurf_amd import meshing as M
from mesh_util import fan, mt_mesh
from test_mesh_export_host import CLEAN_CASES, CLUSTER_F, CLUSTER_V, PLY_COMBOS, clean_case, ply_inputs, quantisation_probes

pytestmark = pytest.mark.gpu

SCAN_H = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "endosurf_amd", "csrc", "scan.h")).read()
SCAN_PER_THREAD = int(re.search(r"SCAN_PER_THREAD = (\d+);", SCAN_H).group(1))
assert re.search(r"SCAN_CHUNK = 256 \* SCAN_PER_THREAD;", SCAN_H)
SCAN_CHUNK = 256 * SCAN_PER_THREAD            # items of one workgroup of the scan
assert re.search(r"per = \(nchunk \+ 255\) / 256", SCAN_H)
SCAN_TWO_LEVEL = 256 * SCAN_CHUNK             # above this a thread of k_scan_blocks owns more than one chunk


@pytest.fixture(scope="module")
def eng():
    from endosurf_amd.engine import Engine
    return Engine("cuda")


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def same(t, a):
    a = np.asarray(a)
    return tuple(t.shape) == a.shape and np.array_equal(t.cpu().numpy(), a)


@pytest.fixture(scope="module")
def sphere():
    return mt_mesh("sphere", (24, 24, 24))


# ---- mesh_clean ------------------------------------------------------------------------------------------------------------------------
def check_clean(eng, v, f):
    """Both forms of Engine.mesh_clean equal the twin; twice the same bytes."""
    dv, df = dev(v), dev(f)
    for compact in (False, True):
        ev, ef, emap, est = M.mesh_clean(v, f, compact)
        for _ in range(2):
            kv, kf, kmap, kst = eng.mesh_clean(dv, df, compact)
            assert kv.dtype == torch.float32 and kf.dtype == torch.int32 and kmap.dtype == torch.int64
            assert same(kv, ev) and same(kf, ef) and same(kmap, emap) and kst == est, (compact, kst, est)
    return est


@pytest.mark.parametrize("name", list(CLEAN_CASES))
def test_clean_hand_made_meshes(eng, name):
    v, f, kept, n_deg, n_dup = clean_case(name)
    st = check_clean(eng, v, f)
    assert st == {"degenerate": n_deg, "duplicates": n_dup, "kept_triangles": len(kept)}
    kv, kf, _, _ = eng.mesh_clean(dev(v), dev(f, torch.int32))
    assert same(kf, f[kept])


def random_tris(T, ids, seed):
    rng = np.random.default_rng(seed)
    return np.asarray(ids, np.int64)[rng.integers(0, len(ids), size=(T, 3))]


def test_clean_duplicates_everywhere(eng):
    f = random_tris(4000, np.arange(50), 1)          # 4000 draws from 19 600 corner sets and 2 500 degenerate patterns
    st = check_clean(eng, np.random.default_rng(0).normal(size=(50, 3)).astype(np.float32), f)
    assert st["degenerate"] > 100 and st["duplicates"] > 200


def test_clean_indices_above_2_21(eng):
    """Keys must not fold vertex indices: the top indices differ from small ones only above bit 21."""
    V = (1 << 21) + 5
    ids = np.concatenate([np.arange(6), np.arange(1 << 21, V), np.arange((1 << 21) - 3, 1 << 21)])
    f = random_tris(4000, ids, 2)
    st = check_clean(eng, np.random.default_rng(1).normal(size=(V, 3)).astype(np.float32), f)
    assert st["duplicates"] > 300 and int(f.max()) == V - 1


@pytest.mark.parametrize("T", [SCAN_CHUNK - 1, SCAN_CHUNK, SCAN_CHUNK + 1, SCAN_TWO_LEVEL - 1, SCAN_TWO_LEVEL, SCAN_TWO_LEVEL + 1])
def test_clean_around_the_scan_boundaries(eng, T):
    V = 24 if T < 10000 else 150          # about a third of the triangles are duplicates of an earlier one
    f = random_tris(T, np.arange(V), T)
    st = check_clean(eng, np.zeros((V, 3), np.float32), f)
    assert st["duplicates"] > T // 8 and st["kept_triangles"] > 1000


# ---- vertex_normals --------------------------------------------------------------------------------------------------------------------
def check_normals(eng, v, f):
    """Contraction is off in the kernel: bit equality with meshing.vertex_normals; twice the same bytes."""
    want = M.vertex_normals(v, f)
    a, b = eng.vertex_normals(dev(v), dev(f)), eng.vertex_normals(dev(v), dev(f, torch.int32))
    assert a.dtype == torch.float32 and torch.equal(a, b)
    got = a.cpu().numpy()
    bad = np.nonzero((got != want).any(1))[0]
    assert got.shape == want.shape and len(bad) == 0, (len(bad), bad[:5], got[bad[:5]], want[bad[:5]])
    return got


def test_normals_of_a_sphere(eng, sphere):
    v, f = sphere
    assert len(f) > 2000
    n = check_normals(eng, v, f)
    centre = (np.array([24, 24, 24], np.float32) - 1) / 2
    out = (v - centre) / np.linalg.norm(v - centre, axis=1, keepdims=True)
    assert np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-6 and (np.einsum("ij,ij->i", n, out) > 0.8).all()


def test_normals_of_a_vertex_in_3000_triangles(eng):
    T = 3000
    ang = np.linspace(0, 2 * np.pi, T + 1, endpoint=False)
    rng = np.random.default_rng(4)
    rim = np.stack([np.cos(ang), np.sin(ang), 0.3 * rng.normal(size=T + 1)], 1)
    v = np.concatenate([[[0.1, -0.2, 1.0]], rim]).astype(np.float32)
    n = check_normals(eng, v, fan(T))
    assert n[0, 2] > 0.5
    check_normals(eng, v, fan(T)[rng.permutation(T)][:, [1, 2, 0]])          # the hub as another corner, the triangles shuffled


def test_normals_that_are_exactly_zero(eng):
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5], [2, 0, 0], [3, 0, 0], [4, 0, 0]], np.float32)
    f = np.array([[0, 1, 2], [4, 5, 6], [4, 4, 5]])          # 3 is isolated; 4, 5, 6 lie on a line
    n = check_normals(eng, v, f)
    assert (n[3:] == 0).all() and n[:3].tolist() == [[0, 0, 1]] * 3
    e = eng.vertex_normals(torch.zeros(4, 3, device="cuda"), torch.zeros(0, 3, dtype=torch.int64, device="cuda"))
    assert e.shape == (4, 3) and bool((e == 0).all())
    assert eng.vertex_normals(torch.zeros(0, 3, device="cuda"), torch.zeros(0, 3, dtype=torch.int64, device="cuda")).shape == (0, 3)


# ---- cluster_vertices -------------------------------------------------------------------------------------------------------------------
def check_cluster(eng, v, f, cell, origin=(0.0, 0.0, 0.0), att=None):
    want = M.cluster_vertices(v, f, cell, origin, att)
    datt = None if att is None else dev(att)
    for _ in range(2):
        got = eng.cluster_vertices(dev(v), dev(f), cell, origin, datt)
        assert got[0].dtype == torch.float32 and got[1].dtype == torch.int32 and got[3].dtype == torch.int32
        assert same(got[0], want[0]) and same(got[1], want[1]) and same(got[3], want[3]) and got[4] == want[4], (got[4], want[4])
        assert (got[2] is None and want[2] is None) or same(got[2], want[2])
    return want[4]


@pytest.mark.parametrize("cells", [1.0, 2.5, 100.0])
@pytest.mark.parametrize("channels", [0, 1, 8])
def test_cluster_a_sphere(eng, sphere, cells, channels):
    v, f = sphere
    att = None if channels == 0 else np.random.default_rng(channels).normal(size=(len(v), channels)).astype(np.float32)
    st = check_cluster(eng, v, f, cells, att=att)          # (index coordinates: one unit is one grid cell)
    assert st["cells"] == 1 if cells == 100.0 else 1 < st["cells"] < len(v)
    assert st["kept_triangles"] < len(f) and st["degenerate"] > 0
    check_cluster(eng, v - 11.3, f, cells, origin=(-0.25, 0.5, 0.125), att=att)          # negative coordinates, an origin


def test_cluster_5000_vertices_in_one_cell(eng):
    rng = np.random.default_rng(8)
    v = np.concatenate([rng.uniform(0.01, 0.99, size=(5000, 3)), rng.uniform(-3, 3, size=(300, 3))]).astype(np.float32)
    v = v[rng.permutation(len(v))]
    f = rng.integers(0, len(v), size=(2000, 3))
    st = check_cluster(eng, v, f, 1.0, att=rng.normal(size=(len(v), 3)).astype(np.float32))
    assert st["largest_cell"] >= 5000


def test_cluster_hand_made_renumber_and_collapse(eng):
    att = np.arange(12, dtype=np.float32).reshape(6, 2)
    st = check_cluster(eng, CLUSTER_V, CLUSTER_F, 1.0, att=att)
    assert st == {"cells": 4, "largest_cell": 2, "degenerate": 1, "duplicates": 2, "kept_triangles": 2}
    check_cluster(eng, CLUSTER_V, CLUSTER_F, 1.0, origin=(0.5, 0.0, 0.0))
    rng = np.random.default_rng(3)
    v = rng.uniform(-1, 1, size=(40, 3)).astype(np.float32)
    f = rng.integers(0, 40, size=(60, 3))
    assert check_cluster(eng, v, f, 1e-5)["cells"] == 40                                          # renumbers only
    st = check_cluster(eng, v, f, 100.0, origin=(-50.0, -50.0, -50.0))                          # one vertex, no triangle
    assert st["cells"] == 1 and st["kept_triangles"] == 0
    e = eng.cluster_vertices(torch.zeros(0, 3, device="cuda"), torch.zeros(0, 3, dtype=torch.int64, device="cuda"), 1.0)
    assert e[0].shape == (0, 3) and e[1].shape == (0, 3) and e[3].shape == (0,) and e[4]["cells"] == 0


def test_cluster_argument_errors(eng):
    from endosurf_amd._lib import EndoSurfHipError
    f = torch.zeros(0, 3, dtype=torch.int64, device="cuda")
    half = float(1 << 20)
    ok = torch.tensor([[-half * 0.5, 0, 0], [half * 0.5 - 0.25, 0, 0]], device="cuda")
    assert eng.cluster_vertices(ok, f, 0.5)[4]["cells"] == 2
    for bad in ([half * 0.5, 0, 0], [0, 0, 1e9], [float("nan"), 0, 0]):
        with pytest.raises(EndoSurfHipError, match="2\\^20"):
            eng.cluster_vertices(torch.tensor([bad], device="cuda"), f, 0.5)
    with pytest.raises(EndoSurfHipError, match="cell"):
        eng.cluster_vertices(ok, f, 0.0)
    with pytest.raises(EndoSurfHipError, match="attributes"):
        eng.cluster_vertices(ok, f, 1.0, attributes=torch.zeros(2, 9, device="cuda"))
    with pytest.raises(EndoSurfHipError, match="outside"):
        eng.mesh_clean(ok, torch.tensor([[0, 1, 2]], device="cuda"))


# ---- ply_pack ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,T", [(1, 0), (7, 5), (255, 255), (33, 256), (301, 257), (256, 1)])
@pytest.mark.parametrize("with_colors,with_normals", PLY_COMBOS)
def test_ply_pack_equals_the_numpy_packer(eng, V, T, with_colors, with_normals):
    v, f, c, n = ply_inputs(V, T, seed=V + T)
    if with_colors:
        c[:min(V, 4)] = quantisation_probes()[:min(V, 4)]
    for faces in (True, False):
        want = D.ply_body(v, f if faces else None, c if with_colors else None, n if with_normals else None)
        args = (dev(v), dev(f) if faces else None, dev(c) if with_colors else None, dev(n) if with_normals else None)
        a, b = eng.ply_pack(*args), eng.ply_pack(*args)
        assert a.dtype == torch.uint8 and torch.equal(a, b) and same(a, want)


def test_ply_colours_and_files_from_device_tensors(eng, tmp_path):
    c = quantisation_probes()
    body = eng.ply_pack(torch.zeros(len(c), 3, device="cuda"), colors=dev(c)).cpu().numpy().reshape(-1, 15)
    assert np.array_equal(body[:, 12:], D.to8b(c))
    v, f, col, n = ply_inputs(33, 21, seed=5)
    a, b = str(tmp_path / "dev.ply"), str(tmp_path / "host.ply")
    D.write_ply(a, dev(v), dev(f), colors=dev(col), normals=n, comment="x", engine=eng)          # (a host array among device tensors)
    D.write_ply(b, v, f, colors=col, normals=n, comment="x")
    assert open(a, "rb").read() == open(b, "rb").read()
    got = D.read_ply(a)
    assert np.array_equal(got["vertices"], v) and np.array_equal(got["triangles"], f) and np.array_equal(got["colors"], D.to8b(col))


# ---- through the renderer ----------------------------------------------------------------------------------------------------------------
BMIN, BMAX, VIEW, R = [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0], [0.1, -0.2, -1.5], 32


@pytest.fixture(scope="module")
def scene():
    from gpu_util import renderer_for
    return renderer_for(5, "trained", True), torch.tensor([0.37])


@pytest.fixture(scope="module")
def plain(scene):
    r, t = scene
    m = r.extract_observation_mesh(t, BMIN, BMAX, R, view_point=VIEW)
    assert m["triangles"].shape[0] > 200          # the level set is there: the tests below are about something
    return m


def test_default_arguments_change_nothing(scene, plain):
    r, t = scene
    assert set(plain) == {"vertices", "triangles", "normals", "sdf", "colors"}
    again = r.extract_observation_mesh(t, BMIN, BMAX, R, view_point=VIEW, clean=False, simplify=None)
    assert set(again) == set(plain) and all(torch.equal(again[k], plain[k]) for k in plain)
    v, f = r._mesh_on_device(t, BMIN, BMAX, R, 0.0, 1 << 22)
    assert torch.equal(plain["vertices"], v) and torch.equal(plain["triangles"], f)


def test_clean_removes_what_the_twin_removes(scene, plain):
    r, t = scene
    m = r.extract_observation_mesh(t, BMIN, BMAX, R, view_point=VIEW, clean=True)
    ev, ef, emap, est = M.mesh_clean(plain["vertices"].cpu().numpy(), plain["triangles"].cpu().numpy(), compact=True)
    assert set(m) == set(plain) | {"clean"} and m["clean"] == est
    assert same(m["vertices"], ev) and same(m["triangles"], ef)
    dup = torch.cat([plain["triangles"], plain["triangles"][:50].flip(1), plain["triangles"][:7, [0, 0, 1]]])
    kv, kf, _, st = r.engine.mesh_clean(plain["vertices"], dup)
    assert st == {"degenerate": 7 + est["degenerate"], "duplicates": 50 + est["duplicates"], "kept_triangles": est["kept_triangles"]}


def test_simplify_grid(scene, plain):
    r, t = scene
    m = r.extract_observation_mesh(t, BMIN, BMAX, R, view_point=VIEW, simplify="grid")
    assert set(m) == set(plain) | {"simplify"}
    f = m["triangles"].cpu().numpy()
    assert 0 < len(f) < plain["triangles"].shape[0] and m["simplify"]["kept_triangles"] == len(f)
    assert m["simplify"]["cells"] == m["vertices"].shape[0] < plain["vertices"].shape[0]
    assert ((f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])).all()
    assert len(np.unique(np.sort(f, axis=1), axis=0)) == len(f)
    assert m["normals"].shape == m["vertices"].shape == m["colors"].shape and m["sdf"].shape == (m["vertices"].shape[0],)
    ev, ef, _, _, est = M.cluster_vertices(plain["vertices"].cpu().numpy(), plain["triangles"].cpu().numpy(), 2.0 / (R - 1), origin=BMIN)
    assert same(m["vertices"], ev) and same(m["triangles"], ef) and m["simplify"] == est
    c = r.extract_observation_mesh(t, BMIN, BMAX, R, simplify=0.25)
    assert 0 < c["triangles"].shape[0] < len(f)
    with pytest.raises(ValueError):
        r.extract_observation_mesh(t, BMIN, BMAX, R, simplify="coarse")


def test_export_writes_the_three_files(scene, tmp_path):
    r, t = scene
    m = r.export_observation_mesh(str(tmp_path / "007"), t, BMIN, BMAX, R, view_point=VIEW)
    assert sorted(os.path.basename(p) for p in m["paths"].values()) == ["007_color.ply", "007_geometry.ply", "007_normal.ply"]
    g, c, n = (D.read_ply(m["paths"][k]) for k in ("geometry", "color", "normal"))
    assert set(g) == {"vertices", "triangles"} and set(c) == set(n) == {"vertices", "triangles", "colors"}
    v, f = m["vertices"].cpu().numpy(), m["triangles"].cpu().numpy()
    assert len(f) > 200 and m["clean"]["kept_triangles"] == len(f)
    for x in (g, c, n):
        assert np.array_equal(x["vertices"], v) and np.array_equal(x["triangles"], f)
    assert np.array_equal(c["colors"], D.to8b(m["colors"]))
    vn = r.engine.vertex_normals(m["vertices"], m["triangles"])
    assert torch.equal(vn, m["vertex_normals"]) and np.array_equal(vn.cpu().numpy(), M.vertex_normals(v, f))
    assert np.array_equal(n["colors"], D.to8b((-vn * 0.5 + 0.5).clip(0, 1)))
    s = r.export_observation_mesh(str(tmp_path / "008"), t, BMIN, BMAX, R, simplify="grid", components=None)
    assert D.read_ply(s["paths"]["geometry"])["triangles"].shape[0] == s["simplify"]["kept_triangles"] < len(f)
    assert (D.read_ply(s["paths"]["color"])["colors"] == 255).all()          # no view point: white
