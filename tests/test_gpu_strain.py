"""GPU: tissue strain along surface tracks.  Kernel level through the C ABI -- es_deform_jacobian (csrc/deform_jet.hip)
against the fp64 oracle's closed-form Jacobian on rows screened away from the ReLU kinks, es_strain_rows (csrc/strain.hip) against the
fp64 numpy twin ``strain.strain_rows`` -- then Engine and renderer.  Every test prints the figures it asserts on."""
import ctypes as C

import numpy as np
import pytest
import torch

import weightgen
from gpu_util import renderer_for
from oracle import endosurf_oracle as O
from shapes_util import FORWARD_GATE, RELU_MARGIN, inputs, relu_margin
from track_util import assert_contraction, deform_fn, draw, oracle_net

from endosurf_amd import strain, tracking

pytestmark = pytest.mark.gpu

CASES = [(11, "trained"), (23, "trained"), (21, "init")]
M = 200
HALF_MAX_POINTS = 4096          # 8-point tiles up to here, 16-point tiles above (csrc/deform_jet.hip)
RTOL, ATOL = 2.4e-7, 1e-13      # two fp32 ulps: the kernel's fp64 error is far below half an ulp, only the final rounding can differ
KEYS = ("F", "det", "stretch", "area", "surface_stretch", "valid")


class Dev:
    """Weights of one state on the device and the two strain entries on them, inputs and results as host tensors."""
    def __init__(self, state):
        from endosurf_amd import _lib, params
        self._lib, self.lib = _lib, _lib.load()
        _lib.check(self.lib.es_init(), "es_init")
        flat = torch.from_numpy(params.flatten_state(state)).cuda()
        self.weff = torch.zeros(self.lib.es_weff_floats(), device="cuda")
        self.packed = torch.zeros(self.lib.es_packed_floats(), device="cuda")
        _lib.check(self.lib.es_weightnorm_pack(_lib.ptr(flat), _lib.ptr(self.weff), _lib.ptr(self.packed), 1, _lib.stream_ptr()))
        torch.cuda.synchronize()

    def jacobian(self, x, t, want_jac=True, want_xc=True):
        """(J [M,3,3], x + D [M,3]) at fp32 host points; ``t`` [M] or [1] (read as t_scalar).  Unwritten entries would stay NaN."""
        n, ptr = x.shape[0], self._lib.ptr
        jac = torch.full((n, 3, 3), float("nan"), device="cuda") if want_jac else None
        xc = torch.full((n, 3), float("nan"), device="cuda") if want_xc else None
        p = self._lib.es_points()
        xd, td = x.cuda().contiguous(), t.reshape(-1).cuda().contiguous()
        assert td.numel() in (1, n)
        p.x, p.t, p.mode, p.n_per_ray, p.ldz, p.M = ptr(xd), ptr(td), 0, 1, 1, n
        p.t_scalar = 1 if td.numel() == 1 and n != 1 else 0
        self._lib.check(self.lib.es_deform_jacobian(C.byref(p), ptr(self.packed), ptr(self.weff), ptr(jac), ptr(xc), self._lib.stream_ptr()),
                        "es_deform_jacobian")
        torch.cuda.synchronize()
        return (None if jac is None else jac.cpu()), (None if xc is None else xc.cpu())


def strain_dev(jac_from, jac_to, normals):
    """es_strain_rows on fp32 host rows: ``strain.strain_rows``' dict as host tensors (NaN / True where the kernel did not write)."""
    from endosurf_amd import _lib
    lib, ptr = _lib.load(), _lib.ptr
    n = jac_to.shape[0]
    dev = lambda a: None if a is None else a.float().cuda().contiguous()
    ja, jb, nn = dev(jac_from), dev(jac_to), dev(normals)
    out = {"F": (n, 3, 3), "det": (n,), "stretch": (n, 3)}
    if normals is not None:
        out.update(area=(n,), surface_stretch=(n, 2))
    out = {k: torch.full(s, float("nan"), device="cuda") for k, s in out.items()}
    out["valid"] = torch.ones(n, dtype=torch.bool, device="cuda")
    _lib.check(lib.es_strain_rows(ptr(ja), ptr(jb), ptr(nn), n, ptr(out["F"]), ptr(out["det"]), ptr(out["stretch"]), ptr(out.get("area")),
                                  ptr(out.get("surface_stretch")), ptr(out["valid"]), _lib.stream_ptr()), "es_strain_rows")
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def deform_margin(net, x, t):
    """Smallest |pre-activation| over the ReLU layers of the deformation network, per point: the loop of ``shapes_util.relu_margin``
    on that network alone."""
    with torch.no_grad():
        e = torch.cat([O.freq_encode(x, 6), O.freq_encode(t[:, None], 6)], -1)
        u, margin = e, torch.full((x.shape[0],), float("inf"), dtype=x.dtype)
        for l in range(8):
            W, b = net._wb("deform_network", l)
            if l == 4:
                u = torch.cat([u, e], -1) / O.SQRT2
            a = u @ W.t() + b
            margin = torch.minimum(margin, a.abs().min(-1)[0])
            u = torch.relu(a)
    return margin


def screened(net, n, seed):
    """(x [n,3], t [n]) of ``shapes_util.inputs`` -- drawn like test_point_backward's and screened for that module's weights --
    redrawn until every row also keeps RELU_MARGIN from every kink of THIS case's weights (``net``, fp64)."""
    x, d, t, _, _, _ = inputs(n, seed)
    rng = np.random.default_rng(1000 + seed)
    for _ in range(64):
        near = torch.nonzero(relu_margin(net, x.double(), d.double(), t.double()[:, None]) < RELU_MARGIN).reshape(-1)
        if near.numel() == 0:
            return x, t
        x[near] = torch.from_numpy(rng.uniform(-0.7, 0.7, size=(near.numel(), 3)).astype(np.float32))
        t[near] = torch.from_numpy(rng.uniform(size=(near.numel(),)).astype(np.float32))
    raise AssertionError("could not place the points away from the ReLU kinks")


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"{c[1]}{c[0]}")
def case(request):
    """One state: device weights, the fp64 oracle, 200 screened rows, the oracle's J and x + D on them and the device's own (computed
    once, shared, never written to)."""
    seed, mode = request.param
    state = weightgen.make_state(seed, mode, True)
    dev, net64 = Dev(state), oracle_net(state, torch.float64)
    x, t = screened(net64, M, seed)
    with torch.no_grad():
        d64, J64 = net64.deform(x.double(), t.double())
    J, xc = dev.jacobian(x, t)
    return dict(seed=seed, mode=mode, dev=dev, net64=net64, x=x, t=t, J64=J64, xc64=x.double() + d64, J=J, xc=xc, name=f"{mode}{seed}")


def test_jacobian_against_the_fp64_oracle(case):
    """Every entry of J within FORWARD_GATE["v"] (3e-6) and x + D within FORWARD_GATE["xc"] (1e-6) of the fp64 oracle, at the sizes around
    the edges of the 8-point tile, and on the 16-point tiles of the first batch that selects them (the 200 rows repeated to 4 097) and
    of that batch + 17 rows.  (The oracle's own fp32 run is within 4.9e-7 of its fp64 run on such rows.)"""
    dev, x, t, J64, xc64 = case["dev"], case["x"], case["t"], case["J64"], case["xc64"]
    for m in (1, 7, 8, 9, 15, 16, 17, 33, 200):
        J, xc = dev.jacobian(x[:m], t[:m])
        e_j, e_xc = float((J.double() - J64[:m]).abs().max()), float((xc.double() - xc64[:m]).abs().max())
        print(f"[{case['name']}] M {m:4d}: J {e_j:.3e} (gate {FORWARD_GATE['v']:.0e})  x+D {e_xc:.3e} (gate {FORWARD_GATE['xc']:.0e})")
        assert e_j <= FORWARD_GATE["v"] and e_xc <= FORWARD_GATE["xc"], (m, e_j, e_xc)
    for n in (HALF_MAX_POINTS + 1, HALF_MAX_POINTS + 18):
        idx = torch.arange(n) % M
        J, xc = dev.jacobian(x[idx], t[idx])
        e_j, e_xc = float((J.double() - J64[idx]).abs().max()), float((xc.double() - xc64[idx]).abs().max())
        print(f"[{case['name']}] M {n:4d}: J {e_j:.3e}  x+D {e_xc:.3e}  (16-point tiles)")
        assert e_j <= FORWARD_GATE["v"] and e_xc <= FORWARD_GATE["xc"], (n, e_j, e_xc)
    # either output alone is the same as in the pair
    assert torch.equal(dev.jacobian(x, t, want_xc=False)[0], case["J"]) and torch.equal(dev.jacobian(x, t, want_jac=False)[1], case["xc"])


def test_rows_do_not_depend_on_their_place_or_neighbours(case):
    """The same rows again, permuted, in a smaller batch and alone: the same bits.  So are the two tile heights: the 200 rows repeated
    to 4 096 (the last batch of the 8-point tiles, 512 of them) and to 4 097 and 4 114 rows (16-point tiles, the last tile one and two
    rows long) come out as in the 200-row batch, so the oracle parity shown on one height holds on the other."""
    dev, x, t, full = case["dev"], case["x"], case["t"], (case["J"], case["xc"])
    perm = torch.from_numpy(np.random.default_rng(3).permutation(M).copy())
    for a, again, shuffled, first, alone in zip(full, dev.jacobian(x, t), dev.jacobian(x[perm], t[perm]), dev.jacobian(x[:21], t[:21]),
                                                dev.jacobian(x[117:118], t[117:118])):
        assert bool(torch.isfinite(a).all())
        assert torch.equal(a, again) and torch.equal(a[perm], shuffled) and torch.equal(a[:21], first) and torch.equal(a[117:118], alone)
    for n in (HALF_MAX_POINTS, HALF_MAX_POINTS + 1, HALF_MAX_POINTS + 18):
        idx = torch.arange(n) % M
        for a, b in zip(full, dev.jacobian(x[idx], t[idx])):
            assert torch.equal(a[idx], b), n


def test_a_shared_time_equals_a_time_per_row(case):
    dev, x, t = case["dev"], case["x"], case["t"]
    shared = dev.jacobian(x, t[:1])                                  # read as t_scalar
    per_row = dev.jacobian(x, t[:1].expand(M).contiguous())
    assert torch.equal(shared[0], per_row[0]) and torch.equal(shared[1], per_row[1])
    assert torch.equal(shared[0][:1], case["J"][:1]) and not torch.equal(shared[0][1:], case["J"][1:])          # (the time is read)


def test_jacobian_against_the_three_launch_path(case):
    """``renderer.deform_jacobian`` and ``model.get_deform_grad_from_observed_space`` (three launches of the point forward, one per unit
    direction) on the same screened rows: each within the gate of the oracle, at most 6e-6 apart -- 0.0 is expected, the kernel
    restates that chain's scheme operand for operand.  Measured on an MI355X: 0.0 on all three cases."""
    r = renderer_for(case["seed"], case["mode"], True)
    xd, td = case["x"].cuda(), case["t"].cuda()
    new = r.deform_jacobian(xd, td)
    old = r.model.get_deform_grad_from_observed_space(xd, td)
    assert new.shape == old.shape == (M, 3, 3) and new.is_cuda
    e_new, e_old = (float((a.cpu().double() - case["J64"]).abs().max()) for a in (new, old))
    diff = float((new - old).abs().max())
    print(f"\n[{case['name']}] one launch against the oracle {e_new:.3e}, three launches {e_old:.3e}, one against three {diff:.3e}")
    assert e_new <= FORWARD_GATE["v"] and e_old <= FORWARD_GATE["v"]
    assert diff <= 6e-6
    assert torch.equal(new.cpu(), case["J"])          # the renderer's weights and call give the C ABI's bits


def hand_rows():
    """(jac_from, jac_to, normals, valid) fp32: the identity, diag(2, 1, 0.5) seen along z and along x, a rotation, I + 1e-9 G (the
    coincident stretches; its diagonal rounds to 1 in fp32, the rest stays), a negative determinant on either side, a NaN entry on
    either side, a zero normal, a NaN normal."""
    eye = np.eye(3)
    q, _ = np.linalg.qr(np.random.default_rng(6).normal(size=(3, 3)))
    q = q * np.sign(np.linalg.det(q))
    near = eye + 1e-9 * np.random.default_rng(4).normal(size=(3, 3))
    flip, nan = np.diag([-1.0, 1.0, 1.0]), eye.copy()
    nan[1, 2] = np.nan
    d = np.diag([2.0, 1.0, 0.5])
    rows = [(eye, eye, [0, 0, 1], True), (d, eye, [0, 0, 1], True), (d, eye, [1, 0, 0], True), (q, eye, [0.3, -0.5, 0.8], True),
            (near, eye, [0.2, 0.9, -0.4], True), (eye, near, [1, 1, 1], True), (flip, eye, [0, 0, 1], False), (eye, flip, [0, 0, 1], False),
            (nan, eye, [0, 0, 1], False), (eye, nan, [0, 0, 1], False), (d, eye, [0, 0, 0], False), (d, eye, [0, np.nan, 1], False)]
    ja, jb, n, v = zip(*rows)
    f = lambda a: torch.from_numpy(np.asarray(a, np.float64)).float()
    return f(ja), f(jb), f(n), torch.tensor(v)


def close(got, want):
    if got.dtype == torch.bool:
        return torch.equal(got, want)
    return bool(((got.double() - want.double()).abs() <= ATOL + RTOL * want.double().abs()).all())


@pytest.fixture(scope="module")
def strain_inputs():
    """The device's own J of the seed-11 weights at 257 points of ``track_util.draw`` at t_from and at t_to, copied to the host, and
    normals of any length."""
    dev = Dev(weightgen.make_state(11, "trained", True))
    x, t_from, t_to = draw(11, 257)
    ja, jb = dev.jacobian(x, t_from, want_xc=False)[0], dev.jacobian(x, t_to, want_xc=False)[0]
    n = torch.from_numpy(np.random.default_rng(9).normal(size=(257, 3)) * 3.0).float()
    return ja, jb, n


@pytest.mark.parametrize("m", [0, 1, 63, 64, 65, 257])
def test_strain_rows_against_the_numpy_twin(strain_inputs, m):
    ja, jb, n = (a[:m] for a in strain_inputs)
    got, want = strain_dev(ja, jb, n), strain.strain_rows(ja, jb, n)
    assert set(got) == set(want) == set(KEYS)
    for k in KEYS:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype and close(got[k], want[k]), (k, m)
    assert bool(want["valid"].all())
    if m:
        worst = max(float(((got[k].double() - want[k].double()).abs() / want[k].double().abs().clamp_min(1e-30)).max()) for k in ("det", "stretch", "area", "surface_stretch"))
        print(f"\nM {m}: largest relative difference to the twin {worst:.3e} (two ulps: {RTOL:.1e}); stretches {float(want['stretch'].min()):.3f} .. "
              f"{float(want['stretch'].max()):.3f}")
    again = strain_dev(ja, jb, n)
    assert all(torch.equal(got[k], again[k]) for k in KEYS)          # bit-identical from call to call
    # without normals: the same F, det, stretch and (here) valid, and no surface outputs
    bare = strain_dev(ja, jb, None)
    assert set(bare) == {"F", "det", "stretch", "valid"} and all(torch.equal(bare[k], got[k]) for k in bare)
    # jac_from null is the identity
    eye = torch.eye(3)[None].expand(m, 3, 3).contiguous()
    canon, given = strain_dev(None, jb, n), strain_dev(eye, jb, n)
    assert all(torch.equal(canon[k], given[k]) for k in KEYS)
    assert all(close(canon[k], v) for k, v in strain.strain_rows(None, jb, n).items())


def test_strain_rows_on_hand_made_rows(strain_inputs):
    ja, jb, n, valid = hand_rows()
    # behind 64 ordinary rows, so that the block holds both kinds
    ja, jb, n = (torch.cat([a[:64], b]) for a, b in zip(strain_inputs, (ja, jb, n)))
    valid = torch.cat([torch.ones(64, dtype=torch.bool), valid])
    got, want = strain_dev(ja, jb, n), strain.strain_rows(ja, jb, n)
    assert torch.equal(got["valid"], valid) and torch.equal(want["valid"], valid)
    for k in KEYS:
        assert bool(torch.isfinite(got[k].double()).all()), k
        assert close(got[k], want[k]), k
        assert not bool(got[k][~valid].double().abs().sum()), k          # zeros in every output of a row that is not valid
    h = {k: v[64:] for k, v in got.items()}
    assert torch.equal(h["stretch"][0], torch.ones(3)) and torch.equal(h["surface_stretch"][0], torch.ones(2)) and float(h["area"][0]) == 1.0
    assert h["stretch"][1].tolist() == [2.0, 1.0, 0.5] and float(h["area"][1]) == 2.0 and h["surface_stretch"][1].tolist() == [2.0, 1.0]
    assert float(h["area"][2]) == 0.5 and h["surface_stretch"][2].tolist() == [1.0, 0.5] and float(h["det"][2]) == 1.0
    assert float((h["stretch"][3] - 1).abs().max()) <= RTOL and float((h["surface_stretch"][3] - 1).abs().max()) <= RTOL          # the rotation (fp32 entries)
    assert float((h["stretch"][4:6] - 1).abs().max()) <= RTOL          # coincident stretches: no sqrt(eps) = 1.5e-8 ... 1e-4 loss
    # without normals the last two rows are valid again
    bare = strain_dev(ja, jb, None)
    assert torch.equal(bare["valid"][64:], torch.cat([valid[64:-2], torch.ones(2, dtype=torch.bool)]))


@pytest.fixture(scope="module")
def R():
    return renderer_for(11, "trained", True)


def test_track_strain_end_to_end_on_the_oracles_tracks(R):
    """500 rows tracked in fp64 on the host, the positions rounded to fp32 and both ends handed to ``renderer.track_strain`` and to the
    fp64 twin over the fp64 oracle at the same fp32 points.  On the rows that keep 1e-5 from every kink of the deformation network at
    both ends (at least 60 % of them; a row nearer may take the other branch in fp32, which says nothing about the kernels) the
    stretches agree within 4 x the worst-row error of the oracle's own fp32 run on the same rows -- the two fp32 evaluations differ
    in the summation order of 256-term dot products only."""
    state = weightgen.make_state(11, "trained", True)
    net64, net32 = oracle_net(state, torch.float64), oracle_net(state, torch.float32)
    x, t_from, t_to = draw(11, 500)
    assert_contraction(net64, x, t_from, t_to)
    ref = tracking.warp_points(deform_fn(net64), x.double(), t_from.double(), t_to.double(), max_iters=300, tol=1e-13)
    assert bool(ref["converged"].all())
    y = ref["points"].float()

    def jac(net):
        def fn(p, t):
            with torch.no_grad():
                return net.deform(p, t)[1]
        return fn
    n = torch.from_numpy(np.random.default_rng(2).normal(size=(500, 3))).float()
    want = strain.track_strain(jac(net64), x.double(), t_from.double(), y.double(), t_to.double(), n.double())
    o32 = strain.track_strain(jac(net32), x, t_from, y, t_to, n)
    got = R.track_strain(x, t_from, y, t_to, n)
    assert all(got[k].is_cuda for k in KEYS) and got["F"].shape == (500, 3, 3) and got["stretch"].shape == (500, 3)
    keep = (deform_margin(net64, x.double(), t_from.double()) >= 1e-5) & (deform_margin(net64, y.double(), t_to.double()) >= 1e-5)
    assert bool(want["valid"].all()) and bool(got["valid"].all())
    for k in ("stretch", "surface_stretch"):
        yard = float((o32[k].double() - want[k])[keep].abs().max())
        err = float((got[k].cpu().double() - want[k])[keep].abs().max())
        print(f"\n{k}: kept {int(keep.sum())} of 500 rows; device {err:.3e}, fp32 oracle {yard:.3e} (bound {4 * yard:.3e})")
        assert int(keep.sum()) >= 300
        assert err <= 4 * yard, (k, err, yard)
    # relative to the canonical shape: F = J(y, t_to)^-1
    can = R.track_strain(None, None, y, t_to)
    want_c = strain.track_strain(jac(net64), None, None, y.double(), t_to.double())
    yard = float((strain.track_strain(jac(net32), None, None, y, t_to)["stretch"].double() - want_c["stretch"])[keep].abs().max())
    assert set(can) == {"F", "det", "stretch", "valid"}
    assert float((can["stretch"].cpu().double() - want_c["stretch"])[keep].abs().max()) <= 4 * yard


def _patch(n=17):
    """A planar n x n vertex patch (tilted, 0.02 between vertices) and its 2 (n-1)^2 triangles."""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    v = (np.array([-0.2, -0.25, 0.1])[None] + i.reshape(-1, 1) * np.array([0.02, 0.004, -0.006])[None]
         + j.reshape(-1, 1) * np.array([-0.002, 0.018, 0.008])[None])
    q = (i[:-1, :-1] * n + j[:-1, :-1]).reshape(-1)
    tris = np.concatenate([np.stack([q, q + n, q + n + 1], 1), np.stack([q, q + n + 1, q + 1], 1)])
    return torch.from_numpy(v.astype(np.float32)), torch.from_numpy(tris.astype(np.int32))


def test_mesh_strain_is_the_composition_of_its_two_launches(R):
    verts, tris = _patch()
    assert verts.shape == (289, 3) and tris.shape == (512, 3)
    times = [0.3, 0.31, 0.9]
    track = R.track_mesh(verts.cuda(), tris.cuda(), t=0.3, times=times)
    assert bool(track["converged"].all())
    out = R.mesh_strain(track, times)
    shapes = {"F": (3, 289, 3, 3), "det": (3, 289), "stretch": (3, 289, 3), "area": (3, 289), "surface_stretch": (3, 289, 2), "valid": (3, 289)}
    assert {k: tuple(v.shape) for k, v in out.items()} == shapes and all(v.is_cuda for v in out.values())
    assert bool(out["valid"].all())
    # the composition, spelled out: one Jacobian launch with a time per row, the normals of the reference frame, one strain launch
    tt = torch.tensor(times, device="cuda").repeat_interleave(289)
    J = R.deform_jacobian(track["vertices"].reshape(-1, 3), tt).reshape(3, 289, 3, 3)
    normals = R.engine.vertex_normals(track["vertices"][0].contiguous(), tris.cuda())
    rows = R.engine.strain_rows(J[0][None].expand(3, 289, 3, 3).reshape(-1, 3, 3), J.reshape(-1, 3, 3), normals[None].expand(3, 289, 3).reshape(-1, 3))
    for k in KEYS:
        assert torch.equal(out[k].reshape(rows[k].shape), rows[k]), k
    # the reference frame against itself
    for k in ("det", "stretch", "area", "surface_stretch"):
        assert float((out[k][0] - 1).abs().max()) <= RTOL, k
    print(f"\nframe 2 against frame 0: area ratio {float(out['area'][2].min()):.4f} .. {float(out['area'][2].max()):.4f}, "
          f"stretches {float(out['stretch'][2].min()):.4f} .. {float(out['stretch'][2].max()):.4f}")
    assert float((out["stretch"][2] - 1).abs().max()) > 1e-3          # (the tissue does deform between 0.3 and 0.9)
    # against the twin over the same J: the default normals are the twin's, bit for bit (meshing.vertex_normals)
    twin = strain.mesh_strain(lambda p, t: R.deform_jacobian(p, t).cpu(), {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in track.items()},
                              torch.tensor(times))
    assert all(close(out[k].cpu(), twin[k]) for k in KEYS)
    # host tensors, numpy arrays and lists give the device tensors' result
    host = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in track.items()}
    as_np = {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in host.items()}
    for tr, tm in ((host, torch.tensor(times)), (as_np, np.asarray(times, np.float32))):
        o = R.mesh_strain(tr, tm)
        assert all(torch.equal(o[k], out[k]) for k in KEYS)
    given = R.mesh_strain(track, times, normals=normals.cpu().numpy())
    assert all(torch.equal(given[k], out[k]) for k in KEYS)
    # the canonical reference, and track_strain on host inputs
    can = R.mesh_strain(track, times, reference="canonical")
    assert {k: tuple(v.shape) for k, v in can.items()} == shapes and bool(can["valid"].all())
    v0, v2 = track["vertices"][0], track["vertices"][2]
    a = R.track_strain(v0, 0.3, v2, 0.9, normals)
    b = R.track_strain(v0.cpu().numpy(), 0.3, v2.cpu(), torch.tensor([0.9]), normals.cpu())
    assert all(torch.equal(a[k], b[k]) and torch.equal(a[k], out[k][2]) for k in KEYS)


def test_without_a_deformation_network(monkeypatch):
    r = renderer_for(11, "trained", False)

    def refuse(*a, **k):
        raise AssertionError("the Jacobian kernel was launched")
    monkeypatch.setattr(r.engine, "deform_jacobian", refuse)
    verts, tris = _patch(5)
    J = r.deform_jacobian(verts, 0.4)
    assert J.is_cuda and torch.equal(J, torch.eye(3, device="cuda")[None].expand(25, 3, 3))
    track = r.track_mesh(verts, tris, t=0.3, times=[0.3, 0.9])
    out = r.mesh_strain(track, [0.3, 0.9])
    assert bool(out["valid"].all()) and torch.equal(out["F"], torch.eye(3, device="cuda").expand(2, 25, 3, 3))
    for k in ("det", "stretch", "area", "surface_stretch"):
        assert bool((out[k] == 1).all()), k


def test_engine_methods(case):
    from endosurf_amd import engine
    eng = engine.Engine(torch.device("cuda", torch.cuda.current_device()))
    dev, xd, td = case["dev"], case["x"].cuda(), case["t"].cuda()
    J, xc = eng.deform_jacobian(eng.points(x=xd, t=td), dev.weff, dev.packed, want_xc=True)
    only = eng.deform_jacobian(eng.points(x=xd, t=td), dev.weff, dev.packed)
    assert torch.equal(J.cpu(), case["J"]) and torch.equal(xc.cpu(), case["xc"]) and torch.equal(only, J)
    rows = eng.strain_rows(None, J)
    assert set(rows) == {"F", "det", "stretch", "valid"} and rows["valid"].dtype == torch.bool and rows["F"].shape == (M, 3, 3)
    assert all(close(rows[k].cpu(), v) for k, v in strain.strain_rows(None, case["J"]).items())
    for bad in (lambda: eng.strain_rows(None, J.cpu()), lambda: eng.strain_rows(J[:5], J), lambda: eng.strain_rows(None, J, xd[:5]),
                lambda: eng.strain_rows(None, J.reshape(M, 9))):
        with pytest.raises(ValueError):
            bad()


def test_refusals():
    """Status 1 with a message before anything is launched (the addresses are host numpy's and never dereferenced); M = 0 is status 0."""
    from endosurf_amd import _lib
    lib = _lib.load()
    buf = np.zeros(64, np.float32)
    b = buf.ctypes.data

    def pts(M=4, mode=0):
        p = _lib.es_points()
        p.M, p.mode, p.t_scalar, p.n_per_ray, p.ldz = M, mode, 1, 1, 1
        p.x, p.t, p.rays, p.z = b, b, b, b
        return p
    jac = lambda p, packed=b, weff=b, j=b, xc=b: lib.es_deform_jacobian(C.byref(p), packed, weff, j, xc, None)
    assert jac(pts(mode=1)) == 1 and b"mode 0" in lib.es_last_error()
    assert jac(pts(mode=2)) == 1 and b"mode 0" in lib.es_last_error()
    assert jac(pts(), packed=None) == 1 and b"null buffer" in lib.es_last_error()
    assert jac(pts(), weff=None) == 1 and b"null buffer" in lib.es_last_error()
    assert jac(pts(), j=None, xc=None) == 1 and b"both outputs" in lib.es_last_error()
    nox = pts()
    nox.x = None
    assert jac(nox) == 1 and b"x and t" in lib.es_last_error()
    assert lib.es_deform_jacobian(C.byref(_lib.es_points()), None, None, None, None, None) == 0
    rows = lambda ja=b, jb=b, n=b, M=4, F=b, det=b, st=b, area=b, surf=b, valid=b: lib.es_strain_rows(ja, jb, n, M, F, det, st, area, surf, valid, None)
    assert rows(jb=None) == 1 and b"null buffer" in lib.es_last_error()
    assert rows(F=None, det=None, st=None, area=None, surf=None, valid=None) == 1 and b"every output" in lib.es_last_error()
    assert rows(n=None, surf=None) == 1 and b"normals" in lib.es_last_error()          # area_out without normals
    assert rows(n=None, area=None) == 1 and b"normals" in lib.es_last_error()          # surface_out without normals
    assert rows(M=-1) == 1 and b"negative" in lib.es_last_error()
    assert rows(ja=None, jb=None, n=None, M=0, F=None, det=None, st=None, area=None, surf=None, valid=None) == 0
