"""GPU, kernel level through the C ABI: es_segment_visible (csrc/visible.hip) against the segment rule of ``flow.segment_visible``
 run in fp32 on es_query_sdf_tiles -- the value a row saw, bit for bit -- and against the fp64 twin under the two caps the
fp32 oracle twin meets on the CPU (tests/test_flow_host.py).  Every test prints the figures it asserts on."""
import numpy as np
import pytest
import torch

from flow_util import KINDS, MARGIN, visible_case
from test_gpu_trace import dev_for
from trace_util import CASES, ITERS_CAP, STATUS_CAP, same

from endosurf_amd import flow as FL

pytestmark = pytest.mark.gpu

INF = float("inf")
KEYS = ("status", "iters", "blocker", "clearance", "free_to")
N = 515


def visible(dev, a, b, t, use_deform, margin=MARGIN, tau=0.0, relax=1.0, min_step=1e-3, max_iters=128, tile_points=0, optional=True,
            t_scalar=False):
    """es_segment_visible on host tensors; every output pre-filled with a value the kernel never writes."""
    n, ptr = a.shape[0], dev._lib.ptr
    ad, bd, td = a.cuda().contiguous(), b.cuda().contiguous(), t.reshape(-1).cuda().contiguous()
    out = {"status": torch.full((n,), -7, device="cuda", dtype=torch.int32)}
    if optional:
        out.update(iters=torch.full((n,), -7, device="cuda", dtype=torch.int32), blocker=torch.full((n,), float("nan"), device="cuda"),
                   clearance=torch.full((n,), float("nan"), device="cuda"), free_to=torch.full((n,), float("nan"), device="cuda"))
    dev._lib.check(dev.lib.es_segment_visible(ptr(ad), ptr(bd), ptr(td), int(t_scalar), n, margin, tau, relax, min_step, max_iters, tile_points,
                                              ptr(dev.packed), ptr(dev.weff), int(use_deform), ptr(out["status"]), ptr(out.get("iters")),
                                              ptr(out.get("blocker")), ptr(out.get("clearance")), ptr(out.get("free_to")), dev._lib.stream_ptr()), "es_segment_visible")
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def query_fn(dev, use_deform, tile_points=32):
    """``sdf_fn`` of the twin: the library's own tiled query, inputs and results on the host."""
    return lambda x, t: dev.query(x.contiguous(), t.reshape(-1).contiguous(), use_deform, tile_points)[:, None]


@pytest.fixture(scope="module", params=[(m, s, d) for m, s in CASES for d in (True, False)], ids=lambda p: f"{p[0]}{p[1]}{'' if p[2] else '-static'}")
def vc(request):
    """One state with or without its deformation network: the three kinds of segments in fp32, the device's result on the 515 rows of
    each, and the host twin in fp32 on the library's tiled query."""
    mode, seed, use_deform = request.param
    v = dict(visible_case(mode, seed, use_deform))
    v["dev"], v["use_deform"] = dev_for(mode, seed), use_deform
    v["a32"], v["t32"] = v["a"].float(), v["t"].float()
    for kind in KINDS:
        b = v["ends"][kind].float()
        v[kind, "b32"] = b
        v[kind, "dev"] = visible(v["dev"], v["a32"], b, v["t32"], use_deform)
        v[kind, "twin"] = FL.segment_visible(query_fn(v["dev"], use_deform), v["a32"], b, v["t32"])
    return v


def test_the_kernel_is_the_twin_on_the_tiled_query_bit_for_bit(vc):
    """status, iters and blocker are the twin's; clearance is the bit pattern of the smallest value the query returns along the row
    (the twin keeps exactly that).  M = 1, 31, 32, 33, 64, 65 and 515, each launched on its own."""
    dev, ud = vc["dev"], vc["use_deform"]
    for kind in KINDS:
        full, twin = vc[kind, "dev"], vc[kind, "twin"]
        for k in KEYS:
            assert same(full[k], twin[k]), (kind, k, int((full["status"] != twin["status"]).sum()), int((full["iters"] != twin["iters"]).sum()))
        for n in (1, 31, 32, 33, 64, 65):
            part = visible(dev, vc["a32"][:n], vc[kind, "b32"][:n], vc["t32"][:n], ud)
            for k in KEYS:
                assert same(part[k], twin[k][:n]), (kind, n, k)
        st, it = full["status"], full["iters"]
        assert bool(((st >= 1) & (st <= 3)).all()) and bool(((it >= 0) & (it <= 128)).all())
        assert bool((full["blocker"][st != FL.OCCLUDED] == INF).all()) and bool(torch.isfinite(full["blocker"][st == FL.OCCLUDED]).all())
        assert bool((full["clearance"][it == 0] == INF).all()) and bool((full["clearance"][st == FL.OCCLUDED] <= 0).all())
        assert bool((full["clearance"][st == FL.FREE][it[st == FL.FREE] > 0] > 0).all())
        print(f"\n[{vc['name']} {kind}] FREE / OCCLUDED / UNKNOWN {torch.bincount(st, minlength=4).tolist()[1:]}; evaluations per row mean "
              f"{float(it.double().mean()):.2f} max {int(it.max())}")
    assert len(set(vc["past", "dev"]["iters"].tolist())) > 4          # rows do need different numbers of evaluations
    # the twin on 64-point tiles sees the same values
    other = FL.segment_visible(query_fn(dev, ud, 64), vc["a32"][:130], vc["past", "b32"][:130], vc["t32"][:130])
    for k in KEYS:
        assert same(other[k], vc["past", "twin"][k][:130]), k


def test_rows_do_not_depend_on_the_batch_or_the_tile(vc):
    """Both tile heights, a shuffled batch, a second call: every output of a row as in the 515-row run, bit for bit."""
    dev, ud, a, t = vc["dev"], vc["use_deform"], vc["a32"], vc["t32"]
    for kind in ("hit", "past"):
        b, full = vc[kind, "b32"], vc[kind, "dev"]
        for tile in (32, 64):
            for n in (65, N):
                part = visible(dev, a[:n], b[:n], t[:n], ud, tile_points=tile)
                for k in KEYS:
                    assert same(part[k], full[k][:n]), (kind, tile, n, k)
        again = visible(dev, a, b, t, ud)
        perm = torch.from_numpy(np.random.default_rng(3).permutation(N).copy())
        shuffled = visible(dev, a[perm], b[perm], t[perm], ud)
        for k in KEYS:
            assert same(again[k], full[k]) and same(shuffled[k], full[k][perm]), (kind, k)
    # one shared time read as t_scalar
    t0 = t[:1].expand(70).contiguous()
    rows, shared = visible(dev, a[:70], vc["past", "b32"][:70], t0, ud), visible(dev, a[:70], vc["past", "b32"][:70], t[:1], ud, t_scalar=True)
    for k in KEYS:
        assert same(rows[k], shared[k]), k


def test_against_the_fp64_twin(vc):
    """The device's walk is the fp64 twin's under the two caps the fp32 oracle twin meets on the CPU."""
    for kind in KINDS:
        full, t64 = vc[kind, "dev"], vc[kind, 64]
        d_status, d_iters = int((full["status"] != t64["status"]).sum()), int((full["iters"] != t64["iters"]).sum())
        print(f"\n[{vc['name']} {kind}] status differs from the fp64 twin on {d_status} rows (cap {STATUS_CAP}), iters on {d_iters} (cap {ITERS_CAP})")
        assert d_status <= STATUS_CAP and d_iters <= ITERS_CAP
    hit = vc["hit"]
    assert bool((vc["mid", "dev"]["status"][hit] == FL.FREE).all()) and bool((vc["past", "dev"]["status"][hit] == FL.OCCLUDED).all())
    # OCCLUDED at the fp64 hit +- margin, on every traced row: the hit's arc length lies in the bracket (free_to, blocker] of the crossing
    # the walk found, to the margin at either end
    past = vc["past", "dev"]
    L = torch.sqrt(((vc["ends"]["hit"] - vc["a"]) ** 2).sum(-1))
    lo, hi = (past["free_to"].double() - L)[hit], (past["blocker"].double() - L)[hit]
    print(f"[{vc['name']} past] free_to - L max {float(lo.max()):.3e}; blocker - L min {float(hi.min()):.3e} max {float(hi.max()):.3e}; blocker "
          f"within the margin of the hit on {int((hi.abs() <= MARGIN).sum())} of {int(hit.sum())} rows")
    assert bool((lo <= MARGIN).all()) and bool((hi >= -MARGIN).all()) and bool((past["free_to"] < past["blocker"])[hit].all())
    assert int((vc["hit", "dev"]["status"][hit] == FL.FREE).sum()) > 0.5 * int(hit.sum())


def test_arguments_follow_the_rule(vc):
    """tau, relax, min_step, margin and the cap, each against the twin on the tiled query; the walk does not know the cap."""
    dev, ud = vc["dev"], vc["use_deform"]
    a, b, t = vc["a32"][:97], vc["past", "b32"][:97], vc["t32"][:97]
    for args in (dict(tau=0.02), dict(relax=0.5), dict(min_step=0.02), dict(margin=0.0), dict(margin=0.06), dict(max_iters=1), dict(max_iters=3)):
        got, want = visible(dev, a, b, t, ud, **args), FL.segment_visible(query_fn(dev, ud), a, b, t, **args)
        for k in KEYS:
            assert same(got[k], want[k]), (args, k)
        if "max_iters" in args:
            cap, full = args["max_iters"], vc["past", "dev"]
            done = full["iters"][:97] <= cap
            assert int(done.sum()) < 97
            for k in KEYS:
                assert same(got[k][done], full[k][:97][done]), (args, k)
            assert bool((got["status"][~done] == FL.UNKNOWN).all()) and bool((got["iters"][~done] == cap).all())
            assert bool((got["blocker"][~done] == INF).all())


def test_special_rows_keep_their_neighbours():
    """A NaN row, a == b, a segment wholly outside the unit ball, margin > L, a NaN time -- between valid rows whose bits they leave alone."""
    mode, seed = CASES[0]
    v = visible_case(mode, seed, True)
    dev = dev_for(mode, seed)
    a, b, t = v["a"].float()[:40].clone(), v["ends"]["past"].float()[:40].clone(), v["t"].float()[:40].clone()
    base = visible(dev, a, b, t, True)
    b[3, 1] = float("nan")
    b[9] = a[9]
    a[17], b[17] = torch.tensor([0.0, 3.0, -1.5]), torch.tensor([0.5, 3.0, 0.0])
    b[25] = a[25] + torch.tensor([0.0, 0.0, 0.003])
    t[33] = float("nan")
    out = visible(dev, a, b, t, True)
    keep = torch.ones(40, dtype=torch.bool)
    keep[[3, 9, 17, 25, 33]] = False
    for k in KEYS:
        assert same(out[k][keep], base[k][keep]), k
    print(f"\nspecial rows: status {out['status'][[3, 9, 17, 25, 33]].tolist()} iters {out['iters'][[3, 9, 17, 25, 33]].tolist()}")
    assert out["status"][[3, 9, 17, 25, 33]].tolist() == [FL.UNKNOWN, FL.UNKNOWN, FL.FREE, FL.FREE, FL.UNKNOWN]
    assert out["iters"][[3, 9, 17, 25, 33]].tolist() == [0, 0, 0, 0, 0]
    assert bool((out["blocker"][~keep] == INF).all()) and bool((out["clearance"][~keep] == INF).all()) and bool((out["free_to"][~keep] == -INF).all())
    twin = FL.segment_visible(query_fn(dev, True), a, b, t)
    for k in KEYS:
        assert same(out[k], twin[k]), k


def test_empty_batches_null_outputs_and_refusals():
    """M = 0 is status 0 without a launch; the four optional outputs may be null; each bad argument is status 1 with its name in
    es_last_error() before anything is launched (the addresses are host numpy's and never dereferenced)."""
    from endosurf_amd import _lib
    lib = _lib.load()
    mode, seed = CASES[0]
    v = visible_case(mode, seed, True)
    dev = dev_for(mode, seed)
    a, b, t = v["a"].float()[:70], v["ends"]["past"].float()[:70], v["t"].float()[:70]
    full, lean = visible(dev, a, b, t, True), visible(dev, a, b, t, True, optional=False)
    assert sorted(lean) == ["status"] and same(lean["status"], full["status"])
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data

    def call(M=4, margin=5e-3, tau=0.0, relax=1.0, min_step=1e-3, max_iters=128, tile_points=0, origins=p, points=p, t=p, packed=p, status=p):
        return lib.es_segment_visible(origins, points, t, 0, M, margin, tau, relax, min_step, max_iters, tile_points, packed, p, 1, status, None,
                                      None, None, None, None)

    assert call(M=0, origins=None, points=None, t=None, packed=None, status=None) == 0
    bad = [("M", dict(M=-1)), ("margin", dict(margin=-1e-9)), ("margin", dict(margin=float("inf"))), ("margin", dict(margin=float("nan"))),
           ("tau", dict(tau=float("nan"))), ("tau", dict(tau=float("inf"))), ("relax", dict(relax=0.0)), ("relax", dict(relax=1.5)),
           ("relax", dict(relax=float("nan"))), ("min_step", dict(min_step=0.0)), ("min_step", dict(min_step=float("inf"))),
           ("min_step", dict(min_step=float("nan"))), ("max_iters", dict(max_iters=0)), ("max_iters", dict(max_iters=1025)),
           ("tile_points", dict(tile_points=16)), ("null buffer", dict(origins=None)), ("null buffer", dict(points=None)),
           ("null buffer", dict(t=None)), ("null buffer", dict(packed=None)), ("null buffer", dict(status=None))]
    for name, kw in bad:
        assert call(**kw) == 1 and name.encode() in lib.es_last_error(), (name, kw, lib.es_last_error())
        if name != "M":          # the arguments are checked before M == 0 returns; the buffers only when M > 0 needs them
            assert call(M=0, **kw) == (0 if name == "null buffer" else 1)
