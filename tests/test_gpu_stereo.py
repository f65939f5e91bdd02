"""GPU: the stereo matcher on the device (csrc/stereo.hip) against its numpy twin, bit for bit on every element: census,
S, d0, flags, valid and the disparity's fp32 bits on every case of ``stereo_util`` and both image kinds; the speckle filter for any
polling interval; batching and chunking; repeatability; and ``stereo_depth`` / ``FrameSet.from_stereo`` on the analytic scenes.  The
sweep (``stereo_util.SWEEP``) runs every stage over the argument space the matcher admits, and the stage tests give each entry of the
C ABI inputs that only its contract bounds -- any int64 census word, any cost byte, any uint16 sum, any int32 d0 -- still bit for bit."""
import numpy as np
import pytest
import torch

import stereo_util as U
from endosurf_amd import _lib
from endosurf_amd import data as DT
from endosurf_amd import stereo as ST
from endosurf_amd._lib import check, ptr

pytestmark = pytest.mark.gpu

PARAMS = [(*p, kind) for p in U.CASES for kind in U.KINDS]
param_id = lambda q: f"{U.case_id(q)}-{q[5]}"
SELECT_KEYS = ("disparity", "valid", "d0", "flags")
# what the reference's preprocessing calls depth_near_thresh / depth_far_thresh: a working range set from the scenes' geometry (their
# surfaces lie between z = 50 and z = 78), a third of the nearest and 2.5 times the farthest
NEAR, FAR = 20.0, 200.0


@pytest.fixture(scope="module")
def eng():
    from endosurf_amd.engine import Engine
    return Engine("cuda")


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()          # (a copy: the fixtures are read-only)


def host(t):
    return t.cpu().numpy()


def same_select(got, want):
    """Every output equal on every element; the disparity compared as fp32 bit patterns."""
    assert sorted(got) == sorted(SELECT_KEYS)
    for k in SELECT_KEYS:
        g = host(got[k]) if torch.is_tensor(got[k]) else got[k]
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, k
        if k == "disparity":
            g, w = g.view(np.uint32), want[k].view(np.uint32)
        else:
            w = want[k]
        assert np.array_equal(g, w), (k, int((g != w).sum()))


def test_case_list_exercises_every_flag():
    assert U.flags_seen() == (7, 7)


@pytest.mark.parametrize("q", PARAMS, ids=param_id)
def test_kernels_against_the_twin(eng, q):
    H, W, D, dmin, paths, kind = q
    c = U.case(*q)
    for side in ("left", "right"):
        got = eng.census(dev(c[side]))
        assert got.dtype == torch.int64 and np.array_equal(host(got), c["census_" + side])
    S = eng.sgm_volume(dev(c["left"]), dev(c["right"]), D, dmin, U.P1, U.P2, paths)
    assert S.dtype == torch.uint16 and tuple(S.shape) == (H, W, D)
    assert np.array_equal(host(S), c["S"]), int((host(S) != c["S"]).sum())
    same_select(eng.sgm_select(S, dmin, U.UNIQUENESS, U.LR_MAX, True), c["select"])
    same_select(eng.sgm_select(S, dmin, U.UNIQUENESS, U.LR_MAX, False), ST.select(c["S"], dmin, U.UNIQUENESS, U.LR_MAX, False))
    full = eng.stereo_disparity(dev(c["left"]), dev(c["right"]), D, dmin, U.P1, U.P2, paths, U.UNIQUENESS, U.LR_MAX, True, U.SPECKLE_SIZE, 1)
    same_select(full, c["full"])


@pytest.mark.parametrize("q", PARAMS, ids=param_id)
def test_speckle_filter_for_any_poll(eng, q):
    c = U.case(*q)
    sel = c["select"]
    d0, valid = dev(sel["d0"]), dev(sel["valid"])
    for r in (0, 1):
        for poll in (1, 8, 1000):
            got = eng.speckle_filter(d0, valid, U.SPECKLE_SIZE, r, poll=poll)
            assert got.dtype == torch.bool and np.array_equal(host(got), c["speckle"][r]), (r, poll)
    assert torch.equal(d0, dev(sel["d0"])) and torch.equal(valid, dev(sel["valid"]))          # the inputs are left alone


# ---- the stages through the C ABI, where Engine has no method for one -------------------------------------------------------------------------
def abi_cost(census_left, census_right, D, dmin):
    """es_sgm_cost called directly: two int64 [H,W] arrays -> C uint8 [H,W,D] numpy."""
    lib, st = _lib.load(), _lib.stream_ptr()
    H, W = census_left.shape
    cl, cr = dev(census_left), dev(census_right)
    cost = torch.full((H, W, D), 0xAA, device="cuda", dtype=torch.uint8)
    check(lib.es_sgm_cost(ptr(cl), ptr(cr), 1, H, W, D, dmin, ptr(cost), st), "es_sgm_cost")
    return host(cost)


def abi_aggregate(C, p1, p2, paths):
    """es_sgm_aggregate called directly on a given cost volume: uint8 [H,W,D] -> S uint16 [H,W,D] numpy."""
    lib, st = _lib.load(), _lib.stream_ptr()
    H, W, D = C.shape
    cost = dev(C)
    sums = torch.full((H, W, D), 0x5555, device="cuda", dtype=torch.int16)          # (never cleared: the first direction stores)
    check(lib.es_sgm_aggregate(ptr(cost), 1, H, W, D, p1, p2, paths, ptr(sums), st), "es_sgm_aggregate")
    return host(sums).view(np.uint16)


def same_array(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert np.array_equal(got, want), (what, int((got != want).sum()))


# ---- the argument sweep --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(U.SWEEP)), ids=[U.sweep_id(q) for q in U.SWEEP])
def test_sweep_against_the_twin(eng, i):
    H, W, D, dmin, p1, p2, paths, uniqueness, lr_max, size, srange, kind = U.SWEEP[i]
    c = U.sweep_case(i)
    for side in ("left", "right"):
        same_array(host(eng.census(dev(c[side]))), c["census_" + side], "census " + side)
    same_array(abi_cost(c["census_left"], c["census_right"], D, dmin), c["C"], "cost")
    same_array(abi_aggregate(c["C"], p1, p2, paths), c["S"], "aggregate")
    S = eng.sgm_volume(dev(c["left"]), dev(c["right"]), D, dmin, p1, p2, paths)
    assert S.dtype == torch.uint16
    same_array(host(S), c["S"], "S")
    same_select(eng.sgm_select(S, dmin, uniqueness, lr_max, True), c["select"])
    same_select(eng.sgm_select(S, dmin, uniqueness, lr_max, False), c["select_whole"])
    for poll in (1, 1000):
        full = eng.stereo_disparity(dev(c["left"]), dev(c["right"]), D, dmin, p1, p2, paths, uniqueness, lr_max, True, size, srange, poll=poll)
        same_select(full, c["full"])


# ---- each stage on inputs only its contract bounds -----------------------------------------------------------------------------------------------
WORDS = {"uniform": lambda rng, shape: rng.integers(-2 ** 63, 2 ** 63, shape, dtype=np.int64), "ones": lambda rng, shape: np.full(shape, -1, np.int64),
         "sign": lambda rng, shape: np.full(shape, -2 ** 63, np.int64), "zero": lambda rng, shape: np.zeros(shape, np.int64)}
WORD_PAIRS = [("uniform", "uniform"), ("ones", "uniform"), ("uniform", "sign"), ("ones", "sign"), ("sign", "ones"), ("ones", "zero")]


@pytest.mark.parametrize("shape", [(5, 9), (12, 70)], ids=["5x9", "12x70"])
@pytest.mark.parametrize("D", [7, 65])
@pytest.mark.parametrize("dmin", [0, 2])
def test_cost_of_any_census_words(shape, D, dmin):
    rng = np.random.default_rng([2026, 500 + 100 * dmin + D + shape[0]])
    top = 0
    for left, right in WORD_PAIRS:
        cl, cr = WORDS[left](rng, shape), WORDS[right](rng, shape)
        want = ST.cost_volume(cl, cr, D, dmin)
        same_array(abi_cost(cl, cr, D, dmin), want, (left, right))
        top = max(top, int(want.max()))
    assert top == 64          # (all ones against zero: beyond the 62 bits a census sets)


@pytest.mark.parametrize("shape", [(9, 11, 4), (6, 13, 65), (5, 9, 256)], ids=lambda s: "x".join(map(str, s)))
def test_aggregate_of_any_bytes(shape):
    C = np.random.default_rng([2026, 600 + shape[2]]).integers(0, 256, shape, dtype=np.uint8)
    for p1, p2 in ((0, 0), (0, 1024), (1024, 1024), (7, 60)):
        for paths in (4, 8):
            want = ST.aggregate(C, p1, p2, paths)
            same_array(abi_aggregate(C, p1, p2, paths), want, (p1, p2, paths))
            assert int(want.max()) > 63 * paths


def test_aggregate_reaches_the_largest_sum():
    C = U.saturating_volume()
    for paths, top in ((8, 10232), (4, 5116)):
        got = abi_aggregate(C, 1024, 1024, paths)
        same_array(got, ST.aggregate(C, 1024, 1024, paths), paths)
        assert int(got.max()) == top and (got[6, 6, 1:] == top).all()


@pytest.mark.parametrize("D", U.SELECT_D)
@pytest.mark.parametrize("kind", U.SELECT_VOLUMES)
def test_select_of_any_uint16_sums(eng, kind, D):
    want_S = U.select_volume(kind, D)
    S = dev(want_S.view(np.int16)).view(torch.uint16)
    for dmin in (0, 3, U.SELECT_W):
        for uniqueness in (0, 10, 100):
            for lr_max in (0, 1000):
                for subpixel in (True, False):
                    same_select(eng.sgm_select(S, dmin, uniqueness, lr_max, subpixel), ST.select(want_S, dmin, uniqueness, lr_max, subpixel))
    assert torch.equal(S.view(torch.int16), dev(want_S.view(np.int16)))          # the sums are left alone


FIELDS = U.speckle_fields()


@pytest.mark.parametrize("field", FIELDS, ids=[f[0] for f in FIELDS])
def test_speckle_filter_on_hand_made_fields(eng, field):
    name, d0, valid, size, srange, want = field
    assert np.array_equal(ST.speckle_keep(d0, valid, size, srange), want)
    for poll in (1, 7, 1000):
        got = eng.speckle_filter(dev(d0), dev(valid), size, srange, poll=poll)
        assert got.dtype == torch.bool and tuple(got.shape) == valid.shape and np.array_equal(host(got), want), (name, poll)


def test_speckle_segments_stay_inside_their_image_and_row(eng):
    d0, valid, want = U.speckle_stack()
    for size, keep in want.items():
        for poll in (1, 7, 1000):
            got = eng.speckle_filter(dev(d0), dev(valid), size, 0, poll=poll)
            assert np.array_equal(host(got), keep), (size, poll)
            assert np.array_equal(host(got), np.stack([ST.speckle_keep(d0[i], valid[i], size, 0) for i in range(2)]))


def test_a_stack_equals_its_pairs(eng):
    H, W, D, dmin, paths = 24, 33, 16, 3, 8
    pairs = [U.pair(H, W, D, dmin, "noise", seed) for seed in (1, 2)] + [U.pair(H, W, D, dmin, "constant", 3)]
    left, right = dev(np.stack([p[0] for p in pairs])), dev(np.stack([p[1] for p in pairs]))
    args = (D, dmin, U.P1, U.P2, paths)
    tail = (U.UNIQUENESS, U.LR_MAX, True, U.SPECKLE_SIZE, 1)
    singles = [eng.stereo_disparity(left[i], right[i], *args, *tail) for i in range(3)]
    S1 = [eng.sgm_volume(left[i], right[i], *args) for i in range(3)]
    for i, (l, r) in enumerate(pairs):          # (and each is the twin's)
        same_select(singles[i], ST.stereo_disparity(l, r, *args, *tail))
    budget = eng.stereo_scratch_budget
    assert eng._stereo_chunk(3, H, W, D) == 3
    try:
        for b in (budget, 1):
            eng.stereo_scratch_budget = b
            assert eng._stereo_chunk(3, H, W, D) == (3 if b == budget else 1)
            stack = eng.stereo_disparity(left, right, *args, *tail)
            S = eng.sgm_volume(left, right, *args)
            for i in range(3):
                assert torch.equal(S[i].view(torch.int16), S1[i].view(torch.int16))
                for k in SELECT_KEYS:
                    a, w = stack[k][i], singles[i][k]
                    assert torch.equal(a.view(torch.int32), w.view(torch.int32)) if k == "disparity" else torch.equal(a, w), (b, i, k)
    finally:
        eng.stereo_scratch_budget = budget


def test_two_calls_give_the_same_bits(eng):
    H, W, D, dmin, paths = 16, 130, 70, 5, 8
    l, r = (dev(a) for a in U.pair(H, W, D, dmin, "noise"))
    runs = [(eng.sgm_volume(l, r, D, dmin), eng.stereo_disparity(l, r, D, dmin, speckle_size=U.SPECKLE_SIZE)) for _ in range(2)]
    assert torch.equal(runs[0][0].view(torch.int16), runs[1][0].view(torch.int16))
    for k in SELECT_KEYS:
        a, b = runs[0][1][k], runs[1][1][k]
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) if k == "disparity" else torch.equal(a, b), k


def test_image_kinds_give_the_same_disparity(eng):
    s = U.scene("bump")
    grey_l, grey_r = s["left"], s["right"]
    want = eng.stereo_disparity(dev(grey_l), dev(grey_r), U.SCENE_D)
    rgb = lambda g: np.stack([g, g, g], -1)                                            # 77 + 150 + 29 = 256: this picture's grey is g
    as_float = lambda g: (rgb(g).astype(np.float32) + np.float32(0.5)) / np.float32(255)      # to8b truncates back to g
    assert np.array_equal(ST.to_grey(as_float(grey_l)), grey_l)
    for l, r in ((rgb(grey_l), rgb(grey_r)), (as_float(grey_l), as_float(grey_r))):
        got = eng.stereo_disparity(dev(l), dev(r), U.SCENE_D)
        for k in SELECT_KEYS:
            assert torch.equal(got[k], want[k]), k
        same_select(got, ST.stereo_disparity(l, r, U.SCENE_D))
    # a picture with three different channels: the device's grey is the twin's
    rng = np.random.default_rng(5)
    cl, cr = rng.integers(0, 256, (2, 20, 40, 3), dtype=np.uint8)
    same_select(eng.stereo_disparity(dev(cl), dev(cr), 16), ST.stereo_disparity(cl, cr, 16))
    fl, fr = rng.uniform(-0.1, 1.1, (2, 20, 40, 3)).astype(np.float32)
    same_select(eng.stereo_disparity(dev(fl), dev(fr), 16), ST.stereo_disparity(fl, fr, 16))


def scene_sequence():
    names = ("plane", "slant", "bump")
    left = np.stack([np.stack([U.scene(n)["left"]] * 3, -1) for n in names])
    right = np.stack([np.stack([U.scene(n)["right"]] * 3, -1) for n in names])
    K = np.tile(np.eye(4, dtype=np.float32), (3, 1, 1))
    K[:, 0, 0] = K[:, 1, 1] = U.FOCAL
    K[:, 0, 2], K[:, 1, 2] = (U.SCENE_W - 1) / 2.0, (U.SCENE_H - 1) / 2.0
    poses = np.tile(np.eye(4, dtype=np.float32), (3, 1, 1))
    return left, right, K, poses, np.stack([U.scene(n)["depth"] for n in names])


def test_stereo_depth_and_from_stereo(eng):
    left, right, K, poses, z = scene_sequence()
    on_dev = DT.stereo_depth(dev(left), dev(right), U.FOCAL, U.BASELINE, U.SCENE_D, near=NEAR, far=FAR, engine=eng, speckle_size=U.SPECKLE_SIZE)
    on_host = DT.stereo_depth(left, right, U.FOCAL, U.BASELINE, U.SCENE_D, near=NEAR, far=FAR, speckle_size=U.SPECKLE_SIZE)
    assert sorted(on_dev) == sorted(on_host) == ["color_mask", "depth", "depth_mask", "disparity", "valid"]
    for k, v in on_host.items():
        g = on_dev[k]
        assert g.is_cuda and not v.is_cuda and g.dtype == v.dtype and g.shape == v.shape == (3, U.SCENE_H, U.SCENE_W), k
        assert np.array_equal(host(g).view(np.uint32) if g.dtype == torch.float32 else host(g), v.numpy().view(np.uint32) if v.dtype == torch.float32 else v.numpy()), k
    for i, name in enumerate(("plane", "slant", "bump")):
        ok = host(on_dev["depth_mask"][i])
        rel = np.abs(host(on_dev["depth"][i]).astype(np.float64)[ok] - z[i][ok]) / z[i][ok]
        print(f"\n{name}: {ok.mean():.3f} of the pixels have depth, mean relative depth error {rel.mean():.4%}, worst {rel.max():.3%}")
        assert ok.mean() > 0.5
        assert rel.mean() < 0.02
    kw = dict(max_disparity=U.SCENE_D, near=NEAR, far=FAR, engine=eng, speckle_size=U.SPECKLE_SIZE)
    fs_dev = DT.FrameSet.from_stereo(dev(left), dev(right), dev(K), dev(poses), U.BASELINE, **kw)
    fs_host = DT.FrameSet.from_stereo(left, right, K, poses, U.BASELINE, **kw)
    d = on_dev["depth"]
    bounds = torch.stack([torch.stack([d[i][d[i] > 0].min(), d[i][d[i] > 0].max()]) for i in range(3)])
    fs_raw = DT.FrameSet.from_raw(dev((left / 255.0).astype(np.float32)), d, dev(K), dev(poses), bounds, color_masks=on_dev["color_mask"].float(),
                                  depth_masks=(d > 0).float()[..., None])
    for other in (fs_host, fs_raw):
        for name in ("colors", "depths", "depth_masks", "color_masks", "masks", "rays", "intrinsics", "poses", "scale_mat", "bbox_minmax"):
            assert torch.equal(getattr(fs_dev, name), getattr(other, name)), name
        assert fs_dev.depth_scale == other.depth_scale
    assert tuple(fs_dev.depths.shape) == (3, U.SCENE_H, U.SCENE_W, 1) and bool((fs_dev.depth_masks == (fs_dev.depths > 0)).all())
    own = DT.FrameSet.from_stereo(dev(left), dev(right), dev(K), dev(poses), U.BASELINE, depth_masks=torch.ones(3, U.SCENE_H, U.SCENE_W, 1), **kw)
    assert bool((own.depth_masks == 1).all())
