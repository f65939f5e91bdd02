"""CPU: the stereo matcher's numpy twin (endosurf_amd/stereo.py) on analytic scenes with ground truth in closed form and
on the algebra its rules imply; the path recurrence against a scalar restatement of the header's formula; what the device tests' argument
sweep, uint16 volumes and speckle fields cover, as conditions on those inputs; ``disparity_to_depth`` against the reference's rule restated here; ``close_mask``'s properties; and the
refusals of the library's stereo entries, which come before any launch."""
import ctypes as C

import numpy as np
import pytest
import torch

import stereo_util as U
from endosurf_amd import data as DT
from endosurf_amd import stereo as ST


# ---- 1. the twin against ground truth ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paths", [4, 8])
@pytest.mark.parametrize("name", sorted(U.SCENES))
def test_twin_on_analytic_scenes(name, paths):
    e = U.scene_errors(name, paths)
    print(f"\n{name}, {paths} paths: density {e['density']:.4f}, within 1 px {e['within'][1.0]:.4f}, within 0.5 px {e['within'][0.5]:.4f}, "
          f"mean |error| {e['mean_abs_error']:.3f} px over {e['count']} pixels")
    assert e["density"] >= 0.98
    assert e["within"][1.0] >= 0.99


def test_case_list_exercises_every_flag():
    on, off = U.flags_seen()
    assert on == 7 and off == 7, (on, off)


# ---- 2. algebra -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", U.CASES, ids=U.case_id)
def test_constant_pair(p):
    H, W, D, dmin, paths = p
    c = U.case(*p, "constant")
    assert (c["S"].astype(np.int64).argmin(-1) == 0).all()
    sel = c["select"]
    assert (sel["d0"][sel["valid"]] == 0).all()
    assert (sel["disparity"][sel["valid"]] == np.float32(dmin)).all()
    assert (sel["disparity"][~sel["valid"]] == 0).all() and (sel["d0"][~sel["valid"]] == -1).all()
    if dmin == 0:
        assert sel["valid"].all()


@pytest.mark.parametrize("k,dmin,paths", [(5, 0, 8), (9, 3, 8), (0, 0, 4), (12, 4, 4)])
def test_shifted_pair(k, dmin, paths):
    H, W, D = 20, 64, 16
    rng = np.random.default_rng(k)
    left = rng.integers(0, 256, (H, W), dtype=np.uint8)
    right = rng.integers(0, 256, (H, W), dtype=np.uint8)
    right[:, :W - k] = left[:, k:]
    r = ST.stereo_disparity(left, right, D, dmin, paths=paths)
    inner = np.zeros((H, W), bool)
    inner[3:-3, dmin + D + 4:-4] = True          # away from the border: the whole range and the whole census window lie in the image
    ok = r["valid"] & inner
    assert ok.sum() > 0.9 * inner.sum()
    assert (r["d0"][ok] == k - dmin).all()
    assert np.abs(r["disparity"][ok] - k).max() < 0.5


@pytest.mark.parametrize("p", U.CASES, ids=U.case_id)
def test_sum_bounds(p):
    H, W, D, dmin, paths = p
    for kind in U.KINDS:
        c = U.case(*p, kind)
        S4, S8 = ST.aggregate(c["C"], U.P1, U.P2, 4), ST.aggregate(c["C"], U.P1, U.P2, 8)
        assert (S8 >= S4).all()
        assert int(S4.max()) <= 4 * (63 + U.P2) and int(S8.max()) <= 8 * (63 + U.P2)
        assert np.array_equal(c["S"], S8 if paths == 8 else S4)
        for r in ST.DIRECTIONS:          # every path cost is at least the matching cost and at most 63 + P2
            L = ST.path_costs(c["C"], r, U.P1, U.P2)
            assert (L >= c["C"]).all() and int(L.max()) <= 63 + U.P2


def test_census_bits_and_grey():
    g = np.arange(63, dtype=np.uint8).reshape(7, 9) * 3
    c = ST.census(g)
    # at the centre every neighbour before it in row-major order is smaller, every one after it larger: the top 31 of 62 bits
    assert int(c[3, 4]) == ((1 << 31) - 1) << 31
    assert int(c.max()) < 1 << 62 and int(c.min()) >= 0
    assert (ST.census(np.full((5, 6), 9, np.uint8)) == 0).all()
    rgb = np.random.default_rng(0).integers(0, 256, (4, 5, 3), dtype=np.uint8)
    grey = ST.to_grey(rgb)
    want = (77 * rgb[..., 0].astype(int) + 150 * rgb[..., 1].astype(int) + 29 * rgb[..., 2].astype(int) + 128) >> 8
    assert grey.dtype == np.uint8 and np.array_equal(grey, want)
    assert np.array_equal(ST.to_grey(np.stack([grey] * 3, -1)), grey)          # 77 + 150 + 29 = 256: grey stays grey
    assert np.array_equal(ST.to_grey(rgb.astype(np.float32) / 255), ST.to_grey(DT.to8b(rgb.astype(np.float32) / 255)))
    assert np.array_equal(ST.popcount64(np.array([0, 1, (1 << 62) - 1, 0b1011], np.int64)), [0, 1, 62, 3])


def test_speckle_segments():
    d0 = np.zeros((6, 8), np.int32)
    d0[:, 4:] = 5                                  # two halves, 24 pixels each, that differ by more than the range
    valid = np.ones((6, 8), bool)
    valid[2, :] = False                            # ... cut into four segments of 8 and 12 pixels
    assert np.array_equal(ST.speckle_keep(d0, valid, 9, 1), valid & (np.arange(6)[:, None] > 2))
    assert np.array_equal(ST.speckle_keep(d0, valid, 8, 1), valid)
    assert not ST.speckle_keep(d0, valid, 13, 1).any()
    assert np.array_equal(ST.speckle_keep(d0, valid, 13, 5), valid)                                      # joined across the halves: 16 and 24
    assert np.array_equal(ST.speckle_keep(d0, valid, 17, 5), valid & (np.arange(6)[:, None] > 2))


def flood_keep(d0, valid, size, max_diff):
    """``speckle_keep`` by a flood fill from every pixel not yet visited: independent of how labels travel."""
    H, W = valid.shape
    seen, keep = np.zeros((H, W), bool), np.zeros((H, W), bool)
    for y0 in range(H):
        for x0 in range(W):
            if not valid[y0, x0] or seen[y0, x0]:
                continue
            seen[y0, x0] = True
            stack, members = [(y0, x0)], []
            while stack:
                y, x = stack.pop()
                members.append((y, x))
                for v, u in ((y, x - 1), (y, x + 1), (y - 1, x), (y + 1, x)):
                    if 0 <= v < H and 0 <= u < W and valid[v, u] and not seen[v, u] and abs(int(d0[v, u]) - int(d0[y, x])) <= max_diff:
                        seen[v, u] = True
                        stack.append((v, u))
            if len(members) >= size:
                for y, x in members:
                    keep[y, x] = True
    return keep


@pytest.mark.parametrize("p", U.CASES, ids=U.case_id)
def test_speckle_against_a_flood_fill(p):
    sel = U.case(*p, "noise")["select"]
    for r in (0, 1):
        assert np.array_equal(U.case(*p, "noise")["speckle"][r], flood_keep(sel["d0"], sel["valid"], U.SPECKLE_SIZE, r))
    # a segment whose smallest index has to travel right to left and upwards: a U, open at the top
    valid = np.zeros((5, 7), bool)
    valid[:, 1] = valid[:, 5] = valid[4, 1:6] = True
    d0 = np.zeros((5, 7), np.int32)
    assert np.array_equal(ST.speckle_keep(d0, valid, 13, 0), valid) and not ST.speckle_keep(d0, valid, 14, 0).any()


FIELDS = U.speckle_fields()


@pytest.mark.parametrize("field", FIELDS, ids=[f[0] for f in FIELDS])
def test_speckle_on_hand_made_fields(field):
    name, d0, valid, size, srange, want = field
    got = ST.speckle_keep(d0, valid, size, srange)
    assert np.array_equal(got, flood_keep(d0, valid, size, srange)) and np.array_equal(got, want), name


def test_speckle_fields_are_what_they_claim():
    by_name = {f[0]: f for f in FIELDS}
    snake = by_name["snake-159"][2]
    assert snake.shape == (9, 31) and int(snake.sum()) == 159 and snake[0::2].all() and np.array_equal(by_name["snake-159"][5], snake)
    assert not by_name["snake-160"][5].any()
    d0 = by_name["extreme-row"][1]
    assert d0.dtype == np.int32 and d0.tolist() == [[2 ** 31 - 1, -2 ** 31, 5, 6]] and by_name["extreme-row"][5].tolist() == [[False, False, True, True]]
    with np.errstate(over="ignore"):          # in 32 bits the first difference wraps to 1: a sweep that subtracts in int32 keeps all four
        assert np.abs(d0[0, :1] - d0[0, 1:2]).tolist() == [1]
    assert np.array_equal(by_name["size-0"][5], by_name["size-0"][2])
    d0, valid, want = U.speckle_stack()
    for size, keep in want.items():
        per_image = np.stack([ST.speckle_keep(d0[i], valid[i], size, 0) for i in range(2)])
        assert np.array_equal(per_image, keep) and np.array_equal(per_image, np.stack([flood_keep(d0[i], valid[i], size, 0) for i in range(2)])), size
    # ... and a filter that ran over the stack as one 8 x 5 image, or over each image as one row of 20, would answer differently
    assert not np.array_equal(ST.speckle_keep(d0.reshape(8, 5), valid.reshape(8, 5), 6, 0).reshape(2, 4, 5), want[6])
    assert not np.array_equal(np.stack([ST.speckle_keep(d0[i].reshape(1, 20), valid[i].reshape(1, 20), 2, 0).reshape(4, 5) for i in range(2)]), want[2])


def test_stereo_errors():
    d = np.array([[1.0, 2.0, 0.0, 4.0]], np.float32)
    e = ST.stereo_errors(d, d > 0, np.array([[1.25, 4.0, 3.0, 4.0]]), np.array([[True, True, True, False]]), thresholds=(0.5, 1))
    assert e["density"] == pytest.approx(2 / 3) and e["mean_abs_error"] == pytest.approx(1.125)
    assert e["within"] == {0.5: 0.5, 1.0: 0.5} and e["count"] == 2


def test_matcher_arguments_are_checked():
    for bad in (dict(max_disparity=0), dict(max_disparity=257), dict(max_disparity=8, min_disparity=-1), dict(max_disparity=8, p1=9, p2=8),
                dict(max_disparity=8, p2=1025), dict(max_disparity=8, paths=5), dict(max_disparity=8, uniqueness=101),
                dict(max_disparity=8, lr_max=-1), dict(max_disparity=8, speckle_size=-1)):
        with pytest.raises(ValueError):
            ST.check_matcher(**bad)


def test_min_disparity_is_bounded_by_the_largest_image_side():
    for dmin in (8193, 2 ** 31 - 1):
        with pytest.raises(ValueError, match="min_disparity"):
            ST.check_matcher(8, min_disparity=dmin)
    assert ST.check_matcher(8, min_disparity=8192)[1] == 8192
    # nothing is lost: from W on, every min_disparity means "no column", so every cost is 63 and every pixel fails left-right
    l, r = U.pair(6, 9, 4, 0, "noise")
    at_w, beyond = (ST.stereo_disparity(l, r, 4, dmin) for dmin in (9, 8192))
    assert (ST.sgm_volume(l, r, 4, 9) == ST.sgm_volume(l, r, 4, 8192)).all() and (ST.cost_volume(ST.census(l), ST.census(r), 4, 9) == 63).all()
    for k in ("valid", "d0", "flags"):
        assert np.array_equal(at_w[k], beyond[k]), k
    assert not beyond["valid"].any() and (beyond["flags"] & ST.FLAG_LEFT_RIGHT).all()


# ---- 2b. the recurrence restated, the largest sums, and what the sweep and the stage volumes cover ---------------------------------------------
SCALAR_SHAPES = [(6, 7, 5), (4, 5, 1), (3, 6, 2), (1, 7, 4), (6, 1, 3), (1, 1, 1), (5, 4, 3)]
SCALAR_PENALTIES = [(0, 0), (0, 5), (7, 60), (1024, 1024)]


@pytest.mark.parametrize("shape", SCALAR_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_path_costs_against_a_scalar_restatement(shape):
    C = np.random.default_rng([2026, 400 + SCALAR_SHAPES.index(shape)]).integers(0, 256, shape, dtype=np.uint8)
    for p1, p2 in SCALAR_PENALTIES:
        total = np.zeros(shape, np.int64)
        for r in ST.DIRECTIONS:
            want = np.array(U.path_costs_scalar(C.tolist(), r, p1, p2), np.int64).reshape(shape)
            got = ST.path_costs(C, r, p1, p2)
            assert np.array_equal(got, want), (r, p1, p2, int((got != want).sum()))
            total += want
            if r == ST.DIRECTIONS[3]:
                assert np.array_equal(ST.aggregate(C, p1, p2, 4), total)
        assert np.array_equal(ST.aggregate(C, p1, p2, 8), total)


def test_saturating_volume_reaches_the_largest_sum():
    C = U.saturating_volume()
    S8, S4 = ST.aggregate(C, 1024, 1024, 8), ST.aggregate(C, 1024, 1024, 4)
    assert S8.dtype == np.uint16 and int(S8.max()) == 8 * (255 + 1024) == 10232 and int(S4.max()) == 4 * (255 + 1024) == 5116
    assert (S8[6, 6, 1:] == 10232).all() and S8[6, 6, 0] == 0
    for r in ST.DIRECTIONS:
        assert np.array_equal(ST.path_costs(C, r, 1024, 1024), np.array(U.path_costs_scalar(C.tolist(), r, 1024, 1024)))


def test_sweep_covers_what_it_claims():
    """Conditions on the sweep's inputs, by the twin alone: what tests/test_gpu_stereo.py can only catch if it occurs."""
    assert len(U.SWEEP) >= U.SWEEP_DRAWN and U.SWEEP[:U.SWEEP_DRAWN] == [U._draw(i) for i in range(U.SWEEP_DRAWN)]
    on = off = 0
    kd_paths, seen = set(), {k: 0 for k in ("no_right_column", "tie", "subpixel", "p2_1024", "dmin_past_w", "speckle", "p_zero", "p1_is_p2")}
    for i, q in enumerate(U.SWEEP):
        H, W, D, dmin, p1, p2, paths, uniqueness, lr_max, size, srange, kind = q
        assert 1 <= H <= 24 and 1 <= W <= 140 and H * W * D <= U.SWEEP_MAX_CELLS and D in U.SWEEP_D and kind in U.SWEEP_KINDS
        ST.check_matcher(D, dmin, p1, p2, paths, uniqueness, lr_max, size, srange)
        c = U.sweep_case(i)
        f = c["full"]["flags"].reshape(-1)
        on |= int(np.bitwise_or.reduce(f))
        off |= int(np.bitwise_or.reduce(~f & 7))
        kd_paths.add(((D + 63) // 64, paths))
        Si = c["S"].astype(np.int64)
        d0 = Si.argmin(-1)
        seen["no_right_column"] += bool((c["dR"] == -1).any())
        seen["tie"] += bool(((Si == Si.min(-1, keepdims=True)).sum(-1) > 1).any())
        seen["subpixel"] += bool(((d0 > 0) & (d0 < D - 1)).any())
        seen["p2_1024"] += p2 == 1024
        seen["dmin_past_w"] += dmin >= W
        seen["speckle"] += bool((f & ST.FLAG_SPECKLE).any())
        seen["p_zero"] += p1 == 0 == p2
        seen["p1_is_p2"] += p1 == p2
    print(f"\n{len(U.SWEEP)} configurations: flags set {on}, clear {off}; {seen}")
    assert on == 7 and off == 7, (on, off)
    assert kd_paths == {(kd, paths) for kd in (1, 2, 3, 4) for paths in (4, 8)}, sorted(kd_paths)
    assert all(seen.values()), seen
    for name, values in (("uniqueness", (0, 100)), ("lr_max", (0,)), ("size", (0, 1))):
        col = {"uniqueness": 7, "lr_max": 8, "size": 9}[name]
        assert set(values) <= {q[col] for q in U.SWEEP}, name
    assert any(q[8] >= q[2] for q in U.SWEEP) and any(q[9] > q[0] * q[1] for q in U.SWEEP) and any(q[10] == 300 for q in U.SWEEP)


def signed_key_argmin(S):
    """What a 32-bit SIGNED key ``S << 16 | d`` picks: the argmin the device took before its keys became unsigned."""
    keys = ((S.astype(np.int64) << 16) | np.arange(S.shape[-1])).astype(np.uint32).view(np.int32)
    return keys.min(-1) & 0xffff, keys.min(-1) >> 16


def test_select_volumes_tell_signed_keys_from_unsigned():
    """The volumes of the device test order differently under signed 32-bit keys, so that test fails on a library with such keys."""
    for D in U.SELECT_D:
        for kind in U.SELECT_VOLUMES:
            S = U.select_volume(kind, D)
            assert S.dtype == np.uint16 and S.shape == (U.SELECT_H, U.SELECT_W, D)
            d0, s0 = signed_key_argmin(S)
            want = S.astype(np.int64).argmin(-1)
            if kind in ("uniform", "edge") and D >= 2:
                assert (d0 != want).mean() > 0.25, (kind, D)          # (about half the pixels at D = 2, nearly all at large D)
            if kind in ("max", "high"):          # the argmin survives, the minimum read back by an arithmetic shift does not
                assert np.array_equal(d0, want) and (s0 < 0).all() and int(S.min()) >= 32768
    half = U.select_volume("uniform", 65) >> 1
    assert np.array_equal(signed_key_argmin(half)[0], half.astype(np.int64).argmin(-1))


# ---- 3. disparity to depth ----------------------------------------------------------------------------------------------------------------------
def reference_depth(disp, disp_const, near, far):
    """The reference's SCARED rule (data/scared2019/preprocess.py:100-107), restated: fp32 disparities, the constant in fp64."""
    disp = disp.astype(np.float32)
    mask_valid = disp != 0
    depth = np.zeros_like(disp)
    depth[mask_valid] = (np.float64(disp_const) / disp[mask_valid].astype(np.float64)).astype(np.float32)
    depth[depth > far] = 0
    depth[depth < near] = 0
    return depth


def test_disparity_to_depth_is_the_references_rule():
    rng = np.random.default_rng(3)
    disp = rng.uniform(0.5, 40.0, (17, 23)).astype(np.float32)
    disp[rng.uniform(size=disp.shape) < 0.2] = 0
    const, near, far = 96.0, 12.0, 48.0
    disp[0, :4] = [8.0, 2.0, 0.0, 1.0]          # exactly near (kept), exactly far (kept), no match, beyond far
    disp[1, :2] = [np.nextafter(np.float32(8), np.float32(9)), np.nextafter(np.float32(2), np.float32(1))]      # just below near, just above far
    got = DT.disparity_to_depth(disp, const, near, far)
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), reference_depth(disp, const, near, far))
    assert got[0, :4].tolist() == [12.0, 48.0, 0.0, 0.0] and got[1, :2].tolist() == [0.0, 0.0]
    free = DT.disparity_to_depth(disp, 1039.7123)
    assert np.array_equal(free.numpy(), reference_depth(disp, 1039.7123, -np.inf, np.inf))
    assert (free.numpy()[disp == 0] == 0).all() and (free.numpy()[disp > 0] > 0).all()


# ---- 4. closing ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_close_mask_properties(k):
    rng = np.random.default_rng(k)
    mask = torch.from_numpy(rng.uniform(size=(3, 31, 44)) < 0.6)
    closed = DT.close_mask(mask, k)
    assert closed.dtype == torch.bool and closed.shape == mask.shape
    assert bool((closed | ~mask).all())                                   # closed >= mask
    assert torch.equal(DT.close_mask(closed, k), closed)                  # idempotent
    if k == 1:
        assert torch.equal(closed, mask)
    solid = torch.ones(40, 50)
    small, large = solid.clone(), solid.clone()
    if k > 1:
        small[10:10 + k - 1, 20:20 + k - 1] = 0                           # a hole smaller than k is filled
        assert torch.equal(DT.close_mask(small, k), solid)
    large[10:10 + 2 * k, 20:20 + 2 * k] = 0                               # a hole of 2 k is not
    assert torch.equal(DT.close_mask(large, k), large)
    assert DT.close_mask(solid, k).dtype == torch.float32


def test_stereo_depth_on_the_host():
    s = U.scene("slant")
    r = DT.stereo_depth(s["left"], s["right"], U.FOCAL, U.BASELINE, U.SCENE_D, near=20.0, far=200.0)
    assert set(r) == {"disparity", "depth", "valid", "depth_mask", "color_mask"}
    ok = r["depth_mask"].numpy().copy()
    ok[:, :U.SCENE_D] = False
    rel = np.abs(r["depth"].numpy()[ok] - s["depth"][ok]) / s["depth"][ok]
    print(f"\nslant: mean relative depth error {rel.mean():.4%} over {ok.sum()} pixels")
    assert rel.mean() < 0.02
    assert torch.equal(r["color_mask"], DT.close_mask(r["depth_mask"], 1)) and torch.equal(r["depth_mask"], r["depth"] > 0)
    assert torch.equal(r["depth"], DT.disparity_to_depth(r["disparity"], U.FOCAL * U.BASELINE, 20.0, 200.0))


def test_from_stereo_names_the_empty_frame():
    left = np.stack([U.scene("plane")["left"], np.zeros((U.SCENE_H, U.SCENE_W), np.uint8)])
    right = np.stack([U.scene("plane")["right"], np.full((U.SCENE_H, U.SCENE_W), 255, np.uint8)])
    K = np.tile(np.eye(4), (2, 1, 1))
    K[:, 0, 0] = K[:, 1, 1] = U.FOCAL
    with pytest.raises(ValueError, match="frame 1"):
        # (a constant pair matches at disparity 0: no depth anywhere)
        DT.FrameSet.from_stereo(np.stack([left] * 3, -1), np.stack([right] * 3, -1), K, np.tile(np.eye(4), (2, 1, 1)), U.BASELINE,
                                max_disparity=U.SCENE_D, device="cpu")


# ---- 5. refusals of the library's entries (host addresses: never dereferenced, nothing launches) ----------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from endosurf_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


@pytest.fixture()
def buf():
    return np.zeros(64, np.int64)


def entries(lib, b, n=1, H=8, W=8, D=8, dmin=0, p1=7, p2=60, paths=8, uniqueness=10, lr_max=1, size=8, srange=1, null=None, odd=None):
    """Every stereo entry with the given arguments: name -> status.  ``null`` / ``odd`` name one buffer to pass as null / misaligned."""
    a = lambda name: None if name == null else (b.ctypes.data + 1 if name == odd else b.ctypes.data)
    return {
        "es_stereo_census": lambda: lib.es_stereo_census(a("grey"), n, H, W, a("census"), None),
        "es_sgm_cost": lambda: lib.es_sgm_cost(a("census_left"), a("census_right"), n, H, W, D, dmin, a("cost"), None),
        "es_sgm_aggregate": lambda: lib.es_sgm_aggregate(a("cost"), n, H, W, D, p1, p2, paths, a("sums"), None),
        "es_sgm_select": lambda: lib.es_sgm_select(a("sums"), n, H, W, D, dmin, uniqueness, lr_max, 1, a("d0"), a("disparity"), a("flags"),
                                                   a("valid"), a("scratch"), None),
        "es_speckle_label": lambda: lib.es_speckle_label(a("d0"), a("valid"), n, H, W, srange, 1, a("scratch"), a("changed"), None),
        "es_speckle_apply": lambda: lib.es_speckle_apply(n, H, W, size, a("scratch"), a("valid"), a("d0"), a("disparity"), a("flags"), None),
    }


ALL = ("es_stereo_census", "es_sgm_cost", "es_sgm_aggregate", "es_sgm_select", "es_speckle_label", "es_speckle_apply")
WITH_D = ("es_sgm_cost", "es_sgm_aggregate", "es_sgm_select")
REFUSALS = [
    (dict(n=-1), ALL, b"n must not be negative"),
    (dict(H=0), ALL, b"height"), (dict(H=8193), ALL, b"height"), (dict(W=0), ALL, b"width"), (dict(W=8193), ALL, b"width"),
    (dict(D=0), WITH_D, b"max_disparity"), (dict(D=257), WITH_D, b"max_disparity"),
    (dict(n=2, H=4096, W=4096, D=64), WITH_D, b"n H W D"), (dict(n=1, H=4096, W=2048, D=256), WITH_D, b"n H W D"),
    (dict(dmin=-1), ("es_sgm_cost", "es_sgm_select"), b"min_disparity"),
    (dict(dmin=8193), ("es_sgm_cost", "es_sgm_select"), b"min_disparity"), (dict(dmin=2**31 - 1), ("es_sgm_cost", "es_sgm_select"), b"min_disparity"),
    (dict(p1=-1), ("es_sgm_aggregate",), b"p1"), (dict(p1=61), ("es_sgm_aggregate",), b"p1"), (dict(p2=1025), ("es_sgm_aggregate",), b"p2"),
    (dict(paths=5), ("es_sgm_aggregate",), b"paths"), (dict(paths=0), ("es_sgm_aggregate",), b"paths"),
    (dict(uniqueness=-1), ("es_sgm_select",), b"uniqueness"), (dict(uniqueness=101), ("es_sgm_select",), b"uniqueness"),
    (dict(lr_max=-1), ("es_sgm_select",), b"lr_max"),
    (dict(size=-1), ("es_speckle_apply",), b"speckle_size"), (dict(srange=-1), ("es_speckle_label",), b"speckle_range"),
    (dict(null="grey"), ("es_stereo_census",), b"grey"), (dict(null="census"), ("es_stereo_census",), b"census"),
    (dict(odd="census"), ("es_stereo_census",), b"census"),
    (dict(null="census_left"), ("es_sgm_cost",), b"census_left"), (dict(odd="census_right"), ("es_sgm_cost",), b"census_right"),
    (dict(null="cost"), ("es_sgm_cost", "es_sgm_aggregate"), b"cost"),
    (dict(null="sums"), ("es_sgm_aggregate", "es_sgm_select"), b"sums"), (dict(odd="sums"), ("es_sgm_aggregate", "es_sgm_select"), b"sums"),
    (dict(null="d0"), ("es_sgm_select", "es_speckle_label"), b"d0"), (dict(odd="d0"), ("es_sgm_select", "es_speckle_label", "es_speckle_apply"), b"d0"),
    (dict(null="disparity"), ("es_sgm_select",), b"disparity"), (dict(odd="disparity"), ("es_sgm_select", "es_speckle_apply"), b"disparity"),
    (dict(null="flags"), ("es_sgm_select",), b"flags"),
    (dict(null="valid"), ("es_sgm_select", "es_speckle_label", "es_speckle_apply"), b"valid"),
    (dict(null="scratch"), ("es_sgm_select", "es_speckle_label", "es_speckle_apply"), b"scratch"),
    (dict(odd="scratch"), ("es_sgm_select", "es_speckle_label", "es_speckle_apply"), b"scratch"),
    (dict(odd="changed"), ("es_speckle_label",), b"changed"),
]


@pytest.mark.parametrize("args,names,word", REFUSALS, ids=[",".join(f"{k}={v}" for k, v in r[0].items()) for r in REFUSALS])
def test_stereo_entries_refuse_bad_arguments(lib, buf, args, names, word):
    calls = entries(lib, buf, **args)
    for name in names:
        assert calls[name]() == 1, name
        msg = lib.es_last_error()
        assert name.encode() in msg and word in msg, (name, msg)


def test_stereo_entries_accept_an_empty_batch(lib, buf):
    for name, call in entries(lib, buf, n=0).items():
        assert call() == 0, name
    for name, call in entries(lib, buf, n=0, null="scratch").items():          # an empty batch asks nothing of its buffers
        assert call() == 0, name


def test_stereo_scratch_bytes(lib):
    up16 = lambda b: (b + 15) // 16 * 16
    for n, H, W in [(1, 1, 1), (3, 48, 96), (2, 7, 9), (8, 512, 640)]:
        assert lib.es_stereo_scratch_bytes(n, H, W) == 3 * up16(4 * n * H * W)
    assert lib.es_stereo_scratch_bytes(0, 8, 8) == 0 and lib.es_stereo_scratch_bytes(-1, 8, 8) == 0
