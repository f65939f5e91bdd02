"""CPU: the narrow-band scheme (endosurf_amd.meshing.band_field, the numpy twin of csrc/band.hip + Engine.band_field) against the dense
field: marching_tetrahedra of the assembled field must be marching_tetrahedra of the dense field, exactly, while far fewer points are
sampled where the surface is a sheet."""
import numpy as np
import pytest

from endosurf_amd.meshing import band_field, marching_tetrahedra
from iso_util import fields


def axes_for(shape):
    return [np.linspace(-1, 1, n).astype(np.float32) for n in shape]


def lookup(u, axes):
    """A sampler that reads the dense array ``u`` at lattice coordinates (and insists that they are lattice coordinates)."""
    def sample(x):
        idx = [np.searchsorted(a, x[:, k]) for k, a in enumerate(axes)]
        assert all(np.array_equal(a[i], x[:, k]) for k, (a, i) in enumerate(zip(axes, idx)))
        return u[idx[0], idx[1], idx[2]]
    return sample


def run(u, thr=0.0, axes=None, **kw):
    """(stats, block_round, dense mesh, band mesh, field)."""
    axes = axes or axes_for(u.shape)
    f, st, rnd = band_field(lookup(u, axes), axes, thr, return_blocks=True, **kw)
    assert f.shape == u.shape and f.dtype == np.float32
    assert st["dense_points"] == u.size and st["blocks"] == rnd.size and st["seed_blocks"] == int((rnd == 1).sum())
    if not st["fallback"]:
        assert st["active_blocks"] == int((rnd > 0).sum()) and st["rounds"] == max(int(rnd.max()) - 1, 0)
    return st, rnd, marching_tetrahedra(u, thr), marching_tetrahedra(f, thr), f


def assert_same_mesh(dense, band):
    (dv, dt), (bv, bt) = dense, band
    assert dv.shape == bv.shape and np.array_equal(dv, bv, equal_nan=True) and np.array_equal(dt, bt)


# (field, shape, threshold, block, upper bound on evaluated / dense points or None)
CASES = [("sphere", (160, 160, 160), 0.0, 8, 0.5), ("sphere", (160, 160, 160), 0.0, 4, 0.2), ("sphere", (97, 97, 97), 0.1, 16, None),
         ("sphere", (33, 33, 33), 0.2, 4, None), ("sphere", (33, 33, 33), -0.2, 2, None), ("torus", (96, 96, 96), 0.0, 8, 0.5),
         ("two_spheres", (65, 65, 65), 0.0, 8, 0.5), ("two_spheres", (65, 65, 65), 0.0, 5, 0.5), ("gyroid", (96, 80, 72), 0.0, 8, None),
         ("gyroid", (48, 48, 48), 0.2, 6, None), ("plane_on_grid", (20, 12, 70), 0.0, 5, 0.6), ("plane_on_grid", (33, 12, 70), 0.0, 8, 0.5),
         ("sphere", (70, 50, 90), 0.0, 8, 0.5), ("torus", (70, 50, 90), 0.0, 7, None), ("sphere", (9, 17, 130), 0.0, 8, None),
         ("sphere", (9, 17, 130), 0.0, 16, None), ("torus", (9, 17, 130), 0.0, 32, None), ("random", (9, 17, 130), 0.2, 3, None),
         ("sphere", (2, 3, 2), 0.9, 8, None), ("random", (2, 2, 2), 0.1, 2, None)]


@pytest.mark.parametrize("name,shape,thr,block,bound", CASES)
def test_band_mesh_is_the_dense_mesh(name, shape, thr, block, bound):
    u = fields(name, shape, seed=7)
    st, rnd, dense, band, _ = run(u, thr, block=block)
    assert_same_mesh(dense, band)
    assert len(dense[0]) > 0
    coarse = int(np.prod([-(-(n - 1) // block) + 1 for n in shape]))
    assert st["evaluated_points"] <= (1 + 1 / block) ** 3 * st["dense_points"] * 1.5 + coarse
    if bound is not None:
        assert not st["fallback"] and st["evaluated_points"] < bound * st["dense_points"], st
    # without the distance rule (lipschitz = 0) and without the fallback: whole components of the dense mesh, all of them unless the
    # lattice is a thin slab whose block corners all miss the shape (the documented limit)
    st0, _, _, band0, _ = run(u, thr, block=block, lipschitz=0.0, max_fraction=1.0)
    assert not st0["fallback"] and st0["seed_blocks"] <= st["seed_blocks"]
    if min(shape) > block + 1:
        assert_same_mesh(dense, band0)
    else:
        assert {tuple(v) for v in band0[0]} <= {tuple(v) for v in dense[0]}


def test_counts_of_the_sphere_at_160():
    """The figures DESIGN 7a quotes."""
    u = fields("sphere", (160, 160, 160))
    st8 = run(u, block=8)[0]
    st4 = run(u, block=4)[0]
    assert (st8["blocks"], st8["seed_blocks"], st8["active_blocks"], st8["rounds"], st8["evaluated_points"]) == (8000, 866, 866, 0, 640575)
    assert (st4["blocks"], st4["seed_blocks"], st4["evaluated_points"]) == (64000, 3509, 507546)


def test_growth_on_a_random_field():
    u = fields("random", (70, 50, 90), seed=7)
    st, rnd, dense, band, _ = run(u, block=8, lipschitz=0.0, max_fraction=1.0)
    assert not st["fallback"] and st["seed_blocks"] > 0.7 * st["blocks"]
    assert st["active_blocks"] > st["seed_blocks"] and st["rounds"] >= 1 and int(rnd.max()) == st["rounds"] + 1
    assert_same_mesh(dense, band)


def capsule(shape, a, b, radius):
    """Distance (in cells) to the segment a-b minus ``radius``, on the index lattice."""
    p = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij"), -1)
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    s = np.clip(((p - a) @ (b - a)) / ((b - a) @ (b - a)), 0, 1)
    return np.ascontiguousarray(np.linalg.norm(p - a - s[..., None] * (b - a), axis=-1) - radius, np.float32)


def test_growth_follows_a_thin_capsule():
    """Sign changes only (lipschitz = 0): one coarse corner lies inside the capsule, the growth step walks along it."""
    u = capsule((97, 97, 97), (32.3, 32.2, 32.1), (60.5, 37.5, 43.5), 2.3)
    axes = [np.arange(97, dtype=np.float32)] * 3
    st, rnd, dense, band, _ = run(u, axes=axes, block=8, lipschitz=0.0)
    assert st["seed_blocks"] == 8 and st["active_blocks"] > 8 and st["rounds"] >= 3, st
    assert st["evaluated_points"] < 0.03 * st["dense_points"]
    assert len(dense[0]) > 500
    assert_same_mesh(dense, band)
    # the same with the distance rule: more seeds, no growth needed, same mesh
    st1, _, _, band1, _ = run(u, axes=axes, block=8, lipschitz=1.0)
    assert st1["seed_blocks"] > st["active_blocks"] and st1["rounds"] == 0
    assert_same_mesh(dense, band1)


def test_a_violated_lipschitz_bound_is_caught_by_the_growth():
    """A true distance field scaled by 4 with lipschitz = 1: blocks are culled that a 4 times steeper field may cross."""
    for name, shape in (("sphere", (70, 50, 90)), ("torus", (96, 96, 96)), ("two_spheres", (65, 65, 65))):
        u = fields(name, shape) * np.float32(4.0)
        st, _, dense, band, _ = run(u, block=8, lipschitz=1.0)
        assert not st["fallback"]
        assert_same_mesh(dense, band)
        assert st["seed_blocks"] < run(fields(name, shape), block=8, lipschitz=1.0)[0]["seed_blocks"]


def test_the_documented_limit_a_floater_between_the_corners():
    """A sphere of radius 2.5 cells centred on the middle of an 8-cell block: no block corner is inside it."""
    p = np.stack(np.meshgrid(*[np.arange(73, dtype=np.float64)] * 3, indexing="ij"), -1)
    u = np.ascontiguousarray(np.linalg.norm(p - 36.0, axis=-1) - 2.5, np.float32)
    axes = [np.arange(73, dtype=np.float32)] * 3
    st0, _, dense, band0, _ = run(u, axes=axes, block=8, lipschitz=0.0)
    assert len(dense[0]) > 50
    assert st0["seed_blocks"] == 0 and st0["active_blocks"] == 0 and st0["rounds"] == 0 and len(band0[0]) == 0 and len(band0[1]) == 0
    assert st0["evaluated_points"] == 10 ** 3
    st1, _, _, band1, _ = run(u, axes=axes, block=8, lipschitz=1.0)
    assert st1["seed_blocks"] >= 1 and not st1["fallback"]
    assert_same_mesh(dense, band1)


@pytest.mark.parametrize("name,shape", [("gyroid", (96, 80, 72)), ("random", (70, 50, 90))])
def test_fallback_for_space_filling_level_sets(name, shape):
    u = fields(name, shape, seed=7)
    st, _, dense, band, f = run(u, block=8, lipschitz=1.0)
    coarse = int(np.prod([-(-(n - 1) // 8) + 1 for n in shape]))
    assert st["fallback"] is True and st["seed_blocks"] > 0.5 * st["blocks"] and st["active_blocks"] == st["blocks"]
    assert st["evaluated_points"] <= st["dense_points"] + coarse
    assert np.array_equal(f, u)
    assert_same_mesh(dense, band)


def test_nan_corners_and_ties():
    """NaN is outside, a block with a NaN corner is always examined, u == threshold is outside (as in csrc/iso.hip)."""
    u = fields("sphere", (65, 65, 65)).copy()
    u[8, 8, 8] = np.nan                    # a block corner far outside the sphere
    u[20:23, 30:40, 3] = np.nan            # not on the coarse lattice, inside culled blocks: the fill value hides them, like every culled value
    st, rnd, dense, band, f = run(u, block=8)
    assert (rnd[0:2, 0:2, 0:2] == 1).all()          # the 8 blocks around the NaN corner are seeds
    assert np.isnan(f[8, 8, 8]) and not np.isnan(f[21, 35, 3])
    d_ok = ~np.isnan(dense[0]).any(1)
    assert np.array_equal(dense[0][d_ok], band[0][~np.isnan(band[0]).any(1)])          # the sphere's vertices, bit for bit
    # ties: a field that is exactly the threshold on whole planes of lattice points, block faces among them
    for n, block in ((33, 8), (20, 5), (41, 4)):
        u = fields("plane_on_grid", (n, 12, 30))
        for thr in (0.0, 1.0, -2.0, 0.5):
            st, _, dense, band, _ = run(u, thr, block=block)
            assert len(dense[0]) > 0
            assert_same_mesh(dense, band)
    u = fields("ties", (40, 40, 40), seed=7)
    for kw in (dict(block=4), dict(block=8, lipschitz=0.0, max_fraction=1.0)):
        st, _, dense, band, _ = run(u, 0.5, **kw)
        assert_same_mesh(dense, band)


def test_inactive_blocks_hold_their_farthest_corner_value():
    u = fields("sphere", (65, 65, 65))
    st, rnd, _, _, f = run(u, block=8)
    assert rnd[0, 0, 0] == 0 and rnd[3, 3, 3] == 0          # a corner block (outside) and a centre block (inside) are culled
    assert (f[1:8, 1:8, 1:8] == u[0, 0, 0]).all()            # corner 0 of block (0, 0, 0) is the farthest from the level
    assert (f[25:32, 25:32, 25:32] == u[32, 32, 32]).all() and u[32, 32, 32] < 0
    active = np.argwhere(rnd > 0)
    for b in active[:: max(1, len(active) // 20)]:
        sl = tuple(slice(8 * c, 8 * c + 9) for c in b)
        assert np.array_equal(f[sl], u[sl])


def test_bad_arguments():
    u = fields("sphere", (9, 9, 9))
    ax = axes_for(u.shape)
    for block in (1, 33):
        with pytest.raises(ValueError):
            band_field(lookup(u, ax), ax, block=block)
    with pytest.raises(ValueError):
        band_field(lookup(u, ax), [ax[0][:1], ax[1], ax[2]])
