"""The conditions that make tests/test_gpu_exact_tally.py meaningful, checked on the CPU oracle alone for every scene that file
uses (tests/exact_scenes.py): the f64 grid is the fixed-point grid times 2^-40 bit for bit, the conservation residual is 0.0,
w_absorbed is the grid's sum; unit scenes hold integers below 2^24; limit scenes fill at least 75 % of their tiles, the first and
the last among them, and stay below 2^63 in fixed point.  Every scene's line -- photons, steps, share of non-empty tiles, hottest
voxel -- is printed past the capture.  To re-check a new exact scene, add it to exact_scenes and run this file.

Coverage as measured here: every limit scene of both families has 100 % of its tiles non-empty; of the 5 voxels in the last
tile of a row or column 1 - 5 are filled, of the 8 x 8 (x 8) in the far-corner tile of the sheet and the block 5 - 16.  The file
takes 20 s on 8 cores."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import exact_scenes as E


def report(capsys, name, kind, prob, n, s):
    with capsys.disabled():
        print("\n  exact scene %-16s %-6s grid %-22s %8d photons %9d steps  %5.1f %% of %6d tiles non-empty (first %d, last %d voxels)"
              "  hottest voxel %.10g" % (name, kind, prob.grid_shape, n, s["steps"], 100 * s["coverage"], E.n_tiles(prob.grid_shape),
                                         s["first"], s["last"], s["hottest"]), end="")


@pytest.mark.parametrize("kind", ["dyadic", "unit"])
@pytest.mark.parametrize("name", list(E.LIMIT_ARRANGEMENTS))
def test_limit_scene_is_exact_and_fills_its_tiles(capsys, name, kind):
    prob, n = E.limit_scene(kind, name)
    nts = E.LIMIT_ARRANGEMENTS[name]
    assert E.n_tiles(prob.grid_shape) == nts[0] * nts[1] * nts[2]
    # the largest readback: 72 MiB, but for the 8 x 8 x 16 block, whose 1024 tiles cannot be had below 93 MiB of 8-byte tally
    assert prob.grid_shape[0] * prob.grid_shape[1] * prob.grid_shape[2] * 8 <= (72 << 20 if name != "xyz8x8x16" else 102 << 20)
    res = E.oracle_run((kind, name), prob, n)
    s = E.check_exact(kind, res, limit=True)
    assert res[2]["photons"] == n and s["steps"] <= 5.2e6
    if kind == "unit":
        E.oracle_as("f32", res)
    report(capsys, name, kind, prob, n, s)


@pytest.mark.parametrize("name", E.ROUTE_SCENES)
def test_route_scene_is_exact(capsys, name):
    """The 3-D scenes at the full launch, at the two small launches the GPU file makes, and as three ragged shards."""
    kind, prob = E.route_scene(name)
    for n in (E.ROUTE_PHOTONS, 700, 16384):
        res = E.oracle_run(name, prob, n)
        s = E.check_exact(kind, res)
        assert res[2]["w_lost_outside_grid"] > 0 or n < E.ROUTE_PHOTONS      # the grid's edges are reached
        if kind == "unit":
            E.oracle_as("f32", res)
        report(capsys, name, kind, prob, n, s)
    whole = E.oracle_run(name, prob, E.ROUTE_PHOTONS)
    fx = np.zeros_like(whole[1])
    steps = 0
    for off, cnt in E.shards(E.ROUTE_PHOTONS):
        part = E.oracle_run(name, prob, cnt, photon_offset=off)
        fx += part[1]; steps += part[2]["steps"]
    assert np.array_equal(fx, whole[1]) and steps == whole[2]["steps"]
    if name.startswith("gap"):      # the clear gap holds nothing, the layers around it do
        z0, z1 = int(round(0.4 / prob.voxel[2])), int(round(0.9 / prob.voxel[2]))
        assert whole[0][z0 + 1:z1 - 1].sum() == 0 and whole[0][:z0].sum() > 0 and whole[0][z1:].sum() > 0


@pytest.mark.parametrize("name", list(E.MESH_SCENES))
def test_mesh_scene_is_exact(capsys, name):
    kind, build, n = E.MESH_SCENES[name]
    prob = build()
    res = E.oracle_run(name, prob, n)
    s = E.check_exact(kind, res, one_step=False)
    assert res[2]["w_escaped_mesh"] > 0
    body = res[0][24:40, 24:40, 24:40].sum()      # the cone's medium absorbs
    assert body > 0
    if kind == "unit":
        E.oracle_as("f32", res)
    report(capsys, name, kind, prob, n, s)


def test_inexact_media_are_told_apart():
    """absorb = 1 / 4 (weights grow powers of 3) and n = 1.4 (specular loss) fail the same conditions: the check can fail."""
    grid = ((40, 40, 40), (-2.0, -2.0, 0.0), (0.1,) * 3)
    quarter = E.dyadic_slab(*grid)
    quarter.media = [(2.5, 7.5, 0.9, 1.0)]
    glass = E.dyadic_slab(*grid)
    glass.media = [(5.0, 5.0, 0.9, 1.4)]
    for prob in (quarter, glass):
        res = prob.oracle().run(20000, seed=E.SEED, threads=E.ORACLE_THREADS, want_fx=True)
        with pytest.raises(AssertionError):
            E.check_exact("dyadic", res)


def test_thin_grid_and_tile_histogram():
    for nts, r in (((1, 1, 1), 5), ((1, 1, 2), 1), ((3, 1, 1), 5), ((1, 4, 1), 7), ((2, 1, 3), 8), ((2, 3, 2), 16)):
        shape, origin, voxel = E.thin_grid(*nts, ragged=r)
        assert E.n_tiles(shape) == nts[0] * nts[1] * nts[2]
        for a in range(3):
            long_ = nts[a] > 1 or (a == 2 and nts == (1, 1, 1))
            assert shape[a] == E.TILE[a] * (nts[a] - 1) + (r if long_ else 1)
            if shape[a] == 1:
                assert origin[a] == -E.WIDE and voxel[a] == 2 * E.WIDE
        # one voxel fewer along a long axis and the tile count drops (r == 1), or the arrangement is the smallest
        if r == 1:
            assert E.n_tiles((shape[0], shape[1], shape[2] - 1)) < E.n_tiles(shape)
    rs = np.random.RandomState(4)
    g = (rs.rand(37, 70, 45) < 0.02) * rs.rand(37, 70, 45)
    h = E.tile_histogram(g)
    assert h.shape == (3, 3, 2) and h.sum() == (g != 0).sum()
    for tz in range(3):
        for ty in range(3):
            for tx in range(2):
                assert h[tz, ty, tx] == (g[16 * tz:16 * tz + 16, 32 * ty:32 * ty + 32, 32 * tx:32 * tx + 32] != 0).sum()


@pytest.mark.parametrize("dtype", ["u64fx", "f64", "f32"])
def test_assert_identical_notices_one_unit_and_one_last_bit(dtype):
    """One unit added to, removed from or moved out of one voxel of the LAST tile, a zero that changed sign, and a last-bit change
    of one counter: each alone fails assert_identical, and nothing else does -- so a deliberately wrong grid passes only where a
    regime's assertion is missing."""
    prob, n = E.limit_scene("unit", "z1025")
    want = E.oracle_as(dtype, E.oracle_run(("unit", "z1025"), prob, n))
    grid, cnt = want
    E.assert_identical((grid.copy(), dict(cnt)), want)
    last = np.flatnonzero(grid.reshape(-1))[-1]
    assert last >= 16 * 1024      # in the last tile
    empty = np.flatnonzero(grid.reshape(-1) == 0)[-1]      # the deepest voxel that holds nothing
    one = np.uint64(1) if dtype == "u64fx" else grid.dtype.type(1)      # one unit of the raw type: 2^-40 / one photon
    mutations = []
    for what in ("added", "removed", "moved", "moved into another tile"):
        g = grid.copy()
        f = g.reshape(-1)
        if what == "added":
            f[last] += one
        elif what == "removed":
            f[last] -= one
        elif what == "moved":
            f[last] -= one; f[empty] += one
        else:
            f[last] -= one; f[3] += one
        assert g.sum() != grid.sum() or what.startswith("moved")
        mutations.append((what, g, dict(cnt)))
    if dtype != "u64fx":
        g = grid.copy()
        g.reshape(-1)[empty] = -0.0
        mutations.append(("a negative zero", g, dict(cnt)))
    for key in ("w_absorbed", "w_lost_outside_grid"):
        c = dict(cnt)
        c[key] = float(np.nextafter(np.float64(c[key]), np.inf))
        mutations.append(("the last bit of " + key, grid.copy(), c))
    for key in ("steps", "photons"):
        c = dict(cnt)
        c[key] += 1
        mutations.append((key, grid.copy(), c))
    for what, g, c in mutations:
        with pytest.raises(AssertionError):
            E.assert_identical((g, c), want, what)
    with pytest.raises(AssertionError):      # another type is never identical
        E.assert_identical((grid.astype(np.float64) if dtype != "f64" else grid.astype(np.float32), dict(cnt)), want)
    assert O.conservation_residual(cnt) == 0.0
