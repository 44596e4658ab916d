"""The slab walk's step without its non-arithmetic vector work (lt_walk_kernel.inc, kDiet: the f64 slab walks): the grid's dimensions
read from LDS and the sign test on the coordinates' high words, one fused product for the deposit with the run-length sum and the
energy bookkeeping taken under the lane mask, the photon-step count on the scalar unit (live lanes per wave-step, less the lanes
handed to the tail kernel, less the capped ones counted in LDS), the interface decision carried as a mask.  None of it touches a
value a photon computes: every case compares the u64 fixed-point tally (2^-40 quantum) and the photon-step count with
oracle.OracleScene.run bit for bit, as tests/test_walk_bookkeeping.py does, and the eight weight counters within 1e-9 n.  Each
scene is first checked on the oracle's result for what it is there to do.  What each test would catch is in its docstring.
"""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import scenes as S
from tests import test_layer_record as LR

SEED = 57
WEIGHTS = ("w_absorbed", "w_lost_outside_grid", "w_escaped_top", "w_escaped_bottom", "w_escaped_mesh", "w_specular",
           "w_roulette_net", "w_capped")
NO_CAP = 1000000
PENCIL = dict(type=0, pos=(0.0, 0.0, 0.0), dir=(0.0, 0.0, 1.0), extra=(0.0,) * 6, start_medium=0)


def corner_grid(shape):
    """A semi-infinite slab of transport length 1 under a grid of 0.1 voxels whose ORIGIN is the beam's entry point: the beam
    runs down the grid's edge x = y = 0, so three quarters of the cloud lie at negative x or y -- coordinates in (-1, 0) voxels,
    which the truncating conversion would put in voxel 0, are as common as any -- and the cloud is wider than 3.3 and deeper
    than 1.7, so weight leaves through the three far faces too."""
    return S.Problem([(0.1, 10.0, 0.9, 1.0)], shape, (0.0, 0.0, 0.0), (0.1,) * 3, layers=dict(z_bounds=[0.0, np.inf], medium_idx=[0]))


# one mean free path is 0.099 in the slab's medium and 0.090 / 0.053 in the two layers': voxels of about one, and of a tenth
DEPOSIT_SCENES = {
    ("slab", "mfp"): lambda **kw: S.slab(n=32, voxel=0.1, **kw), ("slab", "tenth"): lambda **kw: S.slab(n=64, voxel=0.01, **kw),
    ("two_layer", "mfp"): lambda **kw: S.two_layer(n=32, voxel=0.1, **kw), ("two_layer", "tenth"): lambda **kw: S.two_layer(n=64, voxel=0.01, **kw)}

THIN_MEDIA = [(0.3, 12.0, 0.8, 1.33), (0.5, 9.0, 0.9, 1.5)]


def thin_layer(source):
    """Three layers, the middle one ONE voxel thin (0.1, about a mean free path) right under the surface, indices 1.5 / 1.33 / 1.5
    under air: every photon starts within a step of an interface and most of the walk stays there."""
    return S.Problem(list(THIN_MEDIA), (32, 32, 32), (-1.6, -1.6, 0.0), (0.1,) * 3,
                     layers=dict(z_bounds=[0.0, 0.1, 0.2, np.inf], medium_idx=[1, 0, 1], n_above=1.0, n_below=1.0), source=source)


BOUNDARY_SCENES = {
    # uz exactly +1 from the surface: the first hop of every lane is measured against the plane 0.1 below
    "down_from_surface": lambda: thin_layer(dict(PENCIL)),
    # uz exactly -1 from the plane z = 0.1 (the photon is in the middle layer, zb[1] <= pz): dz == 0 at emission, tb = 0 <= s
    "up_from_plane": lambda: thin_layer(dict(PENCIL, pos=(0.0, 0.0, 0.1), dir=(0.0, 0.0, -1.0))),
    # uz == 0 inside a slab 1 thick: no lane is near a plane, whatever its free path, until it has scattered
    "along_x": lambda: S.Problem([(0.1, 10.0, 0.9, 1.4)], (32, 32, 10), (-1.6, -1.6, 0.0), (0.1,) * 3,
                                 layers=dict(z_bounds=[0.0, 1.0], medium_idx=[0], n_above=1.0, n_below=1.0),
                                 source=dict(PENCIL, pos=(0.0, 0.0, 0.5), dir=(1.0, 0.0, 0.0)))}


@functools.lru_cache(maxsize=None)
def oracle_run(kind, key, n, quantity=0, max_steps=NO_CAP, f64=False):
    """(u64 grid, counters[, f64 grid]) of the oracle: computed once per case, shared, never written to."""
    if kind == "corner":
        prob = corner_grid(key)
    elif kind == "deposit":
        prob = DEPOSIT_SCENES[key](max_steps=max_steps)
    elif kind == "boundary":
        prob = BOUNDARY_SCENES[key]()
    else:
        prob = S.slab(n=32, voxel=0.8, max_steps=max_steps)
    o = prob.oracle()
    o.quantity = quantity
    g, fx, c = o.run(n, seed=SEED, threads=8, want_fx=True, want_f64=f64)
    fx.setflags(write=False)
    if f64:
        g.setflags(write=False)
    return (fx, c, g) if f64 else (fx, c)


def launch(ctx, n):
    ctx.launch(n, seed=SEED); ctx.sync()
    return ctx.read_grid_raw(), ctx.read_counters()


def reset(ctx):
    ctx.set_tally_mode("auto"); ctx.set_overlap(0); ctx.set_tuning("tail_split", -1); ctx.set_tally_quantity("absorbed")


def assert_weights(c, co, n, what):
    for k in WEIGHTS:
        assert abs(c[k] - co[k]) <= 1e-9 * n, "%s: %s %.17g, oracle %.17g" % (what, k, c[k], co[k])
    assert c["photons"] == co["photons"] == n


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["log", "atomic"])
@pytest.mark.parametrize("shape", [(33, 31, 17), (17, 33, 31), (31, 17, 33)])
def test_in_grid_test_at_the_grids_corner(ctx, shape, mode):
    """Dimensions that are no multiples of the 32 x 32 x 16 tile, all different, in three orders: a dimension compared with the
    wrong axis, a coordinate in (-1, 0) taken for voxel 0, or a bound off by one puts weight into another voxel (or past the
    grid) and moves w_absorbed against w_lost_outside_grid by whole photon weights."""
    n = 20000
    nx, ny, nz = shape
    fxo, co = oracle_run("corner", shape, n)
    # the scene does what it is for: weight is lost outside, and deposits reach the voxel rows on all six faces of the grid
    assert fxo.shape == (nz, ny, nx) and co["w_lost_outside_grid"] > 0.25 * n and co["w_absorbed"] > 0
    for face in (fxo[0], fxo[-1], fxo[:, 0, :], fxo[:, -1, :], fxo[:, :, 0], fxo[:, :, -1]):
        assert face.sum() > 0
    try:
        corner_grid(shape).apply(ctx, "u64fx"); ctx.set_tally_mode(mode)
        fx, c = launch(ctx, n)
    finally:
        reset(ctx)
    print(shape, mode, "lost outside %.17g (oracle %.17g)" % (c["w_lost_outside_grid"], co["w_lost_outside_grid"]))
    LR.assert_same(fx, c, fxo, co, "grid %s, %s" % (shape, mode))
    assert_weights(c, co, n, "grid %s, %s" % (shape, mode))


@pytest.mark.gpu
@pytest.mark.parametrize("quantity", ["absorbed", "fluence"])
@pytest.mark.parametrize("voxel", ["mfp", "tenth"])
@pytest.mark.parametrize("scene", ["slab", "two_layer"])
def test_deposit_runs(ctx, scene, voxel, quantity):
    """The run-length accumulator with voxels of one mean free path (consecutive deposits often share a voxel: the sum goes onto
    the run) and of a tenth (they rarely do: it goes onto zero and the old run leaves), for both tally quantities -- w absorb and
    w / mu_t are different factors of the same product -- in the log and the atomic build.  u64 tally: bit for bit.  f64 tally,
    the build in which the deposit is ONE fused multiply-add for both cases: against the oracle's f64 grid within
    scenes.assert_grid_close's 1e-9 relative (the same addends summed in another order: at most 10^6 of them per voxel, 10^6 x
    2^-53 = 1e-10); a run that lost or kept a deposit is off by that deposit, 1e-4 of a voxel's sum or more."""
    n = 10000
    q = {"absorbed": 0, "fluence": 1}[quantity]
    fxo, co, go = oracle_run("deposit", (scene, voxel), n, q, NO_CAP, True)
    prob = DEPOSIT_SCENES[(scene, voxel)]()
    nz = fxo.shape[0]
    # the scene does what it is for: deposits in hundreds of voxels, from the first row to the last (both layers of two_layer)
    assert (fxo > 0).sum() > 1000 and fxo[0].sum() > 0 and fxo[nz - 1].sum() > 0 and co["w_absorbed"] > 0
    try:
        for mode in ("log", "atomic"):
            prob.apply(ctx, "u64fx"); ctx.set_tally_quantity(quantity); ctx.set_tally_mode(mode)
            fx, c = launch(ctx, n)
            LR.assert_same(fx, c, fxo, co, "%s %s %s %s" % (scene, voxel, quantity, mode))
            assert_weights(c, co, n, "%s %s %s %s" % (scene, voxel, quantity, mode))
            prob.apply(ctx, "f64"); ctx.set_tally_quantity(quantity); ctx.set_tally_mode(mode)
            ctx.launch(n, seed=SEED); ctx.sync()
            g = ctx.read_grid()
            assert ctx.read_counters()["steps"] == co["steps"]
            d = np.abs(g - go)
            print(scene, voxel, quantity, mode, "f64 tally: max |d| / (1e-12 + 1e-9 E) = %.3g" % float(np.max(d / (1e-12 + 1e-9 * np.abs(go)))))
            S.assert_grid_close(g, go)
    finally:
        reset(ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("quantity", ["absorbed", "fluence"])
@pytest.mark.parametrize("max_steps", [1, 2])
@pytest.mark.parametrize("scene", ["slab", "two_layer"])
def test_deposit_run_of_length_one_leaves_with_the_final_emit(ctx, scene, max_steps, quantity):
    """Step caps 1 and 2: a photon's only (or second) deposit opens a run that no later step closes -- it leaves through the emit
    behind the loop, with the value the one fused product gave it on top of zero."""
    n = 1000
    q = {"absorbed": 0, "fluence": 1}[quantity]
    fxo, co = oracle_run("deposit", (scene, "mfp"), n, q, max_steps)
    assert fxo.sum() > 0 and co["steps"] == max_steps * n and co["w_capped"] > 0
    try:
        for mode in ("log", "atomic"):
            DEPOSIT_SCENES[(scene, "mfp")](max_steps=max_steps).apply(ctx, "u64fx"); ctx.set_tally_quantity(quantity); ctx.set_tally_mode(mode)
            fx, c = launch(ctx, n)
            LR.assert_same(fx, c, fxo, co, "%s cap %d %s %s" % (scene, max_steps, quantity, mode))
            assert_weights(c, co, n, "%s cap %d %s %s" % (scene, max_steps, quantity, mode))
    finally:
        reset(ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("max_steps", [0, 1, 7, NO_CAP])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_step_count_is_exact(ctx, n, max_steps):
    """The step count is the waves' counts of live lanes less the capped photons: partial waves, waves that never get a photon,
    every photon capped at once (cap 0: no step at all), capped after one step and after seven (most photons of this slab live
    longer, a few die sooner), and no cap -- in the log build, the atomic build and the bulk + tail pair (a forced split at a
    threshold of 2: a wave hands its last two photons to the tail kernel, which must not count them twice nor the bulk kernel
    count the step they did not take).  An integer: exact in each."""
    fxo, co = oracle_run("count", None, n, 0, max_steps)
    assert co["steps"] <= max_steps * n and (max_steps > 1 or co["steps"] == max_steps * n)
    try:
        for route in ("log", "atomic", "log_split"):
            S.slab(n=32, voxel=0.8, max_steps=max_steps).apply(ctx, "u64fx")
            ctx.set_tally_mode("atomic" if route == "atomic" else "log"); ctx.set_overlap(1)
            ctx.set_tuning("tail_split", 2 if route == "log_split" else 0)
            fx, c = launch(ctx, n)
            what = "%d photons, cap %d, %s" % (n, max_steps, route)
            print(what, "steps %d" % c["steps"])
            LR.assert_same(fx, c, fxo, co, what, deposits=max_steps > 0)
            assert_weights(c, co, n, what)
    finally:
        reset(ctx)


@pytest.mark.gpu
def test_step_count_with_a_tail_that_takes_over_many_photons(ctx):
    """20 000 photons, the split forced: every wave of the bulk kernel hands over its last photons in mid-walk and the tail kernel
    walks thousands of pool entries on, capped at 300 steps (the mean walk is 283: a third of the photons meet the cap, in the
    bulk kernel or in the tail kernel)."""
    n = 20000
    for max_steps in (300, NO_CAP):
        fxo, co = oracle_run("count", None, n, 0, max_steps)
        assert (co["w_capped"] > 0) == (max_steps == 300)
        try:
            S.slab(n=32, voxel=0.8, max_steps=max_steps).apply(ctx, "u64fx"); ctx.set_tally_mode("log"); ctx.set_overlap(1)
            ctx.set_tuning("tail_split", 2)
            fx, c = launch(ctx, n)
            info = ctx.last_log_info()
        finally:
            reset(ctx)
        print("cap %d: steps %d, w_capped %.17g, log %s" % (max_steps, c["steps"], c["w_capped"], info))
        LR.assert_same(fx, c, fxo, co, "split, cap %d" % max_steps)
        assert_weights(c, co, n, "split, cap %d" % max_steps)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["log", "atomic"])
@pytest.mark.parametrize("scene", ["down_from_surface", "up_from_plane", "along_x"])
def test_interface_decision_as_a_mask(ctx, scene, mode):
    """Whether a hop ends on a plane is a lane mask, set only on lanes within a step of a plane: a lane that crosses without being
    marked, or is marked by a neighbour's quotient, leaves its layer's record behind and changes every later step."""
    n = 20000
    fxo, co = oracle_run("boundary", scene, n)
    # the scenes do what they are for
    if scene == "along_x":      # both planes are reached (after scattering), and the slab absorbs
        assert co["w_escaped_top"] > 0 and co["w_escaped_bottom"] > 0 and co["w_specular"] == 0 and co["w_absorbed"] > 0
    else:                       # all three layers absorb; Fresnel reflection at the surface only for the beam that enters through it
        assert fxo[0].sum() > 0 and fxo[1].sum() > 0 and fxo[2].sum() > 0 and co["w_escaped_top"] > 0
        assert (co["w_specular"] > 0) == (scene == "down_from_surface")
    try:
        BOUNDARY_SCENES[scene]().apply(ctx, "u64fx"); ctx.set_tally_mode(mode)
        fx, c = launch(ctx, n)
    finally:
        reset(ctx)
    LR.assert_same(fx, c, fxo, co, "%s, %s" % (scene, mode))
    assert_weights(c, co, n, "%s, %s" % (scene, mode))
    assert abs(O.conservation_residual(c)) < 1e-9 * n


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["log", "atomic"])
def test_level_beam_in_a_medium_without_interaction(ctx, mode):
    """uz == 0 where mu_t == 0: the free path is infinite and no quotient is taken, and `inf <= inf` has always sent such a photon
    to the plane above it at infinity, where it is reflected at grazing incidence with uz = -0 -- step after step, up to the step
    cap.  It is the one lane that is at a boundary without being near one; a mask taken from the near lanes alone would end it
    as capped in its first step, with no photon-step counted."""
    n, cap = 1000, 7
    prob = S.Problem([(0.0, 0.0, 0.0, 1.4)], (32, 32, 10), (-1.6, -1.6, 0.0), (0.1,) * 3,
                     layers=dict(z_bounds=[0.0, 1.0], medium_idx=[0], n_above=1.0, n_below=1.0),
                     source=dict(PENCIL, pos=(0.0, 0.0, 0.5), dir=(1.0, 0.0, 0.0)), max_steps=cap)
    _, fxo, co = prob.oracle().run(n, seed=SEED, threads=8, want_fx=True, want_f64=False)
    assert co["steps"] == cap * n and co["w_capped"] == n and not fxo.any()
    try:
        prob.apply(ctx, "u64fx"); ctx.set_tally_mode(mode)
        fx, c = launch(ctx, n)
    finally:
        reset(ctx)
    print(mode, "steps %d, w_capped %.17g" % (c["steps"], c["w_capped"]))
    LR.assert_same(fx, c, fxo, co, "level beam in a void, %s" % mode, deposits=False)
    assert_weights(c, co, n, "level beam in a void, %s" % mode)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["hundreds_of_chunks", "log_runs_out"])
def test_log_append_over_many_chunks(ctx, case):
    """The log append behind the leaner step, across chunk claims (the append itself is unchanged: a regression test of the records the
    new deposit hands it).  hundreds_of_chunks: 20 000 photons take 5.7 million steps, four fifths of the weight inside
    the grid, and leave one record per run of same-voxel deposits -- well over a hundred chunks of 8192 (at least a hundred is
    asserted: that is a mean run of five deposits, and at one mean free path per voxel a run is seldom longer than three; seen:
    1 369 631 records, 167 chunks),
    every wave claiming several and appending from record 0 of each.  log_runs_out: a log of one chunk per wave, as in
    tests/test_walk_deposit_route.py -- every wave fills its chunk and meets the exhausted state in mid-walk, after which its
    records are atomics on the linear index.  (Far below 4 GiB of log: the 64-bit side of a chunk's base is covered by reading.)"""
    if case == "hundreds_of_chunks":
        n, log_bytes, prob = 20000, 8 << 30, S.slab(n=64, voxel=0.1)
    else:
        n, log_bytes, prob = 8192, 2 * 64 * 8192 * 12, S.slab(n=64, voxel=0.4, media=((0.01, 10.0, 0.9, 1.0),))
    _, fxo, co = prob.oracle().run(n, seed=SEED, threads=8, want_fx=True, want_f64=False)
    try:
        prob.apply(ctx, "u64fx"); ctx.set_tally_mode("log", log_bytes); ctx.set_overlap(1)
        fx, c = launch(ctx, n)
        info = ctx.last_log_info()
    finally:
        reset(ctx)
    print(case, info)
    if case == "hundreds_of_chunks":
        assert info["overflow_records"] == 0 and info["records"] > 100 * 8192, info
    else:
        assert info["records"] > 0 and info["overflow_records"] > 0 and info["records"] <= 2 * 64 * 8192, info
    LR.assert_same(fx, c, fxo, co, case)
    assert_weights(c, co, n, case)
