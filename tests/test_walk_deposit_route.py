"""The slab walk's deposit route as a build (walk_kernel's ROUTE: log or atomic, chosen by launch_walk from the batch's log), the
log append's single room test with the exhausted state behind it, and the step cap at every size down to none.  None of it
touches a value a photon computes: every case compares the u64 fixed-point tally (2^-40 quantum) and the photon-step count
with oracle.OracleScene.run bit for bit, as tests/test_walk_bookkeeping.py does.
"""
import functools

import pytest

from oracle import oracle as O
from tests import scenes as S
from tests import test_layer_record as LR

SEED = 57
WEIGHTS = ("w_absorbed", "w_lost_outside_grid", "w_escaped_top", "w_escaped_bottom", "w_escaped_mesh", "w_specular",
           "w_roulette_net", "w_capped")
SCENES = {"slab": lambda **kw: S.slab(n=32, voxel=0.8, **kw), "two_layer": lambda **kw: S.two_layer(n=32, **kw),
          # (a tenth of the absorption: walks ten times as long, for the log that is to run out)
          "long_walks": lambda **kw: S.slab(n=64, voxel=0.4, media=((0.01, 10.0, 0.9, 1.0),), **kw)}


@functools.lru_cache(maxsize=None)
def oracle_of(scene, n, max_steps=1000000):
    """(u64 grid, counters) of the oracle: computed once per case, shared, never written to."""
    _, fx, c = SCENES[scene](max_steps=max_steps).oracle().run(n, seed=SEED, threads=8, want_fx=True, want_f64=False)
    fx.setflags(write=False)
    return fx, c


def launch(ctx, n):
    ctx.launch(n, seed=SEED); ctx.sync()
    return ctx.read_grid_raw(), ctx.read_counters()


def reset(ctx):
    ctx.set_tally_mode("auto"); ctx.set_overlap(0); ctx.set_tuning("tail_split", -1)


def sum_bound(n):
    """Two f64 sums of the same n addends, each at most 1, taken in different orders: every partial sum is at most n, so each of
    the n additions rounds by at most n 2^-53, on either side."""
    return 2.0 * n * n * 2.0 ** -53


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("route", ["log", "atomic", "log_split"])
@pytest.mark.parametrize("scene", ["slab", "two_layer"])
def test_route_and_phase(ctx, scene, route):
    """The log build (PHASE 0), the atomic build (PHASE 0), and the bulk kernel (PHASE 1, log) with the tail kernel (PHASE 2,
    atomic only) behind it: one grid, the oracle's.  last_log_info says which route ran."""
    n = 20000
    prob = SCENES[scene]()
    fxo, co = oracle_of(scene, n)
    try:
        prob.apply(ctx, "u64fx"); ctx.set_tally_mode("atomic" if route == "atomic" else "log"); ctx.set_overlap(1)
        if route == "log_split":
            ctx.set_tuning("tail_split", 2)      # forces the split whatever the batch's size; a wave hands over its last 2 photons
        fx, c = launch(ctx, n)
        info = ctx.last_log_info()
        print(scene, route, info)
        LR.assert_same(fx, c, fxo, co, "%s, %s" % (scene, route))
        assert c["photons"] == n and abs(O.conservation_residual(c)) < 1e-9 * n
        if route == "atomic":
            assert info is None
        else:
            assert info["records"] > 0 and info["overflow_records"] == 0, info
        if route == "log_split":      # the tail ran: its deposits went to the grid as atomics, not through the log
            ctx.set_tuning("tail_split", 0)
            prob.apply(ctx, "u64fx")
            fx0, c0 = launch(ctx, n)
            whole = ctx.last_log_info()
            print(scene, "unsplit", whole)
            LR.assert_same(fx0, c0, fxo, co, "%s, unsplit" % scene)
            assert info["records"] < whole["records"], (info, whole)
    finally:
        reset(ctx)


@pytest.mark.gpu
def test_exhausted_log(ctx):
    """A log too small for its batch: every wave claims a chunk, fills it, and meets the exhausted state in mid-walk; from there
    its records go to the grid as atomics on the linear index rebuilt from the tiled one.  The size: a launch under such a
    reservation runs in batches of 4096 photons -- 16 workgroups, 64 waves of 64 photons, four waves to each of the 16 chunk
    groups -- and 12 MiB (64 chunks x 8192 records x 12 B, twice: the log and the partition's copy) is one chunk per wave.  The
    scene absorbs a tenth of what the others do, so its walks are long: 148 records per photon, 9 500 per wave against the
    chunk's 8192 (seen: 1 000 163 records in the log, 95 % of the two batches' chunks, 210 382 to atomics).  Run twice on one
    context: a wave's exhausted state is its own and ends with it."""
    n, log_bytes = 8192, 2 * 64 * 8192 * 12
    prob = SCENES["long_walks"]()
    fxo, co = oracle_of("long_walks", n)
    try:
        for run in (0, 1):
            prob.apply(ctx, "u64fx"); ctx.set_tally_mode("log", log_bytes); ctx.set_overlap(1)
            fx, c = launch(ctx, n)
            info = ctx.last_log_info()
            print("run %d:" % run, info)
            assert info["records"] > 0 and info["overflow_records"] > 0, info
            assert info["records"] <= 2 * 64 * 8192      # (two batches, 64 chunks each)
            LR.assert_same(fx, c, fxo, co, "exhausted log, run %d" % run)
    finally:
        reset(ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["log", "atomic"])
@pytest.mark.parametrize("max_steps", [0, 1, 2, 7])
def test_step_cap(ctx, max_steps, route):
    """A photon alive after max_steps steps is capped with the weight it has then -- after an interaction, after crossing or
    reflecting at the interface 0.1 below the surface, or as emitted when the cap is 0 -- and takes no further step, in the log
    build and in the atomic build."""
    n = 1000
    prob = SCENES["two_layer"](max_steps=max_steps)
    fxo, co = oracle_of("two_layer", n, max_steps)
    try:
        prob.apply(ctx, "u64fx"); ctx.set_tally_mode(route); ctx.set_overlap(1)
        fx, c = launch(ctx, n)
        print(max_steps, route, "steps %d, w_capped %.17g (oracle %.17g), specular %.17g" % (c["steps"], c["w_capped"], co["w_capped"], c["w_specular"]))
        LR.assert_same(fx, c, fxo, co, "max_steps %d, %s" % (max_steps, route), deposits=max_steps > 0)
        assert abs(c["w_capped"] - co["w_capped"]) <= sum_bound(n) and co["w_capped"] > 0
        assert abs(O.conservation_residual(c)) < 1e-9 * n and abs(O.conservation_residual(co)) < 1e-9 * n
        assert c["steps"] <= max_steps * n
        if max_steps == 0:
            assert c["steps"] == 0 and fx.sum() == 0
            assert c["w_specular"] > 0 and abs(c["w_capped"] - (n - c["w_specular"])) <= sum_bound(n)
    finally:
        reset(ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 65])
def test_tail_kernel_with_empty_and_partial_waves(ctx, n):
    """Fewer photons than a wave has lanes, and one more: with the split forced at a threshold of 2 the bulk kernel hands nearly
    every photon's last stretch to the tail kernel, most of whose waves find no pool entry and some a few.  The launch returns
    and the counters account for every photon."""
    fxo, co = oracle_of("slab", n)
    try:
        SCENES["slab"]().apply(ctx, "u64fx"); ctx.set_tally_mode("log"); ctx.set_overlap(1); ctx.set_tuning("tail_split", 2)
        fx, c = launch(ctx, n)
        info = ctx.last_log_info()
        print(n, info)
        LR.assert_same(fx, c, fxo, co, "%d photons, split" % n)
        assert c["photons"] == n
        total = sum(c[k] for k in WEIGHTS)
        assert abs(O.conservation_residual(c)) < 1e-9 * n and abs(total - n) < 1e-9 * n
        if n == 1:      # (its wave hands the photon over before its first step: the whole walk ran in the tail kernel)
            assert info["records"] == 0 and info["overflow_records"] == 0 and c["steps"] > 0, info
    finally:
        reset(ctx)

