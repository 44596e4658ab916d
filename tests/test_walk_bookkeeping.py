"""The slab walk's wave bookkeeping (lt_walk_kernel.inc, kSlabForm / kLean): the dead-lane mask taken once per iteration and
the loop's exit derived from it, the packet cursor as 32-bit offsets from a 64-bit base, the deposit mask taken on the index
compare, the tile index by 24-bit multiply-adds.  None of it touches a value a photon computes, so every test compares the u64
fixed-point tally (2^-40 quantum) and the photon-step count bit for bit -- with oracle.OracleScene.run unless it says otherwise,
as tests/test_layer_record.py does.  What each test would catch is in its docstring.
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


def small_slab():
    return S.slab(n=32, voxel=0.8)


def sparse_slab(shape):
    """A slab of mean free path 1 (10 voxels of 0.1) and transport length 10, centred in x and y: 20 000 photons deposit in
    voxels a hundred voxels apart, so their records name several 32 x 32 x 16 tiles along every axis that has them."""
    nx, ny, nz = shape
    return S.Problem([(0.1, 1.0, 0.9, 1.0)], shape, (-nx * 0.05, -ny * 0.05, 0.0), (0.1,) * 3,
                     layers=dict(z_bounds=[0.0, np.inf], medium_idx=[0]))


@functools.lru_cache(maxsize=None)
def oracle_small(n, offset=0):
    _, fx, c = small_slab().oracle().run(n, seed=SEED, photon_offset=offset, threads=8, want_fx=True, want_f64=False)
    fx.setflags(write=False)
    return fx, c


def launch(ctx, n, **kw):
    ctx.launch(n, seed=SEED, **kw); ctx.sync()
    return ctx.read_grid_raw(), ctx.read_counters()


def tiles_touched(fx):
    z, y, x = np.nonzero(fx)
    return len(set(zip((z >> 4).tolist(), (y >> 5).tolist(), (x >> 5).tolist())))


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["log", "atomic"])
@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, 255, 257, 1000])
def test_exit_and_refill_with_partial_waves(ctx, n, mode):
    """Fewer photons than kRefillMin dead lanes ever collect, a last packet that is short, waves that never get a photon: the
    launch returns (an exit test that misses `all lanes dead` never does), every photon is walked once (a cursor that skips or
    repeats an id changes the tally and the step count) and the counters account for every photon's weight."""
    small_slab().apply(ctx, "u64fx"); ctx.set_tally_mode(mode)
    fx, c = launch(ctx, n)
    ctx.set_tally_mode("auto")
    LR.assert_same(fx, c, *oracle_small(n), "%d photons, %s" % (n, mode))
    assert c["photons"] == n
    total = sum(c[k] for k in WEIGHTS)
    print("n=%d %s: sum of the weight counters - photons = %.3e" % (n, mode, total - n))
    assert abs(O.conservation_residual(c)) < 1e-9 * n and abs(total - n) < 1e-9 * n


@pytest.mark.gpu
def test_photon_ids_beyond_32_bits(ctx):
    """photon_offset = 2^32 - 500 and 2000 photons: the photon ids cross 2^32 inside one launch.  The cursor counts ids relative
    to the launch (0 ... 1999 here) and the offset is added where a photon is seeded (pid = P.photon_offset + id), so what this
    guards is that sum and everything downstream of it: a pid truncated to 32 bits seeds another photon's stream.  The cursor's
    own 64-bit side -- P.head, nlo and pk_base at or beyond 2^32, a launch of more than 4e9 photons -- is no test's size: it is
    covered by reading (the base and `pk_base + (pk_next + rank)` are 64-bit, the offsets never exceed kPacket)."""
    n, off = 2000, 2 ** 32 - 500
    small_slab().apply(ctx, "u64fx"); ctx.set_tally_mode("log")
    fx, c = launch(ctx, n, photon_offset=off)
    ctx.set_tally_mode("auto")
    fxo, co = oracle_small(n, off)
    LR.assert_same(fx, c, fxo, co, "ids across 2^32")
    assert not np.array_equal(fxo, oracle_small(n)[0])      # (other ids are other photons)


@pytest.mark.gpu
def test_emit_routes_give_one_grid(ctx):
    """The three ways a record leaves the walk: appended to the log, a global atomic, and a log reserved too small (4 MiB for
    ~10^8 records), where most records overflow to atomics on the linear index that emit_deposit rebuilds from the tiled one."""
    n = 300000
    prob = S.slab()
    _, fxo, co = prob.oracle().run(n, seed=SEED, threads=8, want_fx=True, want_f64=False)
    try:
        for mode, log_bytes in (("log", 8 << 30), ("atomic", 0), ("log", 4 << 20)):
            prob.apply(ctx, "u64fx"); ctx.set_tally_mode(mode, log_bytes); ctx.set_overlap(1)
            fx, c = launch(ctx, n)
            info = ctx.last_log_info()
            what = "%s, %d bytes" % (mode, log_bytes)
            if mode == "atomic":
                assert info is None
            elif log_bytes == 8 << 30:
                assert info["overflow_records"] == 0 and info["records"] > 50 * n, info
            else:
                assert info["overflow_records"] > info["records"] > 0, info
            LR.assert_same(fx, c, fxo, co, what)
    finally:
        ctx.set_tally_mode("auto"); ctx.set_overlap(0)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(33, 65, 17), (70, 40, 50), (1024, 32, 16)])
def test_tile_index(ctx, shape):
    """Grids whose dimensions are no multiples of the 32 x 32 x 16 tile, and one with 32 tiles along x: the log's tiled index
    (two 24-bit multiply-adds in the slab walk) against the atomic route's linear one, and both against the oracle on the two
    small grids.  A wrong tile sends a record to another voxel or past the grid."""
    n = 20000
    prob = sparse_slab(shape)
    out = {}
    for mode in ("log", "atomic"):
        prob.apply(ctx, "u64fx"); ctx.set_tally_mode(mode)
        out[mode] = launch(ctx, n)
    ctx.set_tally_mode("auto")
    assert out["log"][1]["steps"] == out["atomic"][1]["steps"]
    assert np.array_equal(out["log"][0], out["atomic"][0]) and out["log"][0].sum() > 0
    n_tiles = tiles_touched(out["log"][0])
    print("grid %s: records in %d tiles" % (shape, n_tiles))
    assert n_tiles >= (8 if shape != (1024, 32, 16) else 16)      # (the oracle's clouds reach 11, 24 and 30 tiles)
    if shape != (1024, 32, 16):
        _, fxo, co = prob.oracle().run(n, seed=SEED, threads=8, want_fx=True, want_f64=False)
        LR.assert_same(*out["log"], fxo, co, "grid %s" % (shape,))


@pytest.mark.gpu
def test_tail_split_leaves_results_unchanged(ctx):
    """One launch that takes the bulk kernel (PHASE 1, which hands its last photons over from the mask of dead lanes) and the
    tail kernel (PHASE 2), against the same launch in one kernel: the set-up and size of test_layer_record.test_tail_split_route.
    The u64 grid and the integer counters are identical.  The eight weight counters are f64 sums of the same addends gathered in
    another order -- per lane, then across the wave, then by atomics whose order differs from run to run -- so two runs of ONE
    route already differ in their last bits; the test runs the unsplit launch twice and prints that spread beside the split's
    difference.  The bound is what reordering can give: the longest chain of additions behind a counter is the ~1500 a lane
    makes (2e7 photon-steps over the 16384 lanes of one 64-thread workgroup per CU) plus the wave's and the atomics', and L
    roundings of 2^-53 relative add up to sqrt(L) 2^-53 = 4e-15 of the counter as a random walk, 1.7e-13 at the very worst:
    1e-13 x max(1, |counter|).  For w_absorbed (1.2e5) that is 1e-8, four orders below the 1e-4 at which a photon's weight goes
    to the roulette: a hand-over that loses or repeats one photon's contribution does not pass.  Seen: split against whole 6e-11, whole against whole 1.5e-10."""
    n = 200000
    prob = LR.three_layers()
    got = {}
    try:
        for run, knob in (("whole", 0), ("again", 0), ("split", 1)):
            with ctx.tuning(tail_split=knob, serial_walks=1):
                prob.apply(ctx, "u64fx"); ctx.set_tally_mode("log"); ctx.set_overlap(1); ctx.set_launch_config(1, 64)
                fx, c = launch(ctx, n)
            info = ctx.last_log_info()
            got[run] = (fx, c, info["records"] + info["overflow_records"])
    finally:
        ctx.set_launch_config(0, 0); ctx.set_tally_mode("auto"); ctx.set_overlap(0)
    (fx0, c0, rec0), (fx1, c1, rec1), c0b = got["whole"], got["split"], got["again"][1]
    assert rec1 < 0.999 * rec0, (rec0, rec1)      # the split was taken: the tail's deposits are atomics, not log records
    assert np.array_equal(fx0, fx1) and fx0.sum() > 0 and np.array_equal(fx0, got["again"][0])
    assert c0["steps"] == c1["steps"] == c0b["steps"] and c0["photons"] == c1["photons"] == n
    for k in WEIGHTS:
        bound = 1e-13 * max(1.0, abs(c0[k]))
        print("%-20s %.17g: split - whole = %.3e, whole again - whole = %.3e, bound %.1e" % (k, c0[k], c1[k] - c0[k], c0b[k] - c0[k], bound))
        assert abs(c0b[k] - c0[k]) <= bound, k
        assert abs(c1[k] - c0[k]) <= bound, k
