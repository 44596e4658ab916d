"""Every deposit route and every tile limit of the deposit log, bit for bit.

On the exact scenes of tests/exact_scenes.py (their exactness is tests/test_exact_scenes_cpu.py's business) every sum of
deposits is exact in any order, so the f64 and f32 grids, all counters and the conservation residual must be the same bits as the
CPU oracle's (f64 walk) and as the atomic route's whichever way the records travel: assert_identical throughout, no tolerance.

A. tile limits: 1, 2, 1024 | 1025 (one pass | two), 4096 | 4097 (level-2 digit 6 | 7 bits), 8192 | 8193 (the hot-tile form ends),
   65536 | 65537 (the log ends: atomics) tiles along z, the upper ones along x and y too, a 128 x 1 x 128 sheet and an 8 x 8 x 16
   block; the route that ran is asserted from last_log_info / last_log_hot_tiles.
B. routes on 3-D scenes: atomic, ample log, >= 4 batches, a log that mostly overflows, 1 - 3 lanes, tail split, small launches,
   shards, the f32 walk.
C. mesh walks, tables in LDS and through the march grid.

Every case prints the route it took past the capture: records, overflow, batches, lanes, hot tiles.  Observed on an MI355X
(DESIGN.md section 5 has the table): hot tiles at 1025 / 4096 / 4097 / 8192 tiles along z 1006 / 797 / 816 / 840 (dyadic) and
1000 / 832 / 829 / 519 (unit); a small budget sends two thirds of the records to the atomic fallback; the whole file takes 8 s.
"""
import numpy as np
import pytest

from oracle import oracle as O
from tests import exact_scenes as E

pytestmark = pytest.mark.gpu

AMPLE = 8 << 30
MAX_LOG_TILES, MAX_HOT_TILES, ONE_PASS_TILES = 65536, 8192, 1024
TALLIES = {"dyadic": ("u64fx", "f64"), "unit": ("u64fx", "f64", "f32")}


def small_budget(dtype):
    """A log budget of 21 (8-byte tallies) / 20 (f32) chunks of 8192 records: less than the chunks the waves of one batch claim."""
    return 4 << 20 if dtype != "f32" else 5 << 19


def say(capsys, text):
    with capsys.disabled():
        print("\n  " + text, end="")


def run(cx, prob, n, dtype, mode="atomic", log_bytes=0, lanes=1, knobs=None, launches=None, config=(0, 0), **kw):
    """One run of `prob` into a fresh tally: ((raw grid, counters), last_log_info or None, hot tiles or None).  `launches`: the
    (photon_offset, count) shards, default one launch of n photons."""
    with cx.tuning(**(knobs or {})):
        prob.apply(cx, dtype); cx.set_tally_mode(mode, log_bytes); cx.set_overlap(lanes); cx.set_launch_config(*config)
        for off, cnt in (launches or ((0, n),)):
            cx.launch(cnt, seed=E.SEED, photon_offset=off, **kw)
        cx.sync()
        if prob.mesh is not None:
            run.marched = bool(cx.mesh_accel_info()["kind"] & 2)      # (read under the knobs that built the tables)
    got = (cx.read_grid_raw(), cx.read_counters())
    info = cx.last_log_info()
    hot = cx.last_log_hot_tiles()[0] if info is not None else None
    return got, info, hot


def check_own_sums(cx, got, what):
    """The GPU's own books: its conservation residual is 0.0 and its absorbed weight is the sum of the grid it reads back."""
    c = got[1]
    assert O.conservation_residual(c) == 0.0, (what, O.conservation_residual(c))
    assert c["w_absorbed"] == cx.read_grid().sum(), what


def restore(*contexts):
    for cx in contexts:
        cx.set_tally_mode("auto", 0); cx.set_overlap(0); cx.set_launch_config(0, 0)


def expected_form(tiles, bits2=None):
    """(passes, bits2, nb1) of a grid of `tiles` tiles as DESIGN.md section 5 tabulates it (0 passes: no log)."""
    if tiles > MAX_LOG_TILES:
        return 0, 0, 0
    b = 0
    if tiles > ONE_PASS_TILES:
        b = 1
        while (1 << (2 * b)) < tiles and b < 7:
            b += 1
    if bits2 is not None:
        b = bits2
    while (tiles >> b) > 1024 and b < 7:
        b += 1
    return (2 if b else 1), b, (-(-tiles // (1 << b)) if b else tiles)


def check_route(info, hot, tiles, what, want_hot=None, overflow=False, lanes=1, bits2=None):
    """The route a limit case took: the log up to 65536 tiles (records, no overflow unless the budget is small), hot tiles on
    two-pass grids of up to 8192 tiles with fewer than 1024 level-1 bins and nowhere else."""
    passes, b, nb1 = expected_form(tiles, bits2)
    if passes == 0:
        assert info is None, (what, info)
        return
    assert info is not None, what
    assert info["records"] > 0 and info["lanes"] == lanes, (what, info)
    if overflow:
        assert info["overflow_records"] > 0, (what, info)
    else:
        assert info["overflow_records"] == 0, (what, info)
    hot_form = passes == 2 and tiles <= MAX_HOT_TILES and nb1 < 1024
    if want_hot is not None:      # log_hot: AT MOST that many -- the tiles at or above a count threshold, and counts tie
        assert (0 < hot <= want_hot) if hot_form and want_hot else hot == 0, (what, hot)
    elif hot_form:
        assert 0 < hot <= 1024 - nb1, (what, hot, nb1)
    else:
        assert hot == 0, (what, hot)


# ---------------------------------------------------------------- A. tile limits
LIMIT_CASES = [(name, kind, dtype) for name in E.LIMIT_ARRANGEMENTS for kind, dtype in (("dyadic", "u64fx"), ("dyadic", "f64"), ("unit", "f32"))]


@pytest.mark.parametrize("name,kind,dtype", LIMIT_CASES, ids=["%s-%s-%s" % c for c in LIMIT_CASES])
def test_tile_limit(ctx, capsys, name, kind, dtype):
    prob, n = E.limit_scene(kind, name)
    tiles = E.n_tiles(prob.grid_shape)
    want = E.oracle_as(dtype, E.oracle_run((kind, name), prob, n))
    try:
        for mode in ("atomic", "log") + (("auto",) if tiles > MAX_LOG_TILES else ()):
            what = "%s %s %s %s" % (name, kind, dtype, mode)
            got, info, hot = run(ctx, prob, n, dtype, mode, AMPLE if mode == "log" else 0)
            say(capsys, "%-34s %6d tiles form %s: %s hot %s" % (what, tiles, expected_form(tiles), info, hot))
            E.assert_identical(got, want, what)
            check_own_sums(ctx, got, what)
            if mode == "atomic":
                assert info is None
            else:
                check_route(info, hot, tiles, what)
    finally:
        restore(ctx)


EXTRA_CASES = [(name, kind, dtype) for name in ("z8192", "z65536", "x65536") for kind, dtype in (("dyadic", "u64fx"), ("dyadic", "f64"), ("unit", "f32"))]


@pytest.mark.parametrize("name,kind,dtype", EXTRA_CASES, ids=["%s-%s-%s" % c for c in EXTRA_CASES])
def test_tile_limit_forced_partitions_budgets_and_lanes(ctx, capsys, name, kind, dtype):
    """At 8192 and 65536 tiles: log_bits2 set so that there are exactly 1024 level-1 bins (3 and 1 -- the latter is raised to 6),
    512 bins + 512 hot tiles (log_bits2 = 4 at 8192), log_hot 0 and 5, a log budget that overflows (on a fresh context: it
    follows an ample one), two and three lanes."""
    import light_transport_amd as lt
    prob, n = E.limit_scene(kind, name)
    tiles = E.n_tiles(prob.grid_shape)
    want = E.oracle_as(dtype, E.oracle_run((kind, name), prob, n))
    full = 3 if tiles == 8192 else 1
    assert expected_form(tiles, full)[2] == 1024
    # (knobs, log budget, lanes, the cap on hot tiles or None = whatever the form gives)
    regimes = [({"log_bits2": full}, AMPLE, 1, 0), ({"log_hot": 0}, AMPLE, 1, 0), ({"log_hot": 5}, AMPLE, 1, 5),
               ({}, small_budget(dtype), 1, None), ({}, AMPLE, 2, None), ({}, AMPLE, 3, None)]
    if tiles == 8192:
        regimes.insert(1, ({"log_bits2": 4}, AMPLE, 1, None))
    c2 = lt.Context(0)
    try:
        ref, info, _ = run(ctx, prob, n, dtype, "atomic")
        assert info is None
        E.assert_identical(ref, want, name + " atomic")
        for knobs, log_bytes, lanes, want_hot in regimes:
            what = "%s %s %s %s budget %d lanes %d" % (name, kind, dtype, knobs, log_bytes, lanes)
            cx = c2 if log_bytes != AMPLE else ctx
            if cx is c2:
                run(c2, prob, n, dtype, "log", AMPLE)      # an ample allocation first: the small budget must be honoured after it
            got, info, hot = run(cx, prob, n, dtype, "log", log_bytes, lanes, knobs)
            say(capsys, "%-60s form %s: %s hot %s" % (what, expected_form(tiles, knobs.get("log_bits2")), info, hot))
            E.assert_identical(got, want, what)
            E.assert_identical(got, ref, what + " against atomic")
            check_own_sums(cx, got, what)
            check_route(info, hot, tiles, what, want_hot, overflow=log_bytes != AMPLE, lanes=lanes, bits2=knobs.get("log_bits2"))
            if knobs.get("log_bits2") == 4:
                assert 0 < hot <= 512, hot
    finally:
        restore(ctx)
        c2.close()


# ---------------------------------------------------------------- B. routes on 3-D scenes
ROUTE_CASES = [(name, dtype) for name in E.ROUTE_SCENES for dtype in TALLIES[name.split("-")[0] if name.startswith("unit") else "dyadic"]]


@pytest.mark.parametrize("name,dtype", ROUTE_CASES, ids=["%s-%s" % c for c in ROUTE_CASES])
def test_routes_are_identical(ctx, capsys, name, dtype):
    """Atomic, ample log, a budget that forces >= 4 batches, a log that mostly overflows, one to three lanes (batches, overflow
    and lanes asserted as test_log_tally_equals_atomic_tally does), the tail split off and forced at thresholds 2 and 16: every
    one identical to the oracle and to the atomic run, counters included."""
    import light_transport_amd as lt
    kind, prob = E.route_scene(name)
    n = E.ROUTE_PHOTONS
    want = E.oracle_as(dtype, E.oracle_run(name, prob, n))
    mid, small = 48 << 20, small_budget(dtype)
    regimes = (("log", AMPLE, 1), ("log", mid, 1), ("log", small, 1), ("log", AMPLE, 2), ("log", AMPLE, 3), ("log", mid, 2))
    c2 = lt.Context(0)
    try:
        ref, info, _ = run(ctx, prob, n, dtype, "atomic")
        assert info is None
        E.assert_identical(ref, want, name + " atomic")
        check_own_sums(ctx, ref, name + " atomic")
        for k, (mode, log_bytes, lanes) in enumerate(regimes):
            cx = ctx if log_bytes == AMPLE else c2       # ample logs on the session context, small budgets on the other
            if cx is c2 and k == 1:
                run(c2, prob, n, dtype, "log", AMPLE)    # ... where an ample allocation is already in place
            what = "%s %s log budget %d lanes %d" % (name, dtype, log_bytes, lanes)
            got, info, hot = run(cx, prob, n, dtype, mode, log_bytes, lanes)
            say(capsys, "%-48s %s" % (what, info))
            E.assert_identical(got, want, what)
            E.assert_identical(got, ref, what + " against atomic")
            check_own_sums(cx, got, what)
            assert info["lanes"] == lanes and info["records"] + info["overflow_records"] >= (n // 2 if kind == "unit" else 5 * n), info
            assert hot == 0
            if log_bytes == AMPLE:
                assert info["overflow_records"] == 0 and info["batches"] <= (2 if lanes == 1 else 12), info      # (+ the pilot)
            if log_bytes == mid:
                assert info["batches"] >= 4, info
            if log_bytes == small:
                assert info["overflow_records"] > info["records"] > 0, info      # most deposits took the atomic fallback
        seen = {}
        for knob in (0, 2, 16):      # off, forced: a wave hands its photons to the tail kernel when at most 2 / 16 are alive
            what = "%s %s tail_split %d" % (name, dtype, knob)
            got, info, _ = run(ctx, prob, n, dtype, "log", 0, 1, dict(tail_split=knob, serial_walks=1), config=(1, 64))
            seen[knob] = info["records"] + info["overflow_records"]
            say(capsys, "%-48s %s" % (what, info))
            E.assert_identical(got, want, what)
            check_own_sums(ctx, got, what)
        # the split was taken: the tail's deposits reach the grid as atomics, not through the log
        # (a unit photon dies at its first interaction: no wave is left with a few long-lived photons to hand over)
        # (measured: threshold 16 moves 0.1 - 0.6 % of the records, threshold 2 a tenth of that -- no more than two identical
        #  launches differ by, since which same-voxel deposits a lane merges depends on scheduling)
        if kind == "dyadic":
            assert seen[16] < seen[2] and seen[16] < 0.9995 * seen[0], seen
    finally:
        restore(ctx)
        c2.close()


@pytest.mark.parametrize("name,dtype", ROUTE_CASES, ids=["%s-%s" % c for c in ROUTE_CASES])
def test_small_launches_and_shards_are_identical(ctx, capsys, name, dtype):
    """700 photons (three workgroups, most log groups unused), 16384 (the largest launch without a pilot batch), and one launch
    against three ragged photon_offset shards accumulated -- atomic and log."""
    kind, prob = E.route_scene(name)
    try:
        for n in (700, 16384):
            want = E.oracle_as(dtype, E.oracle_run(name, prob, n))
            for mode in ("atomic", "log"):
                what = "%s %s %d photons %s" % (name, dtype, n, mode)
                got, info, _ = run(ctx, prob, n, dtype, mode, AMPLE if mode == "log" else 0)
                say(capsys, "%-48s %s" % (what, info))
                E.assert_identical(got, want, what)
                check_own_sums(ctx, got, what)
                assert (info is None) == (mode == "atomic")
                if info is not None:
                    assert info["batches"] == 1 and info["overflow_records"] == 0 and info["records"] > 0, info      # no pilot
        n = E.ROUTE_PHOTONS
        want = E.oracle_as(dtype, E.oracle_run(name, prob, n))
        for mode in ("atomic", "log"):
            what = "%s %s three shards %s" % (name, dtype, mode)
            got, info, _ = run(ctx, prob, n, dtype, mode, 0, launches=E.shards(n))
            E.assert_identical(got, want, what)
            check_own_sums(ctx, got, what)
    finally:
        restore(ctx)


@pytest.mark.parametrize("name,dtype", ROUTE_CASES, ids=["%s-%s" % c for c in ROUTE_CASES])
def test_f32_walk_routes_are_identical(ctx, capsys, name, dtype):
    """The f32 walk's weights are dyadic (unit) too: its routes agree with each other bit for bit, counters included.  Against
    the oracle's f32 restatement the comparison is test_f32_walk_parity's: trajectories agree except where a 1-ulp libm difference
    flips a branch."""
    kind, prob = E.route_scene(name)
    n = E.ROUTE_PHOTONS
    try:
        ref, info, _ = run(ctx, prob, n, dtype, "atomic", f32_walk=True)
        assert info is None
        check_own_sums(ctx, ref, name + " f32 walk atomic")
        for log_bytes, lanes in ((AMPLE, 1), (small_budget(dtype), 1), (AMPLE, 2)):
            what = "%s %s f32 walk log budget %d lanes %d" % (name, dtype, log_bytes, lanes)
            got, info, _ = run(ctx, prob, n, dtype, "log", log_bytes, lanes, f32_walk=True)
            say(capsys, "%-56s %s" % (what, info))
            E.assert_identical(got, ref, what)
            assert info["records"] > 0 and (info["overflow_records"] > 0) == (log_bytes != AMPLE), info
    finally:
        restore(ctx)
    g32, c32 = ref[0].astype(np.float64) * (2.0 ** -40 if dtype == "u64fx" else 1.0), ref[1]
    go32, _, co32 = prob.oracle().run(n, seed=E.SEED, threads=E.ORACLE_THREADS, walk_f32=True)
    assert abs(c32["steps"] - co32["steps"]) / co32["steps"] < 2e-4
    for k in ("w_absorbed", "w_escaped_top", "w_lost_outside_grid"):
        assert abs(c32[k] - co32[k]) / n < 2e-4, k
    assert np.abs(g32 - go32).sum() / go32.sum() < 2e-3


# ---------------------------------------------------------------- C. mesh walks
MESH_CASES = [(name, route, dtype) for name in E.MESH_SCENES for route in ("lds", "march") for dtype in TALLIES[E.MESH_SCENES[name][0]]]


@pytest.mark.parametrize("name,route,dtype", MESH_CASES, ids=["%s-%s-%s" % c for c in MESH_CASES])
def test_mesh_walk_routes_are_identical(ctx, capsys, name, route, dtype):
    """The Cornell cavity with exact media, its tables in LDS and walked through the march grid (force_march): atomic, log, a log
    that overflows and two lanes, identical to each other and to the oracle; mesh_accel_info proves which walk ran."""
    kind, build, n = E.MESH_SCENES[name]
    prob = build()
    want = E.oracle_as(dtype, E.oracle_run(name, prob, n))
    knobs = {"force_march": 1} if route == "march" else {}
    try:
        for mode, log_bytes, lanes in (("atomic", 0, 1), ("log", AMPLE, 1), ("log", small_budget(dtype), 1), ("log", AMPLE, 2)):
            what = "%s %s %s %s budget %d lanes %d" % (name, route, dtype, mode, log_bytes, lanes)
            got, info, _ = run(ctx, prob, n, dtype, mode, log_bytes, lanes, knobs)
            say(capsys, "%-64s %s marched %s" % (what, info, run.marched))
            assert run.marched == (route == "march")
            E.assert_identical(got, want, what)
            check_own_sums(ctx, got, what)
            assert (info is None) == (mode == "atomic")
            if info is not None:
                assert info["lanes"] == lanes and info["records"] > 0, info
                assert (info["overflow_records"] > 0) == (log_bytes != AMPLE), info
    finally:
        restore(ctx)
