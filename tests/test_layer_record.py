"""The slab walk's per-layer step record (LayD, lt_internal.hpp): one LDS record per LAYER holds what a step reads about the
layer it is in -- its medium's constants and its own two bounds -- instead of a layer -> medium index followed by the medium's
record and the bounds table.

GPU tests: the u64 fixed-point tally (2^-40 quantum) against oracle.OracleScene.run bit for bit, and equal photon-step counts,
as in tests/test_gpu_parity.py -- a record indexed by the wrong thing, built from stale tables, or read with the wrong bound
changes trajectories and cannot pass.  The scene: three layers over two media with medium_idx = [1, 0, 1] (layer index and
medium index differ in every layer, two layers share a medium), a middle layer 0.05 thick, indices 1.5 / 1.33 / 1.5 under air,
32^3 voxels of 0.1: photons cross both interfaces often.  CPU test: the host builder's records against the tables they copy.
"""
import functools

import numpy as np
import pytest

from tests import scenes as S

N = 20000
SEED = 41
MEDIA = [(0.3, 12.0, 0.8, 1.33), (0.5, 9.0, 0.9, 1.5)]
OTHER_MEDIA = [(0.6, 7.0, 0.0, 1.33), (0.2, 15.0, 0.7, 1.5)]      # (medium 0 isotropic: the record's g = 0 branch)
Z_BOUNDS = [0.0, 0.15, 0.2, np.inf]
MEDIUM_IDX = [1, 0, 1]


def three_layers(media=MEDIA, source=None):
    n, voxel = 32, 0.1
    half = n * voxel / 2
    return S.Problem(list(media), (n, n, n), (-half, -half, 0.0), (voxel,) * 3,
                     layers=dict(z_bounds=list(Z_BOUNDS), medium_idx=list(MEDIUM_IDX), n_above=1.0, n_below=1.0), source=source)


@functools.lru_cache(maxsize=None)
def oracle_fx(which="first", n=N, seed=SEED):
    """(u64 grid, counters) of the oracle for the three-layer scene: computed once per case, shared, never written to."""
    prob = three_layers(MEDIA if which == "first" else OTHER_MEDIA)
    _, fx, c = prob.oracle().run(n, seed=seed, threads=8, want_fx=True, want_f64=False)
    fx.setflags(write=False)
    return fx, c


def assert_same(fx, c, fxo, co, what="", deposits=True):
    assert c["steps"] == co["steps"], "%s: photon-step counts differ (%d, oracle %d)" % (what, c["steps"], co["steps"])
    diff = int((fx != fxo).sum())
    assert diff == 0, "%s: %d voxels differ in the 2^-40 fixed-point tally" % (what, diff)
    assert fx.sum() > 0 or not deposits


def launch_fx(ctx, n=N, seed=SEED, **kw):
    ctx.launch(n, seed=seed, **kw); ctx.sync()
    return ctx.read_grid_raw(), ctx.read_counters()


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["log", "atomic"])
def test_record_is_indexed_by_layer_not_by_medium(ctx, mode):
    prob = three_layers()
    prob.apply(ctx, "u64fx"); ctx.set_tally_mode(mode)
    fx, c = launch_fx(ctx)
    ctx.set_tally_mode("auto")
    fxo, co = oracle_fx()
    assert_same(fx, c, fxo, co, mode)
    # the scene does what it is for: weight leaves through the top (Fresnel at 1.5 / air) and every layer absorbs
    assert c["w_specular"] > 0 and c["w_escaped_top"] > 0
    assert fx[0].sum() > 0 and fx[1].sum() > 0 and fx[3].sum() > 0      # z in [0, 0.1), [0.1, 0.2) (all three layers), [0.3, 0.4)


@pytest.mark.gpu
def test_records_follow_media_and_layers_in_either_order(ctx):
    prob = three_layers()
    L = prob.layers

    def rest():
        ctx.set_grid(prob.grid_shape, prob.origin, prob.voxel, "u64fx")
        s = prob.source
        ctx.set_source(s["type"], s["pos"], s["dir"], s["extra"], s["start_medium"])
        ctx.set_max_steps(prob.max_steps); ctx.set_tally_quantity("absorbed"); ctx.set_tally_mode("auto")

    # layers first, then the media
    S.slab(n=32, voxel=0.1).apply(ctx, "u64fx")      # (whatever the context held before: another scene)
    ctx.set_layers(L["z_bounds"], L["medium_idx"], L["n_above"], L["n_below"]); ctx.set_media(MEDIA); rest()
    assert_same(*launch_fx(ctx), *oracle_fx("first"), "set_layers, set_media")
    # media first, then the layers
    S.slab(n=32, voxel=0.1).apply(ctx, "u64fx")
    ctx.set_media(MEDIA); ctx.set_layers(L["z_bounds"], L["medium_idx"], L["n_above"], L["n_below"]); rest()
    assert_same(*launch_fx(ctx), *oracle_fx("first"), "set_media, set_layers")
    # the media again, with other coefficients, after both (and after a launch has uploaded the first ones)
    ctx.set_media(OTHER_MEDIA); ctx.zero_tally()
    fxo2, co2 = oracle_fx("other")
    assert_same(*launch_fx(ctx), fxo2, co2, "set_media again")
    assert co2["steps"] != oracle_fx("first")[1]["steps"]      # (the other coefficients are another problem)


@pytest.mark.gpu
def test_tail_split_route(ctx):
    """Bulk kernel (PHASE 1), pool, tail kernel (PHASE 2) on the three-layer scene: tail_split = 1 takes the split where a launch
    has >= 512 photons per launched wave -- one 64-thread workgroup per CU keeps that at 200 000 photons."""
    n = 200000
    prob = three_layers()
    fxo, co = oracle_fx("first", n, SEED)
    seen = {}
    try:
        for knob in (0, 1):
            with ctx.tuning(tail_split=knob, serial_walks=1):
                prob.apply(ctx, "u64fx"); ctx.set_tally_mode("log"); ctx.set_overlap(1); ctx.set_launch_config(1, 64)
                fx, c = launch_fx(ctx, n)
            info = ctx.last_log_info()
            seen[knob] = info["records"] + info["overflow_records"]
            assert_same(fx, c, fxo, co, "tail_split=%d" % knob)
    finally:
        ctx.set_launch_config(0, 0); ctx.set_tally_mode("auto"); ctx.set_overlap(0)
    # the split was taken: the tail's deposits go to the grid as atomics, not through the log
    assert seen[1] < 0.999 * seen[0], seen


@pytest.mark.gpu
def test_table_rng_route(ctx):
    prob = three_layers()
    steps = 80
    tab = np.random.RandomState(3).rand(N, steps, 4)
    prob.apply(ctx, "u64fx")
    fx, c = launch_fx(ctx, rng_table=tab)
    _, fxo, co = prob.oracle().run(N, rng_table=tab, threads=8, want_fx=True, want_f64=False)
    assert_same(fx, c, fxo, co, "table RNG")
    assert c["w_capped"] > 0      # (photons that outlive the table are capped on both sides)


@pytest.mark.gpu
def test_vertex_capture_route(ctx):
    prob = three_layers()
    n, K = N, 8
    prob.apply(ctx, "f64")
    ctx.set_vertex_capture(K)
    try:
        ctx.launch(n, seed=SEED); ctx.sync()
        c = ctx.read_counters()
        v, cnt = ctx.read_vertices(n)
    finally:
        ctx.set_vertex_capture(0)
    _, co, vo, cnto = prob.oracle().run_capture(n, K, seed=SEED)
    assert c["steps"] == co["steps"]
    np.testing.assert_array_equal(cnt, cnto)
    assert cnt.max() == K and cnt.min() >= 1
    rows = np.arange(n)
    for k in (np.zeros(n, dtype=np.int64), cnt.astype(np.int64) - 1):      # the first and the last vertex of every photon
        for f in ("kind", "medium", "step"):
            np.testing.assert_array_equal(v[f][rows, k], vo[f][rows, k])
        np.testing.assert_allclose(v["point"][rows, k], vo["point"][rows, k], rtol=0, atol=1e-10)
        np.testing.assert_allclose(v["direction"][rows, k], vo["direction"][rows, k], rtol=0, atol=1e-11)
        np.testing.assert_allclose(v["throughput"][rows, k], vo["throughput"][rows, k], rtol=1e-12)
        np.testing.assert_allclose(v["pdf_dir"][rows, k], vo["pdf_dir"][rows, k], rtol=1e-9, atol=1e-13)
    assert set(np.unique(v["medium"][rows, cnt.astype(np.int64) - 1])) == {0, 1, 2}      # (the field holds the LAYER of a slab)


@pytest.mark.gpu
def test_f32_walk_log_route_equals_atomic_route(ctx):
    prob = three_layers()
    out = {}
    for mode in ("atomic", "log"):
        prob.apply(ctx, "u64fx"); ctx.set_tally_mode(mode)
        out[mode] = launch_fx(ctx, f32_walk=True)
    ctx.set_tally_mode("auto")
    assert out["log"][1]["steps"] == out["atomic"][1]["steps"]
    assert np.array_equal(out["log"][0], out["atomic"][0]) and out["log"][0].sum() > 0
    # ... and it is the same problem: the f32 walk's totals sit where the f64 oracle's do (5 sigma, sigma < 0.5 per photon)
    co = oracle_fx()[1]
    assert abs(out["log"][1]["w_absorbed"] - co["w_absorbed"]) / N < 5 * 0.5 / np.sqrt(N)


@pytest.mark.gpu
@pytest.mark.parametrize("uz", [1.0, -1.0])
def test_photon_starting_on_an_interface_plane(ctx, uz):
    """pz == zb[1]: the photon belongs to layer 1 (zb[1] <= pz < zb[2]).  Going down its next bound is the record's z_hi, 0.05
    away; going up it is z_lo, at distance 0."""
    src = dict(type=0, pos=(0.0, 0.0, Z_BOUNDS[1]), dir=(0.0, 0.0, uz), extra=(0.0,) * 6, start_medium=0)
    prob = three_layers(source=src)
    for seed in (1, 2, 3):      # one photon per launch
        prob.apply(ctx, "u64fx")
        fx, c = launch_fx(ctx, 1, seed)
        _, fxo, co = prob.oracle().run(1, seed=seed, want_fx=True, want_f64=False)
        assert_same(fx, c, fxo, co, "uz=%g seed=%d" % (uz, seed), deposits=False)      # (a lone photon may leave through the top at once)
    prob.apply(ctx, "f64")
    ctx.set_vertex_capture(4)
    try:
        ctx.launch(1, seed=1); ctx.sync()
        v, cnt = ctx.read_vertices(1)
    finally:
        ctx.set_vertex_capture(0)
    _, _, vo, cnto = prob.oracle().run_capture(1, 4, seed=1)
    assert cnt[0] == cnto[0] and v["medium"][0, 0] == vo["medium"][0, 0] == 1
    np.testing.assert_array_equal(v["medium"][0, :cnt[0]], vo["medium"][0, :cnt[0]])
    np.testing.assert_array_equal(v["step"][0, :cnt[0]], vo["step"][0, :cnt[0]])


# ---------------------------------------------------------------- CPU
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("quantity", [0, 1])
def test_host_records_copy_their_tables_bit_for_bit(f32, quantity):
    """lt_layer_records builds the media table, the bounds and the layer records as a launch does (no device needed): every
    field of every record is the very bits of the MedD / zb value it copies.  A random 8-layer, 4-medium stack."""
    from light_transport_amd import _lib
    rs = np.random.RandomState(11)
    media = [(rs.uniform(0.01, 2.0), rs.uniform(1.0, 30.0), g, rs.uniform(1.0, 1.6)) for g in (0.9, 0.0, -0.3, 0.75)]
    idx = [2, 0, 3, 1, 0, 2, 2, 3]
    zb = np.concatenate([[-0.3], -0.3 + np.cumsum(rs.uniform(0.01, 0.7, size=7)), [np.inf]])
    m, z, r = _lib.layer_records(media, zb, idx, quantity=quantity, f32=f32)
    assert m.shape == (4, 12) and z.shape == (9,) and r.shape == (8, 12) and m.dtype == (np.float32 if f32 else np.float64)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32 if f32 else np.uint64)      # noqa: E731
    MED = dict(mu_t=0, inv_mu_t=1, absorb=2, g=3, n=4, one_m_g2=5, one_p_g2=6, inv_2g=7, dep=8, one_m_g=9, two_g=10)
    REC = dict(mu_t=0, inv_mu_t=1, z_lo=2, z_hi=3, absorb=4, dep=5, two_g=6, one_m_g=7, one_m_g2=8, one_p_g2=9, inv_2g=10, n=11)
    assert np.array_equal(bits(z), bits(zb.astype(m.dtype)))
    for layer, med in enumerate(idx):
        for f, k in REC.items():
            want = z[layer] if f == "z_lo" else (z[layer + 1] if f == "z_hi" else m[med, MED[f]])
            assert bits(r[layer, k:k + 1])[0] == bits(np.array([want], dtype=m.dtype))[0], (layer, f)
    # the table the records copy is the one the walk has always had: one IEEE operation per derived value
    dt = m.dtype.type
    for i, (mu_a, mu_s, g, n) in enumerate(media):
        mu_t = mu_a + mu_s
        gg = dt(g)
        want = [dt(mu_t), dt(1.0 / mu_t), dt(mu_a / mu_t), gg, dt(n), dt(1) - gg * gg, dt(1) + gg * gg,
                dt(1) / (dt(2) * gg) if gg != 0 else dt(0), dt(1.0 / mu_t) if quantity else dt(mu_a / mu_t), dt(1) - gg, dt(2) * gg, dt(0)]
        assert np.array_equal(bits(m[i]), bits(np.array(want, dtype=m.dtype))), i
    # two_g == 0 exactly where g == 0: the walk's isotropic test reads the record's two_g
    assert [rec[REC["two_g"]] == 0 for rec in r] == [media[k][2] == 0 for k in idx]
    with pytest.raises(_lib.LtError):
        _lib.layer_records(media, zb, [0, 1, 2, 3, 4, 0, 0, 0])
