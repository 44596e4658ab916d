"""GPU suite (-m gpu): the HIP path, called through the C ABI, against (a) the
golden vectors captured from the reference's own functions and (b) the CPU
oracle on the same seeded inputs.

Tolerances.  Integer / index / decision results: exact.  Float64 results: the
kernels fuse multiply-adds and use the device libm, the oracle does neither, so
values agree to a few ulp per operation: per-voxel |d| <= 1e-12 + 1e-9 * E
 with ZERO voxels allowed outside; with the u64
fixed-point tally (2^-40 quantum) the grids are compared bit for bit.
The f32 walk is compared statistically (3-sigma on totals).
"""
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import scenes as S
from tests.test_oracle_golden import check_triangle_hits

pytestmark = pytest.mark.gpu


def load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name))


# ---------------------------------------------------------------- library
def test_extension_is_loaded_and_device_is_mi355x(ctx):
    import light_transport_amd as lt
    info = ctx.device_info()
    assert "gfx950" in info["name"] and info["cus"] >= 200
    assert os.path.samefile(lt.lib()._name, lt.LIB_PATH)


def test_xorwow_matches_rocrand_device_generator(ctx):
    c = 0x9E3779B97F4A7C15       # (seed + k c, id - k): the pairs a single-stage hash would have aliased
    for seed, pid in ((0, 0), (42, 1), (2 ** 63 + 5, 10 ** 12 + 7), (7, 2 ** 40), (5, 10), ((5 + c) % 2 ** 64, 9)):
        np.testing.assert_array_equal(ctx.rng_raw(seed, pid, 257), O.rng_raw(seed, pid, 257))


# ---------------------------------------------------------------- reference functions (G1-G6)
def test_g1_henyey_greenstein(ctx, golden_dir):
    g1 = load(golden_dir, "g1_henyey_greenstein.npz")
    from light_transport_amd.src.medium_samples import henyey_greenstein, sample_henyey_greenstein
    for gi, g in enumerate(g1["g"]):
        np.testing.assert_allclose(henyey_greenstein(g1["cos_theta"], g, ctx), g1["value"][gi], rtol=1e-14)
    xi = (np.arange(20000) + 0.5) / 20000
    for g in (-0.7, 0.0, 0.9):
        c = sample_henyey_greenstein(xi, g, ctx)
        np.testing.assert_allclose(c, O.eval_fn("HG_SAMPLE", np.stack([xi, np.full_like(xi, g)], 1))[:, 0], atol=4e-15)
        assert abs(c.mean() - g) < 1e-3


def test_g2_triangle_intersect(ctx, golden_dir):
    g2 = load(golden_dir, "g2_triangle_intersect.npz")
    check_triangle_hits(ctx.triangle_intersect(g2["origins"], g2["dirs"], g2["tris"]), g2)


def test_g3_intersect_bounds(ctx, golden_dir):
    g3 = load(golden_dir, "g3_intersect_bounds.npz")
    boxes = np.concatenate([g3["lo"], g3["hi"]], axis=1)
    hit = ctx.intersect_bounds(g3["origins"], g3["dirs"], boxes, g3["tmax"])
    # decisions are exact: the slab test is (bound - origin) * inv_dir, compares and one widening product --
    # nothing a fused multiply-add could change
    bad = np.flatnonzero(hit != g3["hit"])
    assert len(bad) == 0, "intersect_bounds differs from the reference on rays %s" % bad[:10]


def test_g4_nearest_hit(ctx, golden_dir):
    g4 = load(golden_dir, "g4_scene_nearest_hit.npz")
    from light_transport_amd.src import bvh_new as B
    ordered, linear = S.cornell_scene()
    verts = B.triangles_array(ordered)
    key = {tuple(np.round(v.ravel(), 9)): i for i, v in enumerate(g4["verts"])}
    back = np.array([key[tuple(np.round(v.ravel(), 9))] for v in verts])
    for use_bvh in (True, False, 4):        # 4: the BVH front to back (near child first, bvh_new.py:455-458), the renderers' order
        prim, t = B.intersect_bvh_batch(g4["origins"], g4["dirs"], ordered, linear, g4["tmax"], use_bvh, ctx)
        got = np.where(prim >= 0, back[np.maximum(prim, 0)], -1)
        np.testing.assert_array_equal(got, g4["prim"])
        np.testing.assert_allclose(t, g4["t"], rtol=1e-12)
    # scalar, reference-signature wrappers
    from light_transport_amd.src.rays import Ray
    from light_transport_amd.src.utils import hit_object
    for i in (0, 1, 2, 3):
        ray = Ray(np.append(g4["origins"][i], 1.0), np.append(g4["dirs"][i], 0.0)); ray.tmax = g4["tmax"][i]
        obj, dist_, point, normal = hit_object(ordered, linear, ray)
        if g4["prim"][i] < 0:
            assert obj is None
        else:
            assert obj is ordered[int(np.flatnonzero(back == g4["prim"][i])[0])]
            assert abs(dist_ - g4["t"][i]) < 1e-11 and normal.shape == (4,)


def test_g5_sampling_frames(ctx, golden_dir):
    g5 = load(golden_dir, "g5_sampling.npz")
    np.testing.assert_allclose(ctx.eval("ONB", g5["normals"]), g5["onb"], rtol=0, atol=4e-16)
    np.testing.assert_allclose(ctx.eval("DISK", g5["u"]), g5["disk"], rtol=0, atol=1e-15)
    hemi = ctx.eval("COSINE_HEMI", np.concatenate([g5["normals"], g5["incoming"], g5["u"]], axis=1))
    # z = sqrt(1 - d0^2 - d1^2) is a cancellation on the disk rim: a fused multiply-add moves it by
    # ~sqrt(eps) there (u = (0,0) maps exactly onto the rim); everywhere else agreement is at the ulp level
    rim = np.abs(g5["cosine_hemi"][:, 3]) * np.pi < 1e-3
    assert rim.sum() < 10
    np.testing.assert_allclose(hemi[~rim], g5["cosine_hemi"][~rim], rtol=0, atol=1e-13)
    np.testing.assert_allclose(hemi[rim], g5["cosine_hemi"][rim], rtol=0, atol=1e-7)
    refl = ctx.eval("REFLECT", np.concatenate([g5["incoming"], g5["normals"]], axis=1))
    np.testing.assert_allclose(refl, g5["reflected"], rtol=0, atol=1e-15)
    from light_transport_amd.src.utils import create_orthonormal_system, cosine_weighted_hemisphere_sampling
    from light_transport_amd.src.brdf import get_reflected_direction
    v2, v3 = create_orthonormal_system(np.append(g5["normals"][9], 0.0), ctx)
    np.testing.assert_allclose(np.concatenate([v2, v3]), g5["onb"][9], atol=4e-16)
    d, pdf = cosine_weighted_hemisphere_sampling(np.append(g5["normals"][9], 0.0), np.append(g5["incoming"][9], 0.0),
                                                 list(g5["u"][9]), ctx)
    np.testing.assert_allclose(np.append(d[:3], pdf), g5["cosine_hemi"][9], atol=2e-15)
    r = get_reflected_direction(np.append(g5["incoming"][9], 0.0), np.append(g5["normals"][9], 0.0), ctx)
    np.testing.assert_allclose(r[:3], g5["reflected"][9], atol=1e-15)


def test_boundary_and_spin_match_oracle(ctx):
    rs = np.random.RandomState(5)
    n = 5000
    d = rs.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    nf = rs.normal(size=(n, 3)); nf /= np.linalg.norm(nf, axis=1, keepdims=True)
    nf *= -np.sign(np.einsum("ij,ij->i", d, nf))[:, None]
    n1 = rs.choice([1.0, 1.33, 1.4, 1.5], size=n); n2 = rs.choice([1.0, 1.33, 1.4, 1.5], size=n)
    inp = np.concatenate([d, nf, n1[:, None], n2[:, None]], axis=1)
    a, b = ctx.eval("BOUNDARY", inp), O.eval_fn("BOUNDARY", inp)
    np.testing.assert_allclose(a, b, rtol=0, atol=3e-14)
    assert (b[:, 0] == 1).sum() > 100 and (b[:, 0] == 0).sum() > 500   # TIR and index-matched both covered
    u = rs.normal(size=(n, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    u[:50] = [0, 0, 1]; u[50:100] = [0, 0, -1]
    inp = np.concatenate([u, rs.uniform(-1, 1, size=(n, 1)), rs.rand(n, 1)], axis=1)
    a, b = ctx.eval("SPIN", inp), O.eval_fn("SPIN", inp)
    np.testing.assert_allclose(a, b, rtol=0, atol=2e-14)
    np.testing.assert_allclose(np.linalg.norm(a, axis=1), 1.0, atol=1e-5)   # 0.99999 branch is approximate by design


def test_walk_math_primitives(ctx):
    """The walk's lean f64 -ln, sin/cos(2 pi x), sqrt and quotient (restricted ranges) against the host libm."""
    rs = np.random.RandomState(2)
    x = np.concatenate([rs.rand(200000), 2.0 ** -np.arange(1, 54), 1 - 2.0 ** -np.arange(1, 54), [1.0, 0.5, 0.25, 0.75,
                        0.125, 0.70710678118654752, 0.7071067811865476, 2.0 ** -53]])
    x = x[x > 0]
    out = ctx.eval("WALK_MATH", x[:, None])
    ref = -np.log(x)
    assert np.all(np.abs(out[:, 0] - ref) <= 4e-16 * np.maximum(np.abs(ref), 2.0 ** -53)), "neg_log"
    assert out[x == 1.0, 0].max() == 0.0
    # reference in x87 extended precision: in double, 2*pi*x alone carries up to 7e-16 of angle error
    two_pi = 2 * np.longdouble("3.14159265358979323846264338327950288")
    ang = two_pi * x.astype(np.longdouble)
    np.testing.assert_allclose(out[:, 1], np.sin(ang).astype(np.float64), rtol=0, atol=3e-16)
    np.testing.assert_allclose(out[:, 2], np.cos(ang).astype(np.float64), rtol=0, atol=3e-16)
    np.testing.assert_allclose(out[:, 1] ** 2 + out[:, 2] ** 2, 1.0, rtol=0, atol=5e-16)
    np.testing.assert_allclose(out[:, 3], np.sqrt(x), rtol=3e-16, atol=0)
    np.testing.assert_allclose(out[:, 4], 1.0 / (1.0 + x), rtol=3e-16, atol=0)
    z = ctx.eval("WALK_MATH", np.array([[1.0]]))   # exact corners used by the walk
    assert z[0, 1] == 0.0 or abs(z[0, 1]) < 1e-300 or abs(z[0, 1]) < 3e-16
    assert abs(z[0, 2] - 1.0) < 3e-16 and z[0, 3] == 1.0


def test_walk_math_from_raw_draws(ctx):
    """The forms the f64 XORWOW walk applies to a RAW 32-bit draw k (u = (k + 1) 2^-32: exponent, table cell and remainder by
    integer shifts) against the host libm and against the double-argument forms of the same tables."""
    rs = np.random.RandomState(3)
    k = np.concatenate([rs.randint(0, 2 ** 32, size=200000, dtype=np.uint64), 2 ** np.arange(0, 32, dtype=np.uint64) - 1,
                        2 ** np.arange(1, 33, dtype=np.uint64) - 2, [0, 1, 2, 2 ** 32 - 1, 2 ** 31, 2 ** 31 - 1, 3 * 2 ** 30 - 1, 3 * 2 ** 30,
                                                                      2 ** 26 - 1, 2 ** 25 - 1, 2 ** 25]]).astype(np.float64)
    u = (k + 1.0) * 2.0 ** -32                          # exact
    out = ctx.eval("WALK_MATH_RAW", k[:, None])
    ref = -np.log(u)
    assert np.all(np.abs(out[:, 0] - ref) <= 4e-16 * np.maximum(np.abs(ref), 2.0 ** -53)), "neg_log_raw"
    assert out[u == 1.0, 0].max() == 0.0
    two_pi = 2 * np.longdouble("3.14159265358979323846264338327950288")
    ang = two_pi * u.astype(np.longdouble)
    np.testing.assert_allclose(out[:, 1], np.sin(ang).astype(np.float64), rtol=0, atol=3e-16)
    np.testing.assert_allclose(out[:, 2], np.cos(ang).astype(np.float64), rtol=0, atol=3e-16)
    dbl = ctx.eval("WALK_MATH", u[:, None])
    np.testing.assert_allclose(out[:, 0], dbl[:, 0], rtol=3e-16, atol=1e-300)
    np.testing.assert_allclose(out[:, 1:3], dbl[:, 1:3], rtol=0, atol=2e-16)


# ---------------------------------------------------------------- the walk vs the oracle
def run_gpu(ctx, prob, n, dtype="f64", **kw):
    prob.apply(ctx, dtype)
    ctx.launch(n, **kw)
    ctx.sync()
    return ctx.read_grid(), ctx.read_counters()


def check_counters(c, co, n, rtol=1e-10):
    assert c["photons"] == co["photons"] == n
    assert c["steps"] == co["steps"], "photon-step counts differ: some trajectory diverged"
    for k in c:
        if k.startswith("w_"):
            assert abs(c[k] - co[k]) <= rtol * n + 1e-12, (k, c[k], co[k])
    assert abs(O.conservation_residual(c)) < 1e-10 * n


def test_c1_table_rng_parity(ctx):
    """Config 1 in the reference's RNG mechanism: identical uniform tables on both sides."""
    prob = S.slab()   # 64^3, voxel 0.4
    n, steps = 10000, 120
    tab = np.random.RandomState(0).rand(n, steps, 4)
    g, c = run_gpu(ctx, prob, n, rng_table=tab)
    go, _, co = prob.oracle().run(n, rng_table=tab, threads=8)
    check_counters(c, co, n)
    assert c["w_capped"] > 0    # photons outliving the 120-step table are capped, with their weight conserved
    S.assert_grid_close(g, go)


def test_c1_xorwow_parity_f64(ctx):
    prob = S.slab()
    n = 10000
    g, c = run_gpu(ctx, prob, n, seed=0)
    go, _, co = prob.oracle().run(n, seed=0, threads=8)
    check_counters(c, co, n)
    S.assert_grid_close(g, go)
    assert abs(g.sum() - c["w_absorbed"]) < 1e-8


@pytest.mark.parametrize("mode", ["log", "atomic"])
@pytest.mark.parametrize("name", ["slab", "two_layer", "cornell", "thin_mismatched"])
def test_fixed_point_tally_is_bit_exact(ctx, name, mode):
    prob = dict(slab=S.slab(), two_layer=S.two_layer(), cornell=S.cornell(48),
                thin_mismatched=S.slab(media=((1.0, 9.0, 0.75, 1.4),), thickness=0.5, n=32, voxel=0.05,
                                       n_above=1.0, n_below=1.5))[name]
    n = 20000
    prob.apply(ctx, "u64fx")
    ctx.set_tally_mode(mode)
    ctx.launch(n, seed=17); ctx.sync()
    ctx.set_tally_mode("auto")
    fx, c = ctx.read_grid_raw(), ctx.read_counters()
    _, fxo, co = prob.oracle().run(n, seed=17, threads=8, want_fx=True, want_f64=False)
    check_counters(c, co, n)
    diff = int((fx != fxo).sum())
    assert diff == 0, "%d voxels differ in the 2^-40 fixed-point tally" % diff
    assert fx.sum() > 0
    if name == "thin_mismatched":
        assert c["w_escaped_bottom"] > 0 and c["w_specular"] > 0 and c["w_escaped_top"] > 0
    if name == "cornell":
        assert c["w_escaped_mesh"] > 0


def test_c3_two_layer_parity_f64(ctx):
    prob = S.two_layer()
    n = 20000
    g, c = run_gpu(ctx, prob, n, seed=3)
    go, _, co = prob.oracle().run(n, seed=3, threads=8)
    check_counters(c, co, n)
    S.assert_grid_close(g, go)
    assert abs(c["w_specular"] / n - 0.04) < 1e-12


def test_c4_mesh_bvh_parity_f64(ctx):
    prob = S.cornell(64)
    n = 20000
    g, c = run_gpu(ctx, prob, n, seed=5)
    go, _, co = prob.oracle().run(n, seed=5, threads=8)
    check_counters(c, co, n)
    S.assert_grid_close(g, go)
    # the cone (medium 1: mu_a = 1.0) must show up as an absorbing body around the origin
    mid = g[24:40, 24:40, 24:40].sum()
    assert mid > 0


def test_f32_walk_parity(ctx):
    """f32 walk + f32 tally (the production precision of MC photon codes).  Against the oracle's f32
    restatement on the same XORWOW streams the trajectories agree except where a 1-ulp libm difference flips
    a branch; against the f64 oracle (different draws per uniform) agreement is statistical."""
    prob = S.slab()
    n = 200000
    g32, c32 = run_gpu(ctx, prob, n, dtype="f32", seed=9, f32_walk=True)
    go32, _, co32 = prob.oracle().run(n, seed=9, threads=8, walk_f32=True)
    assert abs(c32["steps"] - co32["steps"]) / co32["steps"] < 2e-4
    for k in ("w_absorbed", "w_escaped_top", "w_lost_outside_grid"):
        assert abs(c32[k] - co32[k]) / n < 2e-4, k
    # voxels with a solid signal: relative agreement (f32 atomics + rare flipped trajectories)
    big = go32 > 1.0
    assert big.sum() > 1000 and np.abs(g32[big] - go32[big]).max() / go32[big].max() < 5e-3
    assert np.abs(g32 - go32).sum() / go32.sum() < 2e-3
    _, _, co = prob.oracle().run(n, seed=9, threads=8, want_f64=False)
    tol = 5 * 0.5 / np.sqrt(n)   # per-photon absorbed weight has sigma < 0.5
    assert abs(c32["w_absorbed"] - co["w_absorbed"]) / n < tol
    assert abs(c32["w_escaped_top"] - co["w_escaped_top"]) / n < tol
    assert abs(c32["steps"] - co["steps"]) / co["steps"] < 0.03
    assert abs(O.conservation_residual(c32)) < 2e-6 * n
    assert abs(g32.sum() - c32["w_absorbed"]) < 1e-4 * n


# ---------------------------------------------------------------- size-independent properties at full size
def test_c2_full_size_properties(ctx):
    """BASELINE config 2: 1e7 photons, 256^3, voxel 0.1 -- too big for the oracle in a test, so:
    energy conservation, launch linearity and shard invariance (bit-exact in fixed point)."""
    prob = S.slab(n=256, voxel=0.1)
    n = 10 ** 7
    prob.apply(ctx, "u64fx")
    ctx.launch(n, seed=1); ctx.sync()
    whole, c = ctx.read_grid_raw(), ctx.read_counters()
    assert c["photons"] == n and abs(O.conservation_residual(c)) < 1e-9 * n
    assert abs(float(whole.sum()) / O.FX_SCALE - c["w_absorbed"]) < 1e-6 * n
    assert 270 < c["steps"] / n < 290 and 0.58 < c["w_absorbed"] / n < 0.61
    # same photons as 3 ragged shards accumulated into one grid: identical bits
    ctx.zero_tally()
    for off, cnt in ((0, 1234567), (1234567, 5000001), (6234568, n - 6234568)):
        ctx.launch(cnt, seed=1, photon_offset=off)
    ctx.sync()
    parts, c2 = ctx.read_grid_raw(), ctx.read_counters()
    assert np.array_equal(whole, parts) and c2["steps"] == c["steps"] and c2["photons"] == n
    # launch geometry must not matter either
    ctx.set_launch_config(2, 128); ctx.zero_tally(); ctx.launch(2000000, seed=1); ctx.sync()
    a = ctx.read_grid_raw()
    ctx.set_launch_config(0, 0); ctx.zero_tally(); ctx.launch(2000000, seed=1); ctx.sync()
    assert np.array_equal(a, ctx.read_grid_raw())


@pytest.mark.parametrize("name", ["c2", "c3", "c4"])
def test_oracle_parity_in_the_shipping_regime(ctx, name):
    """The oracle against the regime that SHIPS.  Every other oracle comparison runs <= 2e5 photons, where the
    library's large-launch machinery is off: two lanes inside a launch need >= 2^21 photons, the tail split >= 512 photons per
    launched wave (2.1e6 on one lane).  Here: BASELINE configs 2, 3 and 4 on their OWN grids (256^3; 0.1 / 0.05 mm / the Cornell
    cube), 2.2e6 photons, default knobs (tally mode auto, overlap auto, tail split default), u64 fixed point -- the first
    launches of a fresh scene run two lanes (pilot batch + 2 : 2 : 1 batches), the third runs one lane, where the slab walks
    end early and a second kernel finishes their photons beside the log reduction.  Each launch must reproduce the oracle's
    grid bit for bit, with equal photon-step counts; lt_last_log_info proves which route ran."""
    import os as _os
    prob = dict(c2=S.slab(n=256, voxel=0.1), c3=S.two_layer(n=256, voxel=0.05), c4=S.cornell(256))[name]
    n = 2200000
    threads = max(1, min(16, len(_os.sched_getaffinity(0))))
    _, fxo, co = prob.oracle().run(n, seed=41, threads=threads, want_fx=True, want_f64=False)
    prob.apply(ctx, "u64fx"); ctx.set_tally_mode("auto"); ctx.set_overlap(0); ctx.set_launch_config(0, 0)
    seen = []
    for k in range(3):
        ctx.zero_tally(); ctx.launch(n, seed=41); ctx.sync()
        fx, c, info = ctx.read_grid_raw(), ctx.read_counters(), ctx.last_log_info()
        assert info is not None, "the default tally mode did not take the deposit log"
        check_counters(c, co, n)
        diff = int((fx != fxo).sum())
        assert diff == 0, "%s, launch %d (%d lanes): %d voxels differ from the oracle in the 2^-40 fixed-point tally" % (name, k, info["lanes"], diff)
        seen.append((info["lanes"], info["records"] + info["overflow_records"], info["batches"]))
    assert fxo.sum() > 0
    # overlap auto: two lanes twice (the first launch of a scene carries the pilot batch: not a clean timing), then one lane
    assert [s[0] for s in seen] == [2, 2, 1], seen
    assert seen[0][2] >= 4 and seen[1][2] >= 3 and seen[2][2] == 1, seen        # pilot + 2 : 2 : 1 batches / 2 : 2 : 1 / one batch
    # the one-lane launch split its walk (slab and LDS-mesh kernels alike): the tail kernel's deposits go to the grid as atomics
    # and are not log records (0.7-1.3 % of them at this size; scheduling alone moves the count by ~1e-5)
    assert seen[2][1] < 0.998 * seen[1][1], seen
    ctx.set_overlap(0)


@pytest.mark.parametrize("name", ["c3", "c4"])
def test_c3_c4_full_size_properties(ctx, name):
    """BASELINE configs 3 (two-layer slab) and 4 (mesh + BVH) at their own size -- 1e7 photons, 256^3: energy
    conservation, one launch == three ragged shards, log tally == atomic tally (u64 fixed point, bit for bit); for the
    mesh also == the walk with every surface-query shortcut switched off (2e6 photons)."""
    prob = S.two_layer(n=256, voxel=0.05) if name == "c3" else S.cornell(256)
    n = 10 ** 7
    prob.apply(ctx, "u64fx"); ctx.set_tally_mode("log")
    ctx.launch(n, seed=3); ctx.sync()
    whole, c = ctx.read_grid_raw(), ctx.read_counters()
    assert ctx.last_log_info() is not None
    assert c["photons"] == n and abs(O.conservation_residual(c)) < 1e-9 * n
    assert abs(float(whole.sum()) / O.FX_SCALE - c["w_absorbed"]) < 1e-6 * n
    if name == "c4":
        assert c["w_escaped_mesh"] > 0.1 * n and 140 < c["steps"] / n < 156
    else:
        assert 260 < c["steps"] / n < 282
    ctx.zero_tally()
    for off, cnt in ((0, 2345678), (2345678, 4000001), (6345679, n - 6345679)):
        ctx.launch(cnt, seed=3, photon_offset=off)
    ctx.sync()
    assert np.array_equal(whole, ctx.read_grid_raw()) and ctx.read_counters()["steps"] == c["steps"]
    prob.apply(ctx, "u64fx"); ctx.set_tally_mode("atomic")
    ctx.launch(n, seed=3); ctx.sync()
    assert np.array_equal(whole, ctx.read_grid_raw()) and ctx.read_counters()["steps"] == c["steps"]
    if name == "c4":
        m = 2 * 10 ** 6
        ctx.zero_tally(); ctx.launch(m, seed=4); ctx.sync()
        a, ca = ctx.read_grid_raw(), ctx.read_counters()
        assert ctx.mesh_accel_info()["kind"] == 1              # (the run above used the clearance grid with near-triangle lists)
        with ctx.tuning(no_clearance=1):                       # every step queries the BVH
            prob.apply(ctx, "u64fx"); ctx.set_tally_mode("atomic")
            ctx.launch(m, seed=4); ctx.sync()
            assert ctx.mesh_accel_info()["kind"] == 0          # ... and this one really ran without it
        assert np.array_equal(a, ctx.read_grid_raw()) and ctx.read_counters()["steps"] == ca["steps"]
        prob.apply(ctx, "u64fx")      # (tables with the clearance grid again for whoever uses the session ctx next)
    ctx.set_tally_mode(2)


def test_large_mesh_full_size_properties(ctx, golden_dir):
    """The reference's teapot (6320 triangles + box: march grid, walk_kernel_m) at the BASELINE size -- 1e7 photons, 256^3:
    energy conservation; one launch == three ragged shards; log tally == atomic tally; and, at 2e6 photons, == the walk
    with the march grid switched off (walk_kernel_q over the BVH) -- u64 fixed point, bit for bit.  At this size every
    wave's candidate queue drains tens of thousands of times under every interleaving of marching, waiting and resolved
    lanes: what a 20 000-photon parity run against the oracle cannot exercise."""
    g = load(golden_dir, "g10_obj_meshes.npz")
    prob = S.obj_in_box(g["teapot_verts"], g["teapot_faces"], n=256)[0]
    n = 10 ** 7
    prob.apply(ctx, "u64fx"); ctx.set_tally_mode("log")
    ctx.launch(n, seed=3); ctx.sync()
    whole, c = ctx.read_grid_raw(), ctx.read_counters()
    assert ctx.mesh_accel_info()["kind"] & 2 and ctx.last_log_info() is not None
    assert c["photons"] == n and abs(O.conservation_residual(c)) < 1e-9 * n
    assert abs(float(whole.sum()) / O.FX_SCALE - c["w_absorbed"]) < 1e-6 * n
    assert 38 < c["steps"] / n < 48 and c["w_escaped_mesh"] > 0.3 * n
    ctx.zero_tally()
    for off, cnt in ((0, 2345678), (2345678, 4000001), (6345679, n - 6345679)):
        ctx.launch(cnt, seed=3, photon_offset=off)
    ctx.sync()
    assert np.array_equal(whole, ctx.read_grid_raw()) and ctx.read_counters()["steps"] == c["steps"]
    prob.apply(ctx, "u64fx"); ctx.set_tally_mode("atomic")
    ctx.launch(n, seed=3); ctx.sync()
    assert np.array_equal(whole, ctx.read_grid_raw()) and ctx.read_counters()["steps"] == c["steps"]
    m = 2 * 10 ** 6
    ctx.zero_tally(); ctx.launch(m, seed=4); ctx.sync()
    a, ca = ctx.read_grid_raw(), ctx.read_counters()
    with ctx.tuning(no_march=1):
        prob.apply(ctx, "u64fx"); ctx.set_tally_mode("atomic")
        ctx.launch(m, seed=4); ctx.sync()
        assert ctx.mesh_accel_info()["kind"] == 0
    assert np.array_equal(a, ctx.read_grid_raw()) and ctx.read_counters()["steps"] == ca["steps"]
    ctx.set_tally_mode(2)


def test_f32_tally_full_size_symmetry(ctx):
    prob = S.slab(n=255, voxel=0.1)   # odd: beam axis through the middle of column 127
    n = 4 * 10 ** 6
    g, c = run_gpu(ctx, prob, n, dtype="f32", seed=2, f32_walk=True)
    a, b = g[:, :, :127].sum(), g[:, :, 128:].sum()
    cc, d = g[:, :127, :].sum(), g[:, 128:, :].sum()
    assert abs(a - b) / (a + b) < 5e-3 and abs(cc - d) / (cc + d) < 5e-3
    # the f32 tally itself loses bits where millions of ~1e-2 deposits pile onto one voxel (the on-axis
    # column holds ~1e4 after 4e6 photons: ulp 1e-3): a documented property of float tallies, bounded here
    assert abs(g.sum() - c["w_absorbed"]) < 2e-3 * n


# ---------------------------------------------------------------- edge cases
def test_edge_cases(ctx):
    prob = S.slab(n=8, voxel=1.0)
    prob.apply(ctx, "f64")
    ctx.launch(0); ctx.sync()                                  # empty launch
    assert ctx.read_counters()["photons"] == 0 and ctx.read_grid().sum() == 0
    ctx.launch(1, seed=4); ctx.sync()                          # a single photon: one lane of one wave
    c = ctx.read_counters()
    go, _, co = prob.oracle().run(1, seed=4)
    assert c["steps"] == co["steps"] and abs(O.conservation_residual(c)) < 1e-12
    ctx.zero_tally()
    ctx.launch(63, seed=4); ctx.launch(65, seed=4, photon_offset=63); ctx.sync()   # ragged around a wave
    go, _, co = prob.oracle().run(128, seed=4)
    check_counters(ctx.read_counters(), co, 128)
    S.assert_grid_close(ctx.read_grid(), go)
    # max_steps cap: every photon stopped after 3 steps keeps its weight in w_capped
    prob.max_steps = 3
    g, c = run_gpu(ctx, prob, 5000, seed=6)
    go, _, co = prob.oracle().run(5000, seed=6)
    check_counters(c, co, 5000)
    assert c["w_capped"] > 4000 and c["steps"] <= 3 * 5000
    # pure absorber (mu_s = 0): Beer-Lambert column, one step per photon
    pa = S.Problem([(2.0, 0.0, 0.0, 1.0)], (1, 1, 40), (-1.0, -1.0, 0.0), (2.0, 2.0, 0.05),
                   layers=dict(z_bounds=[0.0, np.inf], medium_idx=[0]))
    g, c = run_gpu(ctx, pa, 100000, seed=7)
    z = np.arange(41) * 0.05
    expect = 100000 * (np.exp(-2.0 * z[:-1]) - np.exp(-2.0 * z[1:]))
    assert np.all(np.abs(g[:, 0, 0] - expect) < 5 * np.sqrt(expect) + 1) and c["steps"] == 100000
    # non-interacting medium (mu_t = 0) between two planes: everything is transmitted
    tr = S.Problem([(0.0, 0.0, 0.0, 1.0)], (2, 2, 2), (-1, -1, 0), (1, 1, 1),
                   layers=dict(z_bounds=[0.0, 2.0], medium_idx=[0]))
    g, c = run_gpu(ctx, tr, 1000, seed=8)
    assert c["w_escaped_bottom"] == 1000 and g.sum() == 0


def test_api_errors(ctx):
    import light_transport_amd as lt
    with pytest.raises(lt.LtError):
        ctx.set_media([(-1.0, 1.0, 0.0, 1.0)])
    with pytest.raises(lt.LtError):
        ctx.set_layers([0.0, -1.0], [0])
    with pytest.raises(lt.LtError):
        ctx.set_grid((0, 4, 4), (0, 0, 0), (1, 1, 1))
    S.slab(n=8, voxel=1.0).apply(ctx, "f32")
    with pytest.raises(lt.LtError):     # table RNG is the f64 parity mode
        ctx.launch(4, rng_table=np.zeros((4, 3, 4)))
    c2 = lt.Context(0)
    with pytest.raises(lt.LtError):     # launch before the scene is set
        c2.launch(10)
    c2.close()


def test_trace_photons_one_call_api(ctx):
    from light_transport_amd.src import photon_tracing as PT
    slab = PT.LayeredSlab([PT.OpticalMedium(0.1, 10.0, 0.9, 1.0)], [np.inf])
    grid = PT.VoxelGrid((64, 64, 64), (-12.8, -12.8, 0.0), 0.4, dtype="f64")
    dose, cnt = PT.trace_photons(slab, None, None, 10000, seed=0, grid=grid, source=PT.PencilBeam((0, 0, 0), (0, 0, 1)),
                                 return_counters=True)
    go, _, co = S.slab().oracle().run(10000, seed=0, threads=8)
    assert dose.shape == (64, 64, 64) and dose.dtype == np.float64
    S.assert_grid_close(dose, go)
    assert cnt["steps"] == co["steps"]
    # a call is a pure function of its arguments: settings of an earlier call on the shared context do not leak
    capped = PT.trace_photons(slab, None, None, 2000, seed=0, grid=grid, source=PT.PencilBeam((0, 0, 0), (0, 0, 1)), max_steps=5,
                              return_counters=True)[1]
    again = PT.trace_photons(slab, None, None, 2000, seed=0, grid=grid, source=PT.PencilBeam((0, 0, 0), (0, 0, 1)),
                             return_counters=True)[1]
    assert capped["w_capped"] > 1000 and capped["steps"] <= 5 * 2000
    assert again["w_capped"] == 0 and again["steps"] > 100 * 2000
    # mesh scene through the object API
    ordered, linear = S.cornell_scene()
    vol = PT.MeshVolume([PT.OpticalMedium(0.1, 10.0, 0.9, 1.0), PT.OpticalMedium(1.0, 5.0, 0.8, 1.5)], start_medium=0)
    grid = PT.VoxelGrid((32, 32, 32), (-7.5,) * 3, 15.0 / 32, dtype="f64")
    light = PT.AreaLight((-1.0, 7.5, -1.0), (2.0, 0.0, 0.0), (0.0, 0.0, 2.0), (0.0, -1.0, 0.0))
    dose = PT.trace_photons(vol, ordered, linear, 4000, seed=2, grid=grid, source=light)
    go, _, _ = S.cornell(32).oracle().run(4000, seed=2, threads=8)
    S.assert_grid_close(dose, go)


# ---------------------------------------------------------------- tally quantity: fluence in heterogeneous media
def test_fluence_quantity(ctx):
    """lt_set_tally_quantity(LT_QUANTITY_FLUENCE): an interaction adds w / mu_t (= dw / mu_a) to its voxel, so the grid is
    fluence x dV x N without a per-voxel mu_a.  GPU == oracle bit for bit (u64 fixed point) on the two-layer slab and on the
    Cornell cavity + cone (two media, mesh); the counters keep booking absorbed weight (identical to an absorbed-weight run);
    on a slab whose layer plane lies on a voxel boundary  sum_v grid[v] mu_a(layer of v) == w_absorbed;  a layer that does
    not absorb (mu_a = 0) has fluence although it has no absorbed weight."""
    n = 20000
    for prob in (S.two_layer(n=64, voxel=0.05), S.cornell(32)):
        prob.apply(ctx, "u64fx"); ctx.set_tally_quantity("fluence")
        ctx.launch(n, seed=9); ctx.sync()
        fx, c = ctx.read_grid_raw(), ctx.read_counters()
        o = prob.oracle(); o.quantity = 1
        _, fxo, co = o.run(n, seed=9, threads=8, want_fx=True, want_f64=False)
        check_counters(c, co, n)
        assert np.array_equal(fx, fxo)
        ctx.set_tally_quantity("absorbed"); ctx.zero_tally()
        ctx.launch(n, seed=9); ctx.sync()
        ca, fa = ctx.read_counters(), ctx.read_grid_raw()
        # the walk itself is unchanged: identical step count; w_absorbed is a float sum over lanes / waves whose order
        # depends on which lane traced which photon, so two runs agree to rounding (1 ulp seen), not bitwise
        assert ca["steps"] == c["steps"], (ca["steps"], c["steps"])
        assert abs(ca["w_absorbed"] - c["w_absorbed"]) <= 1e-12 * c["w_absorbed"], (ca["w_absorbed"], c["w_absorbed"])
        assert not np.array_equal(fa, fx)
    # conservation through the fluence grid: layer plane z = 0.1 on the boundary of voxel rows 1 | 2 (voxel 0.05)
    prob = S.two_layer(n=64, voxel=0.05)
    prob.apply(ctx, "f64"); ctx.set_tally_quantity("fluence")
    ctx.launch(200000, seed=3); ctx.sync()
    g, c = ctx.read_grid(), ctx.read_counters()
    mu_a = np.where(np.arange(64) < 2, 0.43, 0.27)
    assert abs((g * mu_a[:, None, None]).sum() - c["w_absorbed"]) < 1e-9 * 200000
    # a medium that does not absorb: fluence, but no absorbed weight, in its rows
    prob.media = [(0.0, 10.7, 0.79, 1.5), (0.27, 18.7, 0.82, 1.4)]
    prob.apply(ctx, "f64"); ctx.set_tally_quantity("fluence")
    ctx.launch(50000, seed=4); ctx.sync()
    gf = ctx.read_grid()
    ctx.set_tally_quantity("absorbed"); ctx.zero_tally(); ctx.launch(50000, seed=4); ctx.sync()
    ga = ctx.read_grid()
    assert gf[:2].sum() > 100.0 and ga[:2].sum() == 0.0 and ga[2:].sum() > 0.0
    ctx.set_tally_quantity("absorbed")


# ---------------------------------------------------------------- f1: meshes beyond the LDS budget, SAH builder
def test_large_mesh_in_global_memory(ctx):
    """5140 triangles / ~10^4 nodes (~1.2 MB of tables, beyond the LDS budget): tables in global memory, surface queries
    through the march grid (walk_kernel_m), built with the binned-SAH splitter.  Nearest hits: BVH == brute force == march
    (both forms) == oracle; walk: bit-exact tally; the f32 walk against the oracle's f32 walk."""
    prob, ordered, linear = S.sphere_in_box(4, split_method=0)
    assert len(ordered) == 5140
    from light_transport_amd.src import bvh_new as B
    rs = np.random.RandomState(8)
    o = rs.uniform(-3.9, 3.9, size=(20000, 3))
    d = rs.normal(size=(20000, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    tmax = np.where(rs.rand(20000) < 0.5, np.inf, rs.uniform(0.05, 4.0, size=20000))
    # awkward rays for a grid march: axis-parallel directions (zero components), origins on cell walls / grid corners /
    # outside the box (those take the BVH), hops far shorter than a cell
    d[:300] = np.eye(3)[rs.randint(0, 3, 300)] * rs.choice([-1.0, 1.0], size=(300, 1))
    d[300:600, 0] = 0.0; d[300:600] /= np.linalg.norm(d[300:600], axis=1, keepdims=True)
    o[600:900] = np.round(o[600:900] * 8) / 8
    o[900:1000] = rs.choice([-4.0, 4.0], size=(100, 3))
    o[1000:1300] = rs.uniform(-6, 6, size=(300, 3))
    tmax[1300:1600] = rs.uniform(1e-6, 1e-2, size=300)
    p1, t1 = B.intersect_bvh_batch(o, d, ordered, linear, tmax, True, ctx)
    p0, t0 = B.intersect_bvh_batch(o, d, ordered, linear, tmax, False, ctx)
    np.testing.assert_array_equal(p1, p0); np.testing.assert_array_equal(t1, t0)
    # the grid march (what the walk uses for this mesh) answers every ray exactly as the brute-force scan does
    for form in (2, 3, 4):       # 2: the walk's wave-cooperative service, 3: the same march lane by lane; 4: the BVH front to back
        p2, t2 = B.intersect_bvh_batch(o, d, ordered, linear, tmax, form, ctx)
        np.testing.assert_array_equal(p2, p0); np.testing.assert_array_equal(t2, t0)
    po, to = prob.oracle().intersect_rays(o, d, tmax, use_bvh=True)
    # index work is exact; a different triangle is only accepted as a tie: equal distance on two triangles that share
    # an edge (which of them claims a ray through the common edge is decided in the last bit, and the kernel fuses
    # multiply-adds where the oracle does not)
    assert np.array_equal(p1 >= 0, po >= 0)
    np.testing.assert_allclose(t1[p1 >= 0], to[p1 >= 0], rtol=1e-11)
    verts3 = B.triangles_array(ordered).reshape(-1, 3, 3)
    for i in np.flatnonzero(p1 != po):
        assert S.share_an_edge(verts3[p1[i]], verts3[po[i]]), "ray %d: different triangles that share no edge" % i
    assert (p1 != po).mean() < 2e-3
    assert (p1 >= 0).mean() > 0.5
    n = 20000
    prob.apply(ctx, "u64fx")
    ctx.launch(n, seed=4); ctx.sync()
    fx, c = ctx.read_grid_raw(), ctx.read_counters()
    _, fxo, co = prob.oracle().run(n, seed=4, threads=8, want_fx=True, want_f64=False)
    check_counters(c, co, n)
    assert int((fx != fxo).sum()) == 0
    assert c["w_escaped_mesh"] > 0 and fx.sum() > 0
    # the f32 walk through the same mesh (walk_kernel_m<float>: 32-bit hit slots, f32 march)
    # against the oracle's f32 restatement on the same XORWOW streams, as test_f32_walk_parity does for the slab
    n32 = 100000
    g32, c32 = run_gpu(ctx, prob, n32, dtype="f32", seed=9, f32_walk=True)
    go32, _, co32 = prob.oracle().run(n32, seed=9, threads=8, walk_f32=True)
    assert abs(O.conservation_residual(c32)) < 2e-5 * n32
    assert abs(c32["steps"] - co32["steps"]) / co32["steps"] < 2e-3
    for k in ("w_absorbed", "w_escaped_mesh", "w_lost_outside_grid"):
        assert abs(c32[k] - co32[k]) / n32 < 2e-3, (k, c32[k], co32[k])
    assert np.abs(g32 - go32).sum() / go32.sum() < 2e-2


def test_integration_md_stub_runs_as_written(ctx):
    """INTEGRATION.md shows the ctypes stub a maintainer would put into the reference's empty src/photon_tracing.py.  It
    is documentation that claims to work: extract the FIRST python block verbatim, point its CDLL at the built library,
    execute it, and hold its result against the package's own trace_photons on the same problem -- the same photons
    (seed, ids) through the same kernels, so the f64 grids agree to summation order and the step counts exactly."""
    import re
    import light_transport_amd as lt
    from light_transport_amd.src import photon_tracing as PT
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "INTEGRATION.md")).read()
    block = re.search(r"```python\n(.*?)```", text, re.S).group(1)
    assert "def trace_photons(" in block and 'C.CDLL("liblt_hip.so")' in block
    ns = {}
    exec(compile(block.replace('C.CDLL("liblt_hip.so")', "C.CDLL(%r)" % lt.LIB_PATH), "INTEGRATION.md", "exec"), ns)
    media = [(0.43, 10.7, 0.79, 1.5), (0.27, 18.7, 0.82, 1.4)]
    n, shape, origin, voxel = 50000, (32, 32, 32), (-3.2, -3.2, 0.0), (0.2, 0.2, 0.2)
    got = ns["trace_photons"](media, [0.0, 0.1, np.inf], n, 7, shape, origin, voxel)
    slab = PT.LayeredSlab([PT.OpticalMedium(*m) for m in media], [0.1, np.inf])
    want, c = PT.trace_photons(slab, None, None, n, seed=7, grid=PT.VoxelGrid(shape, origin, voxel), source=PT.PencilBeam((0, 0, 0), (0, 0, 1)),
                               return_counters=True)
    assert got.shape == want.shape == (32, 32, 32) and got.sum() > 0.3 * n
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-12)
    assert abs(got.sum() - c["w_absorbed"]) < 1e-9 * n


def test_open_and_flat_meshes_beyond_lds(ctx):
    """What closed boxes never exercise: photons all AROUND a mesh (an open one: two sheets in free space), outside its
    bounding box too, a sheet with zero extent on one axis, degenerate triangles among the 5003.  Hits: BVH == brute force
    == march (both forms) for rays from everywhere, far outside included; the fixed-point walk == the CPU oracle bit for
    bit, with the march grid in use (one cell of margin around the root bounds keeps photons next to the mesh inside it)
    and with it switched off."""
    prob, ordered, linear = S.open_sheets()
    assert len(ordered) == 5003
    from light_transport_amd.src import bvh_new as B
    rs = np.random.RandomState(12)
    n = 30000
    o = rs.uniform(-7, 7, size=(n, 3)); o[:5000] = rs.uniform(-4, 4, size=(5000, 3)) * [1, 1, 0.2]; o[5000:6000, 2] = -2.0      # incl. ON the flat sheet's plane
    d = rs.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[6000:6500] = [0.0, 0.0, -1.0]; d[6500:7000] = np.eye(3)[rs.randint(0, 2, 500)]          # straight down; sliding parallel to the sheets
    cent = B.triangles_array(ordered).mean(axis=1)          # a third of the rays are aimed at (or just past) random triangles
    aim = cent[rs.randint(0, len(cent), 10000)] + rs.normal(0, 0.05, size=(10000, 3))
    d[20000:] = aim - o[20000:]; d[20000:] /= np.linalg.norm(d[20000:], axis=1, keepdims=True)
    tmax = np.where(rs.rand(n) < 0.4, np.inf, rs.exponential(1.0, size=n))
    tmax[20000:] = np.where(rs.rand(10000) < 0.7, np.inf, rs.exponential(6.0, size=10000))
    p0, t0 = B.intersect_bvh_batch(o, d, ordered, linear, tmax, False, ctx)
    for form in (1, 2, 3):
        p, t = B.intersect_bvh_batch(o, d, ordered, linear, tmax, form, ctx)
        np.testing.assert_array_equal(p, p0); np.testing.assert_array_equal(t, t0)
    assert (p0 >= 0).mean() > 0.25 and len(np.unique(p0[p0 >= 0])) > 3000          # hits on most of the 5000 triangles; two thirds of the rays miss
    assert not np.isin(p0, np.flatnonzero(np.isnan(B.triangles_array(ordered)).any(axis=(1, 2)))).any()
    n = 20000
    _, fxo, co = prob.oracle().run(n, seed=17, threads=8, want_fx=True, want_f64=False)
    for knobs in ({}, {"no_march": 1}, {"march_cells": 40}):
        with ctx.tuning(**knobs):
            prob.apply(ctx, "u64fx")
            ctx.launch(n, seed=17); ctx.sync()
            assert (ctx.mesh_accel_info()["kind"] & 2 != 0) == ("no_march" not in knobs)
        c = ctx.read_counters()
        check_counters(c, co, n)
        assert np.array_equal(ctx.read_grid_raw(), fxo), knobs
    assert c["w_escaped_mesh"] > 0.005 * n and c["w_lost_outside_grid"] > 0.05 * n          # photons did leave through the flat sheet, and roamed off the tally grid


def test_deep_bvh_is_accepted(ctx):
    """A flattened tree far deeper than 31 levels (a chain: every interior node splits one triangle off) is a valid input:
    the device traversal is stackless.  (Rounds 1-2 rejected depth >= 31 'exceeds the traversal stack'.)"""
    T = 60
    verts, nodes = S.chain_mesh(T)
    none = -np.ones(T, np.int32)
    ctx.set_mesh(verts, none, none, nodes)          # depth 59
    ctx._mesh_key = None
    n = 20000
    o, d, k = S.chain_rays(verts, n)
    p1, t1 = ctx.intersect_rays(o, d, None, 1)
    p0, t0 = ctx.intersect_rays(o, d, None, 0)
    np.testing.assert_array_equal(p1, p0); np.testing.assert_array_equal(t1, t0)
    p4, t4 = ctx.intersect_rays(o, d, None, 4)          # front to back, threaded per direction sign pattern: no stack either
    np.testing.assert_array_equal(p4, p0); np.testing.assert_array_equal(t4, t0)
    tm = np.random.RandomState(8).uniform(0.2, 6.0, n)  # ... and with a finite reach (shadow rays, hops)
    p4, t4 = ctx.intersect_rays(o, d, tm, 4); p0b, t0b = ctx.intersect_rays(o, d, tm, 0)
    np.testing.assert_array_equal(p4, p0b); np.testing.assert_array_equal(t4, t0b)
    assert (p0 >= 0).mean() > 0.4 and len(np.unique(p0[p0 >= 0])) == T          # every link of the chain is somebody's nearest hit
    assert (p0[p0 >= 0] != k[p0 >= 0]).mean() > 0.3                             # ... and not always the one aimed at: an earlier link was in the way
    nodes["offset"][0] = 1                          # ... while a malformed tree is still refused
    with pytest.raises(Exception):
        ctx.set_mesh(verts, none, none, nodes)


def test_grid_march_equals_brute_force(ctx):
    """The march grid on meshes of very different grain -- 30 wall-sized triangles (config 4's scene: every triangle spans
    thousands of cells) and the 5140-triangle sphere -- at several resolutions: prim and t equal the brute-force scan's
    bit for bit on 30000 rays (same tri_hit, same nearest / tie rule; only the set of triangles tested differs)."""
    from light_transport_amd.src import bvh_new as B
    rs = np.random.RandomState(21)
    seen = set()
    for (ordered, linear), half in ((S.cornell_scene(), 7.5), (S.sphere_in_box(3)[1:3], 4.0)):
        n = 30000
        o = rs.uniform(-half, half, size=(n, 3))
        d = rs.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
        d[:500] = np.eye(3)[rs.randint(0, 3, 500)] * rs.choice([-1.0, 1.0], size=(500, 1))
        o[500:1500] = np.round(o[500:1500])                      # on cell walls of most resolutions
        tmax = np.where(rs.rand(n) < 0.3, np.inf, rs.exponential(0.5, size=n))
        p0, t0 = B.intersect_bvh_batch(o, d, ordered, linear, tmax, False, ctx)
        for cells in (16, 50, 128, -1):
            ctx.set_tuning("march_cells", cells)
            ctx.set_mesh(B.triangles_array(ordered), -np.ones(len(ordered), np.int32), -np.ones(len(ordered), np.int32),
                         B.linear_bvh_arrays(linear))       # a fresh mesh: the grid is rebuilt at this resolution
            ctx._mesh_key = None
            for form in (2, 3):
                p2, t2 = ctx.intersect_rays(o, d, tmax, form)
                np.testing.assert_array_equal(p2, p0); np.testing.assert_array_equal(t2, t0)
            info = ctx.mesh_accel_info()           # the knob really took: the grid has that many cells along its longest axis
            assert info["kind"] & 2 and info["march_entries"] > 0
            if cells > 0:
                assert max(info["march_dims"]) == cells + 2, info          # (+ one cell of margin on either side)
            else:
                seen.add(max(info["march_dims"]))
        assert (p0 >= 0).mean() > 0.3
    assert len(seen) == 2 and all(34 <= v <= 258 for v in seen)     # the default resolution follows the meshes' grain


# ---------------------------------------------------------------- f3: meshes that came through the OBJ loader (G10)
@pytest.mark.parametrize("name", ["teapot", "cow", "pumpkin", "wine-glass", "glass", "diamond", "square"])
def test_g10_obj_meshes_on_the_gpu(ctx, golden_dir, tmp_path, name):
    """The reference's on-disk input (examples/obj/*.obj; S/io.py:11-40) on the device -- every asset the reference ships:
    fixture vertices / faces -> OBJ file -> load_obj -> SAH build_bvh (S/bvh_new.py:198-258) -> BVH, brute force and grid
    march.  teapot / cow / pumpkin / wine-glass (25 346 triangles, the largest) are far beyond the LDS budget: tables in
    global memory, walk_kernel_m; glass / diamond / square fit LDS.  Nearest hits of the fixture's rays == the reference's
    triangle_intersect run over every triangle (brute force); the fixed-point walk through the mesh == the CPU oracle bit
    for bit."""
    from tests.test_oracle_golden import _g10_file
    g, name = _g10_file(golden_dir, name)
    from light_transport_amd.src import bvh_new as B, constants as K
    from light_transport_amd.src.io import load_obj
    v, f = g[name + "_verts"], g[name + "_faces"]
    path = tmp_path / (name + ".obj")            # the same forms the reference's assets use: v x y z / f a b c / f a//n b//n c//n
    with open(path, "w") as fh:
        fh.write("# %s (G10 fixture)\n" % name)
        for p in v:
            fh.write("v %r %r %r\n" % (float(p[0]), float(p[1]), float(p[2])))
        for k, (a, b, c) in enumerate(f):
            fh.write(("f %d//%d %d//%d %d//%d\n" % (a + 1, 1, b + 1, 1, c + 1, 1)) if k % 2 else ("f %d %d %d\n" % (a + 1, b + 1, c + 1)))
    objects, dimension = load_obj(str(path), K.GLASS_MAT)
    assert len(objects) == len(f) and dimension == abs(v.max())
    for k, t in enumerate(objects):
        t.face_index = k
    ordered, linear = B.build_linear_bvh(objects, 0)
    back = np.array([t.face_index for t in ordered])
    tri_xyz = v[f]
    for use_bvh in (True, False, 2):         # BVH, brute force, grid march
        prim, t = B.intersect_bvh_batch(g[name + "_origins"], g[name + "_dirs"], ordered, linear, None, use_bvh, ctx)
        got = np.where(prim >= 0, back[np.maximum(prim, 0)], -1)
        ties = S.check_hits_against_fixture(got, t, g[name + "_prim"], g[name + "_t"], g[name + "_second"], tri_xyz)
        assert ties <= 6
    assert (g[name + "_prim"] >= 0).sum() >= 190
    # the walk through the loader's mesh (beyond LDS: walk_kernel_m over the march grid), both tally paths
    prob, ordered2, _, _, _, _ = S.obj_in_box(v, f)
    assert len(ordered2) == len(f) + 20
    n = 6000
    _, fxo, co = prob.oracle().run(n, seed=61, threads=8, want_fx=True, want_f64=False)
    for mode in ("atomic", "log"):
        prob.apply(ctx, "u64fx"); ctx.set_tally_mode(mode)
        ctx.launch(n, seed=61); ctx.sync()
        c = ctx.read_counters()
        check_counters(c, co, n)
        assert np.array_equal(ctx.read_grid_raw(), fxo), mode
    ctx.set_tally_mode("auto")
    assert c["w_absorbed"] > 0.05 * n


# ---------------------------------------------------------------- f2: surface path tracer vs the reference render
@pytest.mark.parametrize("name", ["glass", "mirror"])
def test_g8_surface_render(ctx, golden_dir, name):
    """render_scene (path_tracing_fix1.py:139-169) through lt_render_surface against the image the REFERENCE
    produced from the same tables (G8), incl. the +inf markers it leaves in rand_0."""
    from light_transport_amd import _lib
    g8 = load(golden_dir, "g8_render_fix1.npz")
    inp = S.g8_inputs(g8, name)
    m = inp["mesh"]
    ctx.set_mesh(m["verts"], m["med_front"], m["med_back"], m["nodes"])
    mats = (_lib.SurfaceMaterial * len(inp["mats"]))()
    for i, r in enumerate(inp["mats"]):
        mats[i].diffuse[:] = list(r[:3]); mats[i].emission, mats[i].ior, mats[i].transmission = r[3], r[4], r[5]
        mats[i].is_diffuse, mats[i].is_mirror, mats[i].is_light = int(r[6]), int(r[7]), int(r[8])
    lights = (_lib.PointLight * len(inp["lights"]))()
    for i, r in enumerate(inp["lights"]):
        lights[i].source[:] = list(r[:3]); lights[i].normal[:] = list(r[3:6]); lights[i].radiance[:] = list(r[6:9])
        lights[i].total_area = r[9]
    ctx.set_surface_materials(mats); ctx.set_lights(lights)
    H, W, _, _ = inp["shape"]
    img = np.zeros((H, W, 3)); r0 = inp["rand_0"].copy()
    ctx.render_surface(inp["camera"], inp["f_distance"], inp["xs"], inp["ys"], r0, np.ascontiguousarray(inp["rand_1"]),
                       inp["light_choice"], img)
    S.check_g8_image(img, r0, g8, name)
    # accumulation semantics of :166 (4 calls -> full image): a second call adds the same quarter again
    r0b = inp["rand_0"].copy()
    ctx.render_surface(inp["camera"], inp["f_distance"], inp["xs"], inp["ys"], r0b, np.ascontiguousarray(inp["rand_1"]),
                       inp["light_choice"], img)
    np.testing.assert_allclose(img, 2 * g8[name + "_brute_image"], rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("name", ["glass", "mirror"])
def test_g9_recursive_surface_render(ctx, golden_dir, name):
    """path_tracing_old.render_scene (:17-171, the integrator examples/LTS.ipynb calls) through lt_render_surface_old
    against the image the REFERENCE produced from the same tables (G9); the recursion runs on a per-lane stack."""
    from light_transport_amd import _lib
    g9 = load(golden_dir, "g9_render_old.npz")
    inp = S.g8_inputs(g9, name)
    m = inp["mesh"]
    ctx.set_mesh(m["verts"], m["med_front"], m["med_back"], m["nodes"])
    mats = (_lib.SurfaceMaterial * len(inp["mats"]))()
    for i, r in enumerate(inp["mats"]):
        mats[i].diffuse[:] = list(r[:3]); mats[i].emission, mats[i].ior, mats[i].transmission = r[3], r[4], r[5]
        mats[i].is_diffuse, mats[i].is_mirror, mats[i].is_light = int(r[6]), int(r[7]), int(r[8])
    lights = (_lib.PointLight * len(inp["lights"]))()
    for i, r in enumerate(inp["lights"]):
        lights[i].source[:] = list(r[:3]); lights[i].normal[:] = list(r[3:6]); lights[i].radiance[:] = list(r[6:9])
        lights[i].total_area = r[9]
    ctx.set_surface_materials(mats); ctx.set_lights(lights)
    H, W, _, _ = inp["shape"]
    img = np.full((H, W, 3), 9.0); r0 = inp["rand_0"].copy()       # overwritten, not accumulated (:167)
    ctx.render_surface(inp["camera"], inp["f_distance"], inp["xs"], inp["ys"], r0, np.ascontiguousarray(inp["rand_1"]),
                       inp["light_choice"], img, old=True)
    S.check_g9_image(img, r0, g9, name)
    # deeper than the fixture: the unrolled recursion against the oracle's real recursion, wrapped choice table (Q = 5)
    rs = np.random.RandomState(5)
    Hh, Ww, Ss, Dd = 12, 18, 2, 14
    r0 = rs.rand(Hh, Ww, Ss, Dd); r1 = rs.rand(Hh, Ww, Ss, Dd); lc = rs.randint(0, len(inp["lights"]), size=(Hh, Ww, Ss, 5))
    xs, ys = np.linspace(-1, 1, Ww), np.linspace(1 / (Ww / Hh), -1 / (Ww / Hh), Hh)
    img, imgo, r0o = np.zeros((Hh, Ww, 3)), np.zeros((Hh, Ww, 3)), r0.copy()
    ctx.render_surface(inp["camera"], inp["f_distance"], xs, ys, r0, r1, lc, img, old=True)
    sc = O.OracleScene([(0, 0, 0, 1)], (1, 1, 1), (0, 0, 0), (1, 1, 1), mesh=inp["mesh"])
    O.render_surface(sc, inp["mats"], inp["lights"], inp["camera"], inp["f_distance"], xs, ys, r0o, r1, lc, imgo, old=True)
    np.testing.assert_allclose(img, imgo, rtol=1e-9, atol=1e-12)
    assert np.array_equal(np.isinf(r0), np.isinf(r0o))
    with pytest.raises(_lib.LtError):
        ctx.render_surface(inp["camera"], inp["f_distance"], xs, ys, np.zeros((Hh, Ww, 1, 25)), np.zeros((Hh, Ww, 1, 25)),
                           np.zeros((Hh, Ww, 1, 3), np.int32), img, old=True)     # max_depth > 24


def test_render_scene_old_object_api(ctx):
    """The LTS.ipynb call: path_tracing_old.render_scene(scene, primitives, bvh) -> ndarray (overwrites scene.image)."""
    from light_transport_amd.src import constants as K, cornell_box as cb, bvh_new as B
    from light_transport_amd.src.light_samples import generate_area_light_samples
    from light_transport_amd.src.material import Material
    from light_transport_amd.src.path_tracing_old import render_scene
    from light_transport_amd.src.scene import Scene
    depth = 7.5
    surf = Material(color=K.WHITE_2, shininess=30, reflection=0.1, ior=1.521, transmission=1)
    src = Material(color=K.WHITE, shininess=1, reflection=0.9, ior=1.5, emission=200)
    lq = cb.get_light_quad(depth, src)
    objects = cb.get_cornell_box(depth, surf, surf, surf) + cb.get_cone(K.GLASS_MAT) + lq
    np.random.seed(1)
    lights = generate_area_light_samples(lq[0], lq[1], src, 40, 4)
    ordered, linear = B.build_linear_bvh(objects)
    np.random.seed(0)
    sc = Scene(camera=np.array([0, 0, depth + 0.5, 1.0]), lights=lights, width=24, height=16, max_depth=5,
               f_distance=depth, number_of_samples=3)
    sc.image[:] = 5.0
    img = render_scene(sc, ordered, linear, ctx=ctx)
    assert img is sc.image and img.shape == (16, 24, 3) and 0 < img.max() <= 1.0 and np.isinf(sc.rand_0).any()


def test_render_scene_object_api(ctx, golden_dir):
    """The reference-style call: Scene + primitives + linear BVH -> ndarray."""
    from light_transport_amd.src import constants as K, cornell_box as cb, bvh_new as B
    from light_transport_amd.src.material import Material, Color
    from light_transport_amd.src.light_samples import generate_area_light_samples
    from light_transport_amd.src.path_tracing_fix1 import render_scene
    from light_transport_amd.src.scene import Scene
    depth = 7.5
    white = Color(np.zeros(3), np.array([0.55, 0.55, 0.55]), np.array([0.7, 0.7, 0.7]))
    surf = Material(color=white, shininess=30, reflection=0.1, ior=1.521, transmission=1)
    src = Material(color=K.WHITE, shininess=1, reflection=0.9, ior=1.5, emission=200)
    lq = cb.get_light_quad(depth, src)
    objects = cb.get_cornell_box(depth, surf, surf, surf) + cb.get_cone(K.GLASS_MAT) + lq
    np.random.seed(1)
    lights = generate_area_light_samples(lq[0], lq[1], src, 40, 4)
    g8 = load(golden_dir, "g8_render_fix1.npz")
    np.testing.assert_allclose(np.array([l.source[:3] for l in lights]), g8["glass_lights"][:, :3], atol=1e-15)
    ordered, linear = B.build_linear_bvh(objects)
    np.random.seed(0)
    sc = Scene(camera=np.array([0, 0, depth + 0.5, 1.0]), lights=lights, width=24, height=16, max_depth=6,
               f_distance=depth, number_of_samples=2)
    img = render_scene(sc, ordered, linear, ctx=ctx)
    assert img is sc.image and img.shape == (16, 24, 3) and 0 < img.max() <= 0.25 and np.isinf(sc.rand_0).any()


# ---------------------------------------------------------------- f2: both renderers against the oracle on meshes of every size
# mesh in the box (tests/scenes.render_scene) -> (scene tables in LDS for k_render_surface, front-to-back link tables);
# both follow from the mesh's triangle and node counts and are asserted by every test that relies on them
RENDER_LADDER = {
    "cornell": (True, True),           # the notebook's cone: 28 triangles
    "ico2-below": (True, True),        # tables a few hundred bytes under the 48 KiB budget
    "ico2-above": (False, True),       # ... and a few hundred bytes over it
    "ico3": (False, True),             # 1298 triangles
    "teapot": (False, True),           # G10: 6338 triangles, a deep SAH tree from a real asset
    "wine-glass": (False, False),      # G10b: 25 364 triangles, more than 32767 nodes -- no 16-bit link tables
}
_render_scenes = {}


def render_ladder_scene(golden_dir, name, **kw):
    key = (name,) + tuple(sorted(kw.items()))
    if key not in _render_scenes:
        if name == "cornell":
            v, f = S.cone_mesh()
        elif name.startswith("ico2-"):
            v, f = S.icosphere(2)
            f = f[:123 if name == "ico2-below" else 124]        # a cap of the sphere, sized to straddle the LDS budget
        elif name == "ico3":
            v, f = S.icosphere(3)
        else:
            from tests.test_oracle_golden import _g10_file
            g, k = _g10_file(golden_dir, name)
            v, f = g[k + "_verts"], g[k + "_faces"]
        _render_scenes[key] = S.render_scene(v, f, **kw)
    return _render_scenes[key]


def render_kernel_of(sc):
    """(LDS tables, link tables) as launch_render_surface / bvh_octant_links decide them for this scene."""
    return S.render_table_bytes(sc["n_tris"], sc["n_nodes"]) <= S.RENDER_LDS_BUDGET, sc["n_nodes"] <= 32767


def bind_render_scene(ctx, sc):
    from light_transport_amd import _lib
    m = sc["mesh"]
    ctx.set_mesh(m["verts"], m["med_front"], m["med_back"], m["nodes"])
    ctx._mesh_key = None
    mats = (_lib.SurfaceMaterial * len(sc["mats"]))()
    for i, r in enumerate(sc["mats"]):
        mats[i].diffuse[:] = list(r[:3]); mats[i].emission, mats[i].ior, mats[i].transmission = r[3], r[4], r[5]
        mats[i].is_diffuse, mats[i].is_mirror, mats[i].is_light = int(r[6]), int(r[7]), int(r[8])
    lights = (_lib.PointLight * len(sc["lights"]))()
    for i, r in enumerate(sc["lights"]):
        lights[i].source[:] = list(r[:3]); lights[i].normal[:] = list(r[3:6]); lights[i].radiance[:] = list(r[6:9])
        lights[i].total_area = r[9]
    ctx.set_surface_materials(mats); ctx.set_lights(lights)


def render_both(ctx, sc, W, H, Sm, D, old=False, seed=0, choices=7):
    """One render of the bound scene on the device and in the oracle from the same seeded tables: the images and the
    +inf markers in rand_0 must agree (the walks' tolerance: |d| <= 1e-12 + 1e-9 |E|, zero pixels outside; markers
    exact), and every entry the render did not mark is returned unchanged.  -> (image, rand_0 after, tables)"""
    xs, ys, r0, r1, lc = S.render_tables(W, H, Sm, D, len(sc["lights"]), choices if old else None, seed)
    r0g, r0o = r0.copy(), r0.copy()
    img = np.full((H, W, 3), 9.0) if old else np.zeros((H, W, 3))       # old overwrites the image, fix1 adds to it
    imgo = np.zeros((H, W, 3))
    ctx.render_surface(sc["camera"], sc["f_distance"], xs, ys, r0g, r1, lc, img, old=old)
    osc = O.OracleScene([(0, 0, 0, 1)], (1, 1, 1), (0, 0, 0), (1, 1, 1), mesh=sc["mesh"])
    O.render_surface(osc, sc["mats"], sc["lights"], sc["camera"], sc["f_distance"], xs, ys, r0o, r1, lc, imgo, old=old)
    np.testing.assert_allclose(img, imgo, rtol=1e-9, atol=1e-12)
    marks = np.isinf(r0o)
    assert np.array_equal(np.isinf(r0g), marks)
    assert np.array_equal(r0g[~marks], r0[~marks])
    return img, r0g, (xs, ys, r0, r1, lc)


@pytest.mark.parametrize("variant", ["fix1", "old"])
@pytest.mark.parametrize("name", list(RENDER_LADDER))
def test_surface_render_across_mesh_sizes(ctx, golden_dir, name, variant):
    """lt_render_surface (k_render_surface, tables in LDS or in global memory) and lt_render_surface_old against the
    oracle's render on the same tables, from the 28-triangle cone to the 25 364-triangle wine glass whose BVH is too
    large for the front-to-back link tables (the renderers then search it in storage order).  Materials take every
    branch: diffuse, mirror, glass, light.  The object is checked to fill a real share of the picture."""
    sc = render_ladder_scene(golden_dir, name)
    lds, links = render_kernel_of(sc)
    assert (lds, links) == RENDER_LADDER[name], (S.render_table_bytes(sc["n_tris"], sc["n_nodes"]), sc["n_nodes"])
    bind_render_scene(ctx, sc)
    W, H, Sm, D = 24, 16, 2, 6
    img, r0, (xs, ys, r0_in, r1, lc) = render_both(ctx, sc, W, H, Sm, D, old=(variant == "old"), seed=11)
    o, d = S.camera_rays(sc, xs, ys, r0_in)
    p, _ = ctx.intersect_rays(o, d, None, 0)
    assert np.mean((p >= 0) & sc["is_object"][np.maximum(p, 0)]) >= 0.1, "the camera hardly sees the object"
    assert img.sum() > 1 and np.isinf(r0).any() and not np.isinf(r0).all()
    if variant == "fix1":       # the image is accumulated into (:166): a second render adds the same again
        img2 = img.copy()
        ctx.render_surface(sc["camera"], sc["f_distance"], xs, ys, r0_in.copy(), r1, lc, img2)
        np.testing.assert_allclose(img2, 2 * img, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("D", [1, 6])
@pytest.mark.parametrize("WH", [(1, 1), (13, 7), (300, 1)], ids=lambda wh: "%dx%d" % wh)
@pytest.mark.parametrize("Sm", [1, 3, 256, 300])
def test_surface_render_launch_shapes(ctx, golden_dir, Sm, WH, D):
    """k_render_surface's split of the work -- chunk = min(S, 256) samples of a pixel per round, 256 / chunk pixels per
    workgroup, one owner lane per pixel adding its samples -- at one sample, at sample counts that do not divide 256,
    beyond 256 (two rounds, one pixel per workgroup) and at pixel counts that are no multiple of the pixels per workgroup,
    against the oracle (tables in global memory, links present)."""
    sc = render_ladder_scene(golden_dir, "ico3")
    assert render_kernel_of(sc) == (False, True)
    bind_render_scene(ctx, sc)
    W, H = WH
    img, r0, _ = render_both(ctx, sc, W, H, Sm, D, seed=100 * Sm + W + D)
    assert img.sum() > 0


@pytest.mark.parametrize("D", [1, 24])
def test_recursive_render_shallowest_and_deepest(ctx, golden_dir, D):
    """lt_render_surface_old at max_depth 1 and at kRenderOldMaxDepth = 24, where the frame stack takes 137 KiB of LDS
    (the largest the kernel allows), against the oracle's real recursion on the 1298-triangle sphere."""
    sc = render_ladder_scene(golden_dir, "ico3")
    assert render_kernel_of(sc)[1]
    bind_render_scene(ctx, sc)
    img, r0, _ = render_both(ctx, sc, 16, 8, 2, D, old=True, seed=7 + D, choices=5)
    assert img.sum() > 0.1


@pytest.mark.parametrize("name", ["cornell", "ico2-below"])
def test_render_lds_tables_knob_changes_nothing(ctx, golden_dir, name):
    """lt_set_tuning("render_lds_tables", 0) makes lt_render_surface read the scene tables from global memory
    (k_render_surface<false>) where they would be staged in LDS: the two kernels differ only in where the tables live,
    so the images and markers are bit-identical -- the LDS kernel is pinned by G8, the global one to it."""
    sc = render_ladder_scene(golden_dir, name)
    assert render_kernel_of(sc) == (True, True)
    bind_render_scene(ctx, sc)
    img, r0, (xs, ys, r0_in, r1, lc) = render_both(ctx, sc, 24, 16, 3, 6, seed=31)
    img_g, r0_g = np.zeros_like(img), r0_in.copy()
    with ctx.tuning(render_lds_tables=0):
        ctx.render_surface(sc["camera"], sc["f_distance"], xs, ys, r0_g, r1, lc, img_g)
    assert np.array_equal(img_g, img) and np.array_equal(r0_g, r0)


@pytest.mark.parametrize("name", list(RENDER_LADDER))
def test_front_to_back_intersect_on_every_mesh(ctx, golden_dir, name):
    """lt_intersect_rays form 4 (the renderers' front-to-back search; the storage-order BVH where the mesh has no link
    tables) equals brute force -- prim and t exactly -- on every mesh of the ladder, with no reach, a random reach, and
    the reach set exactly at (the hit is excluded: t < tmax) and one ulp past each ray's nearest hit."""
    sc = render_ladder_scene(golden_dir, name)
    assert render_kernel_of(sc)[1] == RENDER_LADDER[name][1]
    m = sc["mesh"]
    ctx.set_mesh(m["verts"], m["med_front"], m["med_back"], m["nodes"])
    ctx._mesh_key = None
    rs = np.random.RandomState(17)
    n = 20000
    o = rs.uniform(-7.0, 7.0, size=(n, 3))
    d = rs.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    tgt = m["verts"][rs.randint(0, sc["n_tris"], n // 2)].mean(axis=1)      # half the rays aimed at a triangle's centre
    d[: n // 2] = tgt - o[: n // 2]; d[: n // 2] /= np.linalg.norm(d[: n // 2], axis=1, keepdims=True)
    p0, t0 = ctx.intersect_rays(o, d, None, 0)
    hit = p0 >= 0
    assert hit.mean() > 0.5 and np.mean(sc["is_object"][p0[hit]]) > 0.2
    reach = rs.exponential(3.0, n)
    at = np.where(hit, t0, reach)
    past = np.where(hit, np.nextafter(t0, np.inf), reach)
    for tm in (None, reach, at, past):
        pb, tb = ctx.intersect_rays(o, d, tm, 0)
        p4, t4 = ctx.intersect_rays(o, d, tm, 4)
        np.testing.assert_array_equal(p4, pb); np.testing.assert_array_equal(t4, tb)
        if tm is at:
            assert not np.any(pb[hit] == p0[hit])         # the nearest hit is just out of reach ...
        if tm is past:
            np.testing.assert_array_equal(pb, p0); np.testing.assert_array_equal(tb, t0)     # ... and just within it


# ---------------------------------------------------------------- f4: light sub-path vertices
@pytest.mark.parametrize("name", ["two_layer", "cornell"])
def test_light_subpath_vertices(ctx, name):
    """The walk stores the first K vertices of every path (role of random_walk / Vertex, bdpt.py:18-147,
    vertex.py:24-37); records must equal the oracle's, and capture must not disturb the tally."""
    prob = dict(two_layer=S.two_layer(n=32), cornell=S.cornell(32))[name]
    n, K = 3000, 12
    prob.apply(ctx, "f64")
    ctx.set_vertex_capture(K)
    ctx.launch(n, seed=31); ctx.sync()
    g, c = ctx.read_grid(), ctx.read_counters()
    v, cnt = ctx.read_vertices(n)
    ctx.set_vertex_capture(0)
    from light_transport_amd import _lib as _kinds
    go, co, vo, cnto = prob.oracle().run_capture(n, K, seed=31)
    check_counters(c, co, n)
    S.assert_grid_close(g, go)
    np.testing.assert_array_equal(cnt, cnto)
    assert cnt.max() == K and cnt.min() >= 1
    live = np.arange(K)[None, :] < cnt[:, None]
    for f in ("kind", "medium", "step"):
        np.testing.assert_array_equal(v[f][live], vo[f][live])
    np.testing.assert_allclose(v["point"][live], vo["point"][live], rtol=0, atol=1e-10)
    np.testing.assert_allclose(v["direction"][live], vo["direction"][live], rtol=0, atol=1e-11)
    np.testing.assert_allclose(v["throughput"][live], vo["throughput"][live], rtol=1e-12)
    # the fields the reference's walk fills (light_samples.py:100-114, bdpt.py:25-27,137): geometric normal, emission
    # densities, density of the outgoing direction
    np.testing.assert_allclose(v["g_norm"][live], vo["g_norm"][live], rtol=0, atol=1e-13)
    np.testing.assert_allclose(v["pdf_pos"][live], vo["pdf_pos"][live], rtol=1e-13)
    np.testing.assert_allclose(v["pdf_dir"][live], vo["pdf_dir"][live], rtol=1e-9, atol=1e-13)
    vol, dlt = v["kind"] == _kinds.VERTEX_VOLUME, (v["kind"] == _kinds.VERTEX_REFLECTIVE) | (v["kind"] == _kinds.VERTEX_TRANSMISSIVE)
    assert np.all(v["g_norm"][live & vol] == 0) and np.allclose(np.linalg.norm(v["g_norm"][live & dlt], axis=-1), 1.0)
    assert np.all((v["pdf_dir"][live & dlt] >= 0) & (v["pdf_dir"][live & dlt] <= 1))          # a branch probability
    if name == "cornell":      # quad light 2 x 2: pdf_pos = 1/4, pdf_dir = cos / pi about the normal (0, -1, 0)
        assert np.allclose(v["pdf_pos"][:, 0], 0.25)
        np.testing.assert_allclose(v["pdf_dir"][:, 0], -v["direction"][:, 0, 1] / np.pi, rtol=1e-12)
    else:                      # pencil beam: a delta source
        assert np.all(v["pdf_pos"][:, 0] == 1.0) and np.all(v["pdf_dir"][:, 0] == 1.0)
    # Henyey-Greenstein value of the deflection actually taken: cos = d_in . d_out between consecutive vertices
    from light_transport_amd.src.medium_samples import henyey_greenstein
    k0 = np.flatnonzero((cnt >= 3) & vol[:, 1] & (v["pdf_dir"][:, 1] > 0))[:200]
    cosd = np.einsum("ij,ij->i", v["direction"][k0, 1], v["direction"][k0, 2])
    gs = np.array([prob.media[m][2] for m in (v["medium"][k0, 1] if name == "cornell" else np.array(prob.layers["medium_idx"])[v["medium"][k0, 1]])])
    np.testing.assert_allclose(v["pdf_dir"][k0, 1], [henyey_greenstein(-c, g) for c, g in zip(cosd, gs)], rtol=1e-9)
    from light_transport_amd import _lib
    assert np.all(v["kind"][:, 0] == _lib.VERTEX_LIGHT) and np.all(v["step"][:, 0] == 0)
    kinds = set(np.unique(v["kind"][live]))
    assert _lib.VERTEX_VOLUME in kinds and (_lib.VERTEX_TRANSMISSIVE in kinds or _lib.VERTEX_REFLECTIVE in kinds)
    # object form
    from light_transport_amd.src import photon_tracing as PT
    tr = PT.PhotonTracer(ctx=ctx)
    paths = PT.generate_light_subpaths(tr, 50, 5, seed=31, as_objects=True)
    assert len(paths) == 50 and all(1 <= len(p) <= 5 for p in paths) and paths[0][0].hit_light
    np.testing.assert_allclose(paths[7][1].point, v["point"][7, 1], atol=1e-12)
    assert paths[7][1].pdf_fwd == paths[7][0].pdf_dir and (len(paths[7]) < 3 or paths[7][1].pdf_rev == paths[7][2].pdf_dir)
    from light_transport_amd.src.vertex import convert_density
    assert convert_density(paths[7][1].pdf_fwd, paths[7][0], paths[7][1]) > 0
    with pytest.raises(Exception):
        ctx.read_vertices(n)       # nothing captured by the last launch
    # a capture size changed AFTER the capturing launch must not resize the read (it would read out of bounds)
    prob.apply(ctx, "f64"); ctx.set_vertex_capture(4); ctx.launch(100, seed=31); ctx.sync()
    ctx.set_vertex_capture(9)
    with pytest.raises(Exception):
        ctx.read_vertices(100)
    ctx.set_vertex_capture(4)
    v4, cnt4 = ctx.read_vertices(100)
    assert v4.shape == (100, 4) and np.array_equal(v4["point"][:, :4][cnt4[:, None] > np.arange(4)[None, :]],
                                                    v["point"][:100, :4][cnt4[:, None] > np.arange(4)[None, :]])
    ctx.set_vertex_capture(0)


# ---------------------------------------------------------------- the two deposition paths
def test_log_tally_equals_atomic_tally(ctx):
    """LT_MODE_LOG (deposit log -> tile partition -> LDS reduce) against LT_MODE_ATOMIC: bit-identical fixed-point
    grids -- with an ample log (one batch), with a log budget that forces several batches, with one so small that
    most records overflow to the atomic fallback, with the batches alternating between two or three lanes of the ctx
    (lt_set_overlap), with the two-pass partition forced on a small grid (hot-tile form and plain), and on a grid whose size is not a
    multiple of the 16384-voxel tile; float tallies equal up to summation order.  Every regime is checked to have
    really been exercised (batches, overflow, lanes reported by lt_last_log_info).  Fresh contexts: a log budget
    smaller than an earlier allocation must be honoured all the same."""
    import light_transport_amd as lt
    odd = S.Problem([(0.1, 10.0, 0.9, 1.0)], (100, 70, 33), (-5.0, -3.5, 0.0), (0.1,) * 3,
                    layers=dict(z_bounds=[0.0, np.inf], medium_idx=[0]))
    big = S.Problem([(0.1, 10.0, 0.9, 1.0)], (300, 300, 200), (-15.0, -15.0, 0.0), (0.1,) * 3,
                    layers=dict(z_bounds=[0.0, np.inf], medium_idx=[0]))   # 1300 tiles: two-pass partition
    # (mode, log budget, lanes, knob log_bits2, knob log_hot): the two-pass form runs with the hot tiles the pilot batch
    # finds (default), with a handful of them, and without (plain two passes)
    regimes = (("atomic", 0, 1, None, None), ("log", 8 << 30, 1, None, None), ("log", 48 << 20, 1, None, None),
               ("log", 4 << 20, 1, None, None), ("log", 8 << 30, 2, None, None), ("log", 48 << 20, 2, None, "0"),
               ("log", 8 << 30, 3, None, "5"), ("log", 8 << 30, 1, "3", None), ("log", 48 << 20, 2, "2", None),
               ("log", 8 << 30, 1, "3", "0"), ("log", 48 << 20, 3, "2", "3"),
               ("log", 4 << 20, 2, None, None))     # a budget that holds ONE lane's minimum log, not two: the launch must fall back to one lane
    for prob, n in ((S.slab(), 300000), (odd, 300000), (S.cornell(64), 100000), (big, 300000)):
        grids = {}
        c2 = lt.Context(0)        # ample logs first on the session ctx, small budgets later: both orders are covered
        for k, (mode, log_bytes, lanes, bits2, hot) in enumerate(regimes):
            cx = ctx if k % 2 == 0 else c2
            knobs = {k: int(v) for k, v in (("log_bits2", bits2), ("log_hot", hot)) if v is not None}
            with cx.tuning(**knobs):
                prob.apply(cx, "u64fx"); cx.set_tally_mode(mode, log_bytes); cx.set_overlap(lanes)
                cx.launch(n, seed=5); cx.sync()
            grids[(mode, log_bytes, lanes, bits2, hot)] = (cx.read_grid_raw(), cx.read_counters())
            info = cx.last_log_info()
            if mode == "atomic":
                assert info is None
                continue
            want_lanes = 1 if (log_bytes == 4 << 20 and lanes == 2) else lanes
            assert info["lanes"] == want_lanes and info["records"] + info["overflow_records"] > 50 * n
            if log_bytes == 4 << 20:
                assert info["overflow_records"] > 0      # such a log overflows: every wave meets the exhausted state
            two_pass = bits2 is not None or prob is big
            n_hot = cx.last_log_hot_tiles()[0]
            if not two_pass or hot == "0":
                assert n_hot == 0
            elif hot is not None:
                assert n_hot == int(hot)                    # (more than that many tiles hold records)
            else:
                assert n_hot >= 16
            if log_bytes == 8 << 30:
                assert info["overflow_records"] == 0 and info["batches"] <= (2 if lanes == 1 else 12)   # (+ the pilot)
            if log_bytes == 48 << 20:
                assert info["batches"] >= 4, info
            if log_bytes == 4 << 20:
                assert info["overflow_records"] > info["records"], info       # most deposits took the atomic fallback
        c2.close()
        ref, cref = grids[("atomic", 0, 1, None, None)]
        for k, (g, c) in grids.items():
            assert np.array_equal(g, ref), k
            assert c["steps"] == cref["steps"] and c["photons"] == n
        ctx.set_overlap(0)
        for dtype in ("f64", "f32"):
            prob.apply(ctx, dtype); ctx.set_tally_mode("atomic"); ctx.launch(n, seed=5, f32_walk=dtype == "f32"); ctx.sync()
            a = ctx.read_grid()
            for lanes in (1, 2):
                prob.apply(ctx, dtype); ctx.set_tally_mode("log", 8 << 30); ctx.set_overlap(lanes)
                ctx.launch(n, seed=5, f32_walk=dtype == "f32"); ctx.sync()
                b = ctx.read_grid()
                tol = 1e-11 if dtype == "f64" else 2e-3   # f32 sums of ~1e-2 deposits onto ~2e3: order matters at 1e-3
                assert np.abs(a - b).max() <= tol * a.max()
            ctx.set_overlap(0)
    ctx.set_tally_mode("auto", 0)


def test_config5_geometry_512_cubed(ctx):
    """BASELINE config 5 at its own shape: two-layer skin model on a 512^3 grid of 0.025 mm voxels (8192 tiles:
    two-pass partition with 64 level-1 bins and up to 960 hot tiles, tile counting, 1 GiB of u64 tally).  (a) <= 2e4
    photons: fixed-point grid and step count equal the CPU oracle's bit for bit; (b) 2e6 photons: log == atomic bit for
    bit, one lane == two == three lanes, hot-tile form == plain two-pass form, energy conservation, one launch == three
    ragged shards; the photon ids of (b) are those a rank of the 8-GPU run would trace (offset 3 * 1.25e7)."""
    prob = S.two_layer(n=512, voxel=0.025)
    n = 20000
    prob.apply(ctx, "u64fx"); ctx.set_tally_mode("log")
    ctx.launch(n, seed=11); ctx.sync()
    fx, c = ctx.read_grid_raw(), ctx.read_counters()
    assert ctx.last_log_info() is not None
    _, fxo, co = prob.oracle().run(n, seed=11, threads=8, want_fx=True, want_f64=False)
    check_counters(c, co, n)
    assert np.array_equal(fx, fxo) and fx.sum() > 0
    del fxo
    n, off = 2 * 10 ** 6, 3 * 12500000
    grids = {}
    for mode, lanes, hot in (("atomic", 1, None), ("log", 1, None), ("log", 2, None), ("log", 1, "0"), ("log", 3, "100")):
        with ctx.tuning(**({"log_hot": int(hot)} if hot is not None else {})):
            prob.apply(ctx, "u64fx"); ctx.set_tally_mode(mode); ctx.set_overlap(lanes)
            ctx.launch(n, seed=12, photon_offset=off); ctx.sync()
        grids[(mode, lanes, hot)] = (ctx.read_grid_raw(), ctx.read_counters())
        if mode == "log":
            info = ctx.last_log_info()
            assert info["lanes"] == lanes and info["overflow_records"] == 0, info
            n_hot = ctx.last_log_hot_tiles()[0]      # 8192 tiles, 64 level-1 bins: up to 960 hot tiles
            assert (n_hot == int(hot)) if hot is not None else (900 <= n_hot <= 960), n_hot
    ref, cref = grids[("atomic", 1, None)]
    assert cref["photons"] == n and abs(O.conservation_residual(cref)) < 1e-9 * n
    assert abs(float(ref.sum()) / O.FX_SCALE - cref["w_absorbed"]) < 1e-6 * n
    for k, (g, c) in grids.items():
        assert np.array_equal(g, ref), k
        assert c["steps"] == cref["steps"]
    del grids
    ctx.set_tally_mode("log"); ctx.set_overlap(0); ctx.zero_tally()
    for o2, cnt in ((0, 345678), (345678, 1000001), (1345679, n - 1345679)):
        ctx.launch(cnt, seed=12, photon_offset=off + o2)
    ctx.sync()
    assert np.array_equal(ctx.read_grid_raw(), ref) and ctx.read_counters()["steps"] == cref["steps"]
    ctx.set_tally_mode("auto", 0)
    ctx.set_grid((8, 8, 8), (0, 0, 0), (1, 1, 1), "f64")     # release the 1 GiB grid of the session ctx


def test_one_pass_partition_on_ragged_logs_equals_the_atomic_tally(ctx):
    """The one-pass log partition (k_log_part straight to tiles) against the atomic tally: bit-identical fixed-point grids and
    equal step counts -- ample log, a log budget that forces several batches (short last chunks, chunks nobody claimed), two
    lanes, a grid that is not a multiple of the tile, a mesh scene, and a launch so small that most items are ragged."""
    odd = S.Problem([(0.1, 10.0, 0.9, 1.0)], (100, 70, 33), (-5.0, -3.5, 0.0), (0.1,) * 3,
                    layers=dict(z_bounds=[0.0, np.inf], medium_idx=[0]))
    for prob, n in ((S.slab(), 300000), (odd, 300000), (S.cornell(64), 100000), (S.slab(), 700)):
        prob.apply(ctx, "u64fx"); ctx.set_tally_mode("atomic"); ctx.set_overlap(1)
        ctx.launch(n, seed=11); ctx.sync()
        ref, cref = ctx.read_grid_raw(), ctx.read_counters()
        for log_bytes, lanes in ((8 << 30, 1), (48 << 20, 1), (8 << 30, 2), (48 << 20, 2)):
            prob.apply(ctx, "u64fx"); ctx.set_tally_mode("log", log_bytes); ctx.set_overlap(lanes)
            ctx.launch(n, seed=11); ctx.sync()
            g, c, info = ctx.read_grid_raw(), ctx.read_counters(), ctx.last_log_info()
            assert info is not None and info["records"] > 0, (log_bytes, lanes)
            assert np.array_equal(g, ref), (n, log_bytes, lanes)
            assert c["steps"] == cref["steps"]
    ctx.set_overlap(0); ctx.set_tally_mode("auto")


def test_retired_tuning_keys_are_unknown(ctx):
    """lt_set_tuning refuses the keys whose code is gone (the LDS-staged partition's, the march grid's print and cell scale) and
    still takes their neighbours."""
    import light_transport_amd as lt
    for k in ("part_lds", "march_info", "march_scale_milli"):
        with pytest.raises(lt.LtError):
            ctx.set_tuning(k, 1)
    try:
        for k in ("tail_split", "march_cells"):
            ctx.set_tuning(k, 1)
    finally:
        for k in ("tail_split", "march_cells"):
            ctx.set_tuning(k, -1)


def test_tail_split_changes_nothing_but_the_route(ctx):
    """Slab walks in log mode end their walk kernel early and finish the last photons of every wave in a second kernel beside
    the log reduction (lt_walk_kernel.inc "Tail split").  Off (knob 0), default, and forced with thresholds 16 / 48 (a wave hands over when at
    most that many lanes are alive): identical u64 grids and step counts on the slab, the two-layer and the Cornell scene, one and two lanes -- and the
    number of deposit records that went through the LOG differs, which proves photons really took the other route (their
    deposits reach the grid as atomics from the tail kernel)."""
    for prob in (S.slab(), S.two_layer(), S.cornell(48)):      # (the Cornell scene: walk_kernel_q hands over steps that wait for a surface query too)
        for lanes in (1, 2):
            seen = {}
            for knob in (0, -1, 16, 48):       # off / default / forced with thresholds 16 and 48
                with ctx.tuning(tail_split=knob):
                    prob.apply(ctx, "u64fx"); ctx.set_tally_mode("log"); ctx.set_overlap(lanes)
                    ctx.launch(600000, seed=31); ctx.sync()
                g, c, info = ctx.read_grid_raw(), ctx.read_counters(), ctx.last_log_info()
                seen[knob] = (g, c["steps"], info["records"] + info["overflow_records"])
            for knob in (-1, 16, 48):
                assert seen[knob][1] == seen[0][1] and np.array_equal(seen[knob][0], seen[0][0]), (lanes, knob)
            assert seen[48][2] < seen[16][2] < seen[0][2], (lanes, [v[2] for v in seen.values()])
            # the DEFAULT does not split a launch this small (146 photons per wave: it would be "all tail", atomics for most
            # deposits): every record goes through the log, as with the split off
            # (record counts of two identical launches differ by a few: which photons share a lane -- and so which consecutive
            #  same-voxel deposits the run-length accumulator merges -- depends on scheduling; a split moves millions)
            assert abs(seen[-1][2] - seen[0][2]) <= 1e-5 * seen[0][2] and seen[16][2] < 0.99 * seen[0][2], (lanes, [v[2] for v in seen.values()])
    ctx.set_tally_mode("auto"); ctx.set_overlap(0)


def test_overlap_auto_tries_both_regimes_then_keeps_one(ctx):
    """lt_set_overlap(0): launches of >= 2^21 photons whose geometry is not pinned run once with two lanes, once with
    one, then with whichever took less device time per photon; results do not depend on it (bit-identical u64 grids)."""
    prob = S.slab(n=128, voxel=0.2)
    n = (1 << 21) + 20000
    prob.apply(ctx, "u64fx"); ctx.set_tally_mode("log"); ctx.set_overlap(0)
    lanes, grids = [], []
    for k in range(5):
        ctx.zero_tally(); ctx.launch(n, seed=3); ctx.sync()
        lanes.append(ctx.last_log_info()["lanes"]); grids.append(ctx.read_grid_raw())
    # (the first launch of a scene starts with the pilot batch: not a clean timing, so two lanes are measured again)
    assert lanes[:3] == [2, 2, 1] and lanes[3] == lanes[4] and lanes[3] in (1, 2), lanes
    assert all(np.array_equal(g, grids[0]) for g in grids[1:])
    ctx.set_launch_config(4, 256)            # a pinned geometry keeps one lane
    ctx.zero_tally(); ctx.launch(n, seed=3); ctx.sync()
    assert ctx.last_log_info()["lanes"] == 1 and np.array_equal(ctx.read_grid_raw(), grids[0])
    ctx.set_launch_config(0, 0)
    ctx.zero_tally(); ctx.launch(100000, seed=3); ctx.sync()          # small launches stay on one lane
    assert ctx.last_log_info()["lanes"] == 1
    ctx.set_tally_mode("auto", 0)


# ---------------------------------------------------------------- several jobs in flight on one GPU
def test_job_pipeline_matches_single_context(ctx):
    """Two contexts taking jobs in turn (light_transport_amd.JobPipeline, what bench.py --inflight 2 does) return, in
    order, exactly the fixed-point grids and counters one context produces job by job -- and the oracle's for job 0."""
    from light_transport_amd import JobPipeline
    prob = S.two_layer(n=32)
    jobs = [dict(n_photons=3000 + 500 * k, seed=40 + k, photon_offset=1000 * k, tag=k) for k in range(5)]

    def configure(c):
        prob.apply(c, "u64fx")
        c.set_tally_mode(1)            # log tally: walk + partition + reduce per job, the kernels that overlap

    pipe = JobPipeline(configure, depth=2, raw=True)
    got = list(pipe.run(jobs))
    pipe.close()
    assert [t for t, _, _ in got] == [0, 1, 2, 3, 4]
    configure(ctx)
    for (tag, grid, cnt), j in zip(got, jobs):
        ctx.zero_tally(); ctx.launch(j["n_photons"], seed=j["seed"], photon_offset=j["photon_offset"]); ctx.sync()
        assert np.array_equal(grid, ctx.read_grid_raw()), "job %d differs from the single-context run" % tag
        c1 = ctx.read_counters()
        assert cnt["steps"] == c1["steps"] and cnt["photons"] == j["n_photons"]
        assert abs(cnt["w_absorbed"] - c1["w_absorbed"]) < 1e-9 * j["n_photons"]
    ctx.set_tally_mode(2)
    _, fxo, co = prob.oracle().run(jobs[0]["n_photons"], seed=jobs[0]["seed"], threads=8, want_fx=True, want_f64=False)
    assert np.array_equal(got[0][1], fxo) and got[0][2]["steps"] == co["steps"]


# ---------------------------------------------------------------- literature known answers at GPU sizes
def test_published_values_at_gpu_scale(ctx):
    """The known answers that pin the volumetric walk (tests/test_oracle_golden.py), at photon counts only the GPU
    reaches in test time: van de Hulst's exact values as quoted by Wang-Jacques-Zheng 1995 -- Table 1, matched slab:
    Rd = 0.09739, Tt = 0.66096; Table 2, mismatched semi-infinite isotropic medium: total R = 0.26000.  At 4e7 photons
    the statistical sigma is 5e-5 (Rd) / 7e-5 (Tt): this is the test that exposed the seed-only XORWOW initialisation
    (9e-5 off, profiles/r01e_rng_seeding.log).  The f32 walk carries a rounding bias of ~2e-4 on this 0.02 cm slab."""
    n = 4 * 10 ** 7
    prob = S.slab(media=((10.0, 90.0, 0.75, 1.0),), thickness=0.02, n=8, voxel=0.0025)
    for f32, tally, tol in ((False, "f64", 2e-4), (True, "f32", 5e-4)):
        prob.apply(ctx, tally)
        ctx.zero_tally(); ctx.launch(n, seed=21, f32_walk=f32); ctx.sync()
        c = ctx.read_counters()
        assert abs(c["w_escaped_top"] / n - 0.09739) < tol, c["w_escaped_top"] / n
        assert abs(c["w_escaped_bottom"] / n - 0.66096) < tol, c["w_escaped_bottom"] / n
        tot = sum(c[k] for k in ("w_absorbed", "w_lost_outside_grid", "w_escaped_top", "w_escaped_bottom", "w_specular",
                                 "w_roulette_net", "w_capped", "w_escaped_mesh"))
        assert abs(tot - n) < (1e-9 if not f32 else 2e-3) * n
    prob = S.slab(media=((10.0, 90.0, 0.0, 1.5),), n=8, voxel=1.0)
    prob.apply(ctx, "f64")
    ctx.zero_tally(); ctx.launch(n, seed=22); ctx.sync()
    c = ctx.read_counters()
    assert abs(c["w_specular"] / n - 0.04) < 1e-12
    assert abs((c["w_escaped_top"] + c["w_specular"]) / n - 0.26000) < 2.5e-4, (c["w_escaped_top"] + c["w_specular"]) / n
    # Table 3 of the same paper: three mismatched layers (n = 1.37 in air); the published numbers are Monte Carlo
    # results themselves -- MCML 0.2375 / 0.0965, Gardner et al. 0.2381 / 0.0974 -- so three digits is the claim
    three = S.Problem([(1.0, 100.0, 0.9, 1.37), (1.0, 10.0, 0.0, 1.37), (2.0, 10.0, 0.7, 1.37)], (8, 8, 8),
                      (-1.0, -1.0, 0.0), (0.25, 0.25, 0.05),
                      layers=dict(z_bounds=[0.0, 0.1, 0.2, 0.4], medium_idx=[0, 1, 2], n_above=1.0, n_below=1.0))
    three.apply(ctx, "f64")
    n3 = 10 ** 7
    ctx.zero_tally(); ctx.launch(n3, seed=23); ctx.sync()
    c = ctx.read_counters()
    assert abs(c["w_specular"] / n3 - (0.37 / 2.37) ** 2) < 1e-12
    assert abs(c["w_escaped_top"] / n3 - 0.2378) < 1.0e-3 and abs(c["w_escaped_bottom"] / n3 - 0.0965) < 1.2e-3


# ---------------------------------------------------------------- randomised scenes
def test_random_layered_scenes_match_oracle(ctx):
    """Thirty random layered problems (1-4 layers, matched and mismatched indices, thin and thick, odd grids, beams
    that start inside the stack or tilted), both tally paths: fixed-point tallies and step counts equal the oracle's."""
    rs = np.random.RandomState(2025)
    for case in range(30):
        nl = int(rs.randint(1, 5))
        media = [(float(rs.uniform(0.01, 2.0)), float(rs.uniform(0.5, 60.0)), float(rs.choice([0.0, 0.3, 0.8, 0.95, -0.4])),
                  float(rs.choice([1.0, 1.33, 1.4, 1.5]))) for _ in range(nl)]
        thick = rs.uniform(0.02, 0.6, size=nl)
        zb = np.concatenate([[0.0], np.cumsum(thick)])
        if rs.rand() < 0.4:
            zb[-1] = np.inf
        shape = tuple(int(x) for x in rs.randint(1, 41, size=3))
        voxel = tuple(float(x) for x in rs.uniform(0.01, 0.2, size=3))
        origin = (-shape[0] * voxel[0] / 2 + float(rs.uniform(-0.05, 0.05)), -shape[1] * voxel[1] / 2, float(rs.uniform(-0.05, 0.05)))
        d = np.array([rs.uniform(-0.4, 0.4), rs.uniform(-0.4, 0.4), 1.0]); d /= np.linalg.norm(d)
        z0 = 0.0 if rs.rand() < 0.5 else float(rs.uniform(0.0, float(np.sum(thick))) * 0.9)
        src = dict(type=0, pos=(float(rs.uniform(-0.1, 0.1)), 0.0, z0), dir=tuple(float(x) for x in d), extra=(0.0,) * 6,
                   start_medium=0)
        prob = S.Problem(media, shape, origin, voxel, source=src, max_steps=int(rs.choice([1000000, 300])),
                         layers=dict(z_bounds=zb, medium_idx=list(rs.permutation(nl)), n_above=float(rs.choice([1.0, 1.33])),
                                     n_below=float(rs.choice([1.0, 1.5]))))
        n = int(rs.randint(1, 1500))
        _, fxo, co = prob.oracle().run(n, seed=case, threads=4, want_fx=True, want_f64=False)
        for mode in ("atomic", "log"):
            prob.apply(ctx, "u64fx"); ctx.set_tally_mode(mode)
            ctx.zero_tally(); ctx.launch(n, seed=case); ctx.sync()
            c = ctx.read_counters()
            assert c["steps"] == co["steps"], (case, mode, c["steps"], co["steps"])
            assert np.array_equal(ctx.read_grid_raw().reshape(-1), fxo.reshape(-1)), (case, mode)
            for k in ("w_absorbed", "w_escaped_top", "w_escaped_bottom", "w_specular", "w_capped", "w_lost_outside_grid"):
                assert abs(c[k] - co[k]) < 1e-9 * max(1, n), (case, mode, k, c[k], co[k])
    ctx.set_tally_mode(2)


def test_surface_query_shortcuts_do_not_change_results(ctx):
    """Every shortcut of the mesh walks is a shortcut, not an approximation: u64 grids and step counts are identical bit for
    bit with each of them varied or switched off (lt_set_tuning).
    Cornell cavity + cone (30 triangles in LDS, walk_kernel_q): near-triangle lists off; clearance grid off altogether (every
    step queries the BVH); a coarse / a fine clearance grid; query services that wait for 1 or for all 64 lanes.
    5140-triangle sphere (tables in global memory, walk_kernel_m): march grid of 16 / 200 cells; no march grid (walk_kernel_q
    over the BVH, no clearance at all); candidate queue drained as soon as 1 / only when 64 answered queries wait."""
    cornell_variants = ({}, {"no_near_lists": 1}, {"no_clearance": 1}, {"clearance_cells": 16}, {"clearance_cells": 200},
                        {"query_min": 1}, {"query_min": 64})
    sphere_variants = ({}, {"march_cells": 16}, {"march_cells": 200}, {"no_march": 1}, {"query_min": 1}, {"query_min": 64})
    cornell_prob = S.cornell(64)
    for prob, n, variants in ((cornell_prob, 200000, cornell_variants), (S.sphere_in_box(4, split_method=0)[0], 60000, sphere_variants)):
        ref = None
        for knobs in variants:
            with ctx.tuning(**knobs):
                prob.apply(ctx, "u64fx"); ctx.set_tally_mode("atomic")
                ctx.launch(n, seed=21); ctx.sync()
                info = ctx.mesh_accel_info()
            # the variant really ran: the acceleration data is what the knob asks for
            if "march_cells" in knobs:
                assert max(info["march_dims"]) == knobs["march_cells"] + 2, info
            if "clearance_cells" in knobs:
                assert max(info["clearance_dims"]) == knobs["clearance_cells"], info
            if "no_march" in knobs or "no_clearance" in knobs:
                assert info["kind"] == 0, info
            if not knobs:
                assert info["kind"] == (2 if prob is not cornell_prob else 1), info
            g, c = ctx.read_grid_raw(), ctx.read_counters()
            if ref is None:
                ref = (g, c)
                assert c["w_escaped_mesh"] > 0 and g.sum() > 0
            assert c["steps"] == ref[1]["steps"] and np.array_equal(g, ref[0]), knobs
    ctx.set_tally_mode(2)


def test_random_mesh_scenes_match_oracle(ctx):
    """Randomised closed-box + sphere scenes (sphere size, position, tessellation, media, indices, source, BVH split
    method drawn at random), both tally paths, f64 walk: fixed-point tallies and step counts equal the oracle's.  These
    run through walk_kernel_q, whose lanes wait for one another before a BVH query."""
    from light_transport_amd.src.io import triangles_from_mesh
    from light_transport_amd.src import cornell_box as cb, constants as K, bvh_new as B
    rs = np.random.RandomState(77)
    for case in range(10):
        dim = float(rs.uniform(1.0, 5.0))
        walls = cb.get_cornell_box(dim, K.GLASS_MAT, K.GLASS_MAT, K.GLASS_MAT) + cb.get_front_wall(dim, K.GLASS_MAT) \
            + cb.get_light_quad(dim, K.GLASS_MAT)
        for t in walls:
            t.med_front, t.med_back = 0, -1
        radius = float(rs.uniform(0.2, 0.45)) * dim
        centre = tuple(float(x) for x in rs.uniform(-0.4, 0.4, size=3) * dim)
        vs, fs = S.icosphere(int(rs.randint(0, 3)), radius, centre)
        ball = triangles_from_mesh(vs, fs, K.GLASS_MAT)
        for t in ball:
            t.med_front, t.med_back = 0, 1
        ordered, linear = B.build_linear_bvh(walls + ball, int(rs.randint(0, 2)))
        mesh = dict(verts=B.triangles_array(ordered), med_front=np.array([t.med_front for t in ordered], np.int32),
                    med_back=np.array([t.med_back for t in ordered], np.int32), nodes=B.linear_bvh_arrays(linear))
        media = [(float(rs.uniform(0.02, 0.5)), float(rs.uniform(1.0, 20.0)), float(rs.choice([0.0, 0.8, 0.9])), 1.0),
                 (float(rs.uniform(0.1, 2.0)), float(rs.uniform(1.0, 30.0)), float(rs.choice([0.0, 0.7, 0.95])),
                  float(rs.choice([1.0, 1.37, 1.5])))]
        if rs.rand() < 0.5:
            src = dict(type=1, pos=(-0.25 * dim, dim, -0.25 * dim), dir=(0.0, -1.0, 0.0),
                       extra=(0.5 * dim, 0.0, 0.0, 0.0, 0.0, 0.5 * dim), start_medium=0)
        else:
            d = rs.normal(size=3); d /= np.linalg.norm(d)
            src = dict(type=0, pos=(0.9 * dim * float(rs.uniform(-1, 1)), -0.95 * dim, 0.0), dir=tuple(float(x) for x in d),
                       extra=(0.0,) * 6, start_medium=0)
        ng = int(rs.randint(8, 40))
        prob = S.Problem(media, (ng, ng, ng), (-dim,) * 3, (2 * dim / ng,) * 3, mesh=mesh, source=src)
        n = int(rs.randint(200, 2500))
        _, fxo, co = prob.oracle().run(n, seed=100 + case, threads=4, want_fx=True, want_f64=False)
        for mode in ("atomic", "log"):
            prob.apply(ctx, "u64fx"); ctx.set_tally_mode(mode)
            ctx.zero_tally(); ctx.launch(n, seed=100 + case); ctx.sync()
            c = ctx.read_counters()
            assert c["steps"] == co["steps"], (case, mode, c["steps"], co["steps"])
            assert np.array_equal(ctx.read_grid_raw().reshape(-1), fxo.reshape(-1)), (case, mode)
            assert abs(c["w_escaped_mesh"] - co["w_escaped_mesh"]) < 1e-9 * n and abs(c["w_absorbed"] - co["w_absorbed"]) < 1e-9 * n
    ctx.set_tally_mode(2)
