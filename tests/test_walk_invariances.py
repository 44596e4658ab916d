"""Exact invariances of the walks: other units, other frames, and every shortcut of the f32 mesh walks.

Nothing here compares an f32 device run with an f32 CPU run (trajectories flip on 1-ulp libm differences): the device is
compared with ITSELF bit for bit (photon streams are seeded per photon id and the f32 walk can deposit into the u64 fixed-point
tally, so two runs of one scene must agree exactly whichever shortcut answered the surface queries), or the f64 walk with the
f64 oracle.

  * the layered walk has no absolute length in it: a rescale by a power of two leaves its u64 tally, step count and counters
    bit-identical, in f64 and in f32 -- pinned on the oracle first (CPU), then asked of every slab build of the device;
  * the mesh walks do have absolute constants (EPSILON 1e-6, the pre-test's `behind`, f16 clearances that saturate at 65504,
    grid and tile index arithmetic at large origins): the f64 walk must equal the oracle -- which has none of the shortcuts --
    at 2^10, 2^-10, 2^14, shifted by ~1e3 and by ~1e6;
  * the plane pre-test (plane_within_reach) may only reject a hop that the triangle test would not have accepted: queried pair
    by pair through lt_eval(LT_FN_PLANE_REACH), 2^20 hops per case that end just beyond a triangle's plane;
  * the f32 mesh walks give the same tally with every shortcut on, off or retuned.

No test excepts a voxel, a photon or a query.
"""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import scenes as S
from tests.test_gpu_parity import check_counters
from tests.test_layer_record import three_layers

SEED = 7

# ---------------------------------------------------------------- scenes
LAYERED = dict(
    slab=lambda: S.slab(n=32, voxel=0.8),
    two_layer=lambda: S.two_layer(n=32),
    thin_mismatched=lambda: S.slab(media=((1.0, 9.0, 0.75, 1.4),), thickness=0.5, n=32, voxel=0.05, n_above=1.0, n_below=1.5),
    three_layers=three_layers,
)
EXPONENTS = (-20, -10, 10, 20)
SHIFT = (1000.5, -2000.25, 512.125)

# mesh scenes and what accelerates them (lt_mesh_accel_info kind): 30 and 100 triangles in LDS (1); 260 -- three balls of 80 --
# with the f32 tables in LDS and the f64 ones beyond it (3; the 340 triangles of sphere_in_box(2) are beyond LDS in f32 too: 68 KB);
# 1300 beyond LDS in both precisions (2: march grid)
MESH = dict(cornell=1, ball1=1, three_balls=3, ball3=2)
THREE_BALLS = ((0.9, (1.6, -1.2, 0.9)), (0.9, (-1.5, 1.0, -1.1)), (0.9, (0.2, -1.8, -2.0)))
TRANSFORMS = dict(up10=(2.0 ** 10, (0.0, 0.0, 0.0)), down10=(2.0 ** -10, (0.0, 0.0, 0.0)),
                  up14=(2.0 ** 14, (0.0, 0.0, 0.0)),       # clearances pass 65504: half_down clamps
                  shift=(1.0, SHIFT), up10_shift=(2.0 ** 10, (1e6, -2e6, 5e5)))
F32_SCALES = dict(one=1.0, up10=2.0 ** 10, down10=2.0 ** -10)
N_MESH = 20000
N_F32 = 50000
# step cap of the f32 mesh runs.  At scale 1 and 2^-10 few photons reach it.  At 2^10 the f32 walk is past its resolution (an ulp
# of a coordinate is 5e-4, EPSILON 1e-6: a photon re-hits the facet it stands on) and single photons live for 10^5 steps, one
# lane each; capped, with their weight counted, every route still has to take the same 2e8 steps
F32_MAX_STEPS = 4000
N_LAYERED = 20000


@functools.lru_cache(maxsize=None)
def mesh_scene(name):
    """Built once, shared, never modified."""
    if name == "cornell":
        return S.cornell(24)
    if name == "three_balls":
        return S.sphere_in_box(1, n=24, balls=THREE_BALLS)[0]
    return S.sphere_in_box(int(name[-1]), n=24)[0]


@functools.lru_cache(maxsize=None)
def mesh_case(name, tf):
    return S.transformed(mesh_scene(name), *TRANSFORMS[tf])


@functools.lru_cache(maxsize=None)
def mesh_oracle(name, tf):
    """(u64 grid, counters) of the f64 oracle at the transformed problem: once per case, shared by the CPU and the GPU test."""
    _, fx, c = mesh_case(name, tf).oracle().run(N_MESH, seed=SEED, threads=8, want_fx=True, want_f64=False)
    fx.setflags(write=False)
    return fx, c


def dense(prob):
    """The same mesh, a hundred times denser (hops of 1e-4 of the scene), lit by a pencil beam that starts 0.05 outside the
    largest tilted facet of the inner body (cone / ball: med_back = 1) and is aimed at it -- at a point well inside the facet
    and slightly off its normal: the f32 triangle test is not watertight on a shared edge."""
    v = prob.mesh["verts"]
    ab, ac = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    nn = np.cross(ab, ac)
    area = np.linalg.norm(nn, axis=1)
    nn = nn / area[:, None]
    tilted = (prob.mesh["med_back"] == 1) & (np.sort(np.abs(nn), axis=1)[:, 1] > 0.2)      # two components: no axis-aligned facet
    k = int(np.argmax(np.where(tilted, area, 0.0)))
    assert tilted[k]
    p = 0.5 * v[k, 0] + 0.3 * v[k, 1] + 0.2 * v[k, 2]
    d = -nn[k] + 0.15 * ab[k] / np.linalg.norm(ab[k])
    d /= np.linalg.norm(d)
    src = dict(type=0, pos=tuple(p + 0.05 * nn[k]), dir=tuple(d), extra=(0.0,) * 6, start_medium=0)
    media = [(m[0] * 100.0, m[1] * 100.0, m[2], m[3]) for m in prob.media]
    return S.Problem(media, prob.grid_shape, prob.origin, prob.voxel, mesh=prob.mesh, source=src, max_steps=prob.max_steps)


@functools.lru_cache(maxsize=None)
def f32_case(name, scale, medium):
    p = dense(mesh_scene(name)) if medium == "dense" else mesh_scene(name)
    p = S.Problem(p.media, p.grid_shape, p.origin, p.voxel, mesh=p.mesh, source=p.source, max_steps=F32_MAX_STEPS)
    return S.transformed(p, F32_SCALES[scale])


@functools.lru_cache(maxsize=None)
def layered_oracle(name, n, e=0, f32=False, threads=8):
    """(u64 grid, counters) of the oracle for a layered scene scaled by 2^e."""
    prob = S.transformed(LAYERED[name](), 2.0 ** e)
    _, fx, c = prob.oracle().run(n, seed=SEED, walk_f32=f32, threads=threads, want_fx=True, want_f64=False)
    fx.setflags(write=False)
    return fx, c


# ---------------------------------------------------------------- the helper
def test_transformed_moves_lengths_and_nothing_else():
    prob = mesh_scene("cornell")
    t = S.transformed(prob, 4.0, SHIFT)
    sh = np.array(SHIFT)
    assert np.array_equal(t.mesh["verts"], prob.mesh["verts"] * 4.0 + sh)
    assert np.array_equal(t.mesh["nodes"]["hi"], prob.mesh["nodes"]["hi"] * 4.0 + sh)
    assert np.array_equal(t.mesh["nodes"]["offset"], prob.mesh["nodes"]["offset"])
    assert np.array_equal(t.origin, np.array(prob.origin) * 4.0 + sh) and t.voxel == tuple(4.0 * x for x in prob.voxel)
    assert np.array_equal(t.source["pos"], np.array(prob.source["pos"]) * 4.0 + sh)
    assert t.source["extra"] == tuple(4.0 * x for x in prob.source["extra"]) and t.source["dir"] == prob.source["dir"]
    assert t.media == [(m[0] / 4.0, m[1] / 4.0, m[2], m[3]) for m in prob.media]
    assert t.grid_shape == prob.grid_shape and t.max_steps == prob.max_steps and t.source["type"] == prob.source["type"]
    assert prob.mesh["verts"].max() == 7.5 and prob.origin == (-7.5, -7.5, -7.5)      # (the original is left alone)
    lay = S.transformed(S.two_layer(n=32), 0.5, SHIFT)
    assert lay.layers["z_bounds"] == [SHIFT[2], 0.05 + SHIFT[2], np.inf] and lay.layers["medium_idx"] == [0, 1]
    assert lay.mesh is None and lay.layers["n_above"] == 1.0


# ---------------------------------------------------------------- CPU: the oracle
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("name", list(LAYERED))
def test_oracle_layered_walk_has_no_absolute_length(name, f32):
    """(a) 3000 photons: fixed-point grid, steps and EVERY counter of the scaled problem equal the unscaled run's exactly."""
    fx0, c0 = layered_oracle(name, 3000, 0, f32, 1)
    assert fx0.sum() > 0 and c0["steps"] > 3000
    for e in EXPONENTS:
        fx, c = layered_oracle(name, 3000, e, f32, 1)
        assert c == c0, (e, c, c0)
        assert np.array_equal(fx, fx0), e


@pytest.mark.parametrize("tf", list(TRANSFORMS))
@pytest.mark.parametrize("name", list(MESH))
def test_oracle_runs_the_transformed_mesh_problems(name, tf):
    """(b) the reference the device is held to below is itself sound there: energy is conserved to 1e-9 n, and where EPSILON
    does not grow against the scene (scales >= 1, the shifts) no weight is lost outside the grid."""
    fx, c = mesh_oracle(name, tf)
    assert c["photons"] == N_MESH and fx.sum() > 0 and c["w_escaped_mesh"] > 0
    assert abs(O.conservation_residual(c)) < 1e-9 * N_MESH
    if TRANSFORMS[tf][0] >= 1.0:
        assert c["w_lost_outside_grid"] == 0.0


# ---------------------------------------------------------------- 1. the plane pre-test, pair by pair
HOP_REL = (1e-2, 1e-3, 1e-4, 1e-5)
REACH_F32 = (("one", 1.0, 0.0), ("up10", 2.0 ** 10, 0.0), ("down10", 2.0 ** -10, 0.0))
REACH_F64 = REACH_F32 + (("up14", 2.0 ** 14, 0.0), ("shift4096", 1.0, 4096.0), ("shift1e6", 1.0, 1e6))
REACH_CASES = [(s, True) + t for s in ("tilted", "cornell", "ball") for t in REACH_F32] + \
              [(s, False) + t for s in ("tilted", "cornell", "ball") for t in REACH_F64]
REACH_IDS = ["%s-%s-%s" % (c[0], "f32" if c[1] else "f64", c[2]) for c in REACH_CASES]


@functools.lru_cache(maxsize=None)
def reach_triangles(which):
    """(triangles [K, 3, 3], extent of their scene): one tilted triangle in a random orthonormal frame at Cornell scale, the 30
    triangles of the Cornell scene, the 80 of the ball of sphere_in_box(1)."""
    if which == "tilted":
        q, _ = np.linalg.qr(np.random.RandomState(12).normal(size=(3, 3)))
        local = np.array([[-5.0, -4.0, 0.0], [6.0, -3.0, 0.0], [-1.0, 6.0, 0.0]])
        tris = (local @ q.T + np.array([0.5, -0.3, 0.4]))[None]
        assert np.abs(tris).max() <= 7.5
        return tris, 7.5
    if which == "cornell":
        return np.array(mesh_scene("cornell").mesh["verts"]), 7.5
    v, f = S.icosphere(1, 1.5, (0.3, -0.2, 0.1))
    return v[f], 4.0


def reach_queries(which, f32, scale, shift, hop_rel, n, seed):
    """n hops that end just beyond the plane of a triangle they hit: rows [n, 17] for LT_FN_PLANE_REACH and t_exact.

    A point P inside the triangle (every barycentric coordinate >= 0.05), a side, a direction towards the plane with
    cos = |d.n| uniform up to 1, an origin o = P - d h / cos at height h = hop_rel * extent * U(0.05, 1) over the plane;
    o and d are rounded to the walk's precision, t_exact is computed in float64 from the rounded values and
    s = t_exact (1 + U(0, 3e-2)) (f32; 3e-4 for f64), rounded likewise.  So that the hops ARE hits of the triangle test
    (a query that it refuses says nothing about the pre-test) two of its absolute constants bound the draw: cos stays above
    3e-7 / |ab x ac| (its |det| > 1e-7; never below 0.02), and h above (2..5)e-6 cos plus four roundings of a coordinate
    (its t > EPSILON = 1e-6) -- which only matters where hop_rel * extent itself falls below EPSILON (2^-10 scenes)."""
    rs = np.random.RandomState(seed)
    dt = np.float32 if f32 else np.float64
    base, extent = reach_triangles(which)
    tris = base * scale + np.array([shift, -shift, shift])
    extent *= scale
    k = rs.randint(0, len(tris), n)
    tri = tris[k]
    a, ab, ac = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    nn = np.cross(ab, ac)
    area2 = np.linalg.norm(nn, axis=1)
    unit = nn / area2[:, None]
    w = 0.05 + 0.85 * rs.dirichlet([1.0, 1.0, 1.0], n)
    p = a + w[:, 1:2] * ab + w[:, 2:3] * ac
    cos_min = np.clip(3e-7 / area2, 0.02, 0.9)
    cos = cos_min + (1.0 - cos_min) * rs.rand(n)
    r = rs.normal(size=(n, 3))
    tng = r - (r * unit).sum(axis=1)[:, None] * unit
    tng /= np.linalg.norm(tng, axis=1)[:, None]
    side = rs.choice([-1.0, 1.0], n)
    d = -(side * cos)[:, None] * unit + np.sqrt(1.0 - cos * cos)[:, None] * tng
    h = hop_rel * extent * rs.uniform(0.05, 1.0, n)
    h = np.maximum(h, (2.0 + 3.0 * rs.rand(n)) * 1e-6 * cos + 4.0 * np.finfo(dt).eps * float(np.abs(tris).max()))
    o = p - d * (h / cos)[:, None]
    o, d = o.astype(dt).astype(np.float64), d.astype(dt).astype(np.float64)
    t_exact = ((a - o) * nn).sum(axis=1) / (d * nn).sum(axis=1)
    s = (t_exact * (1.0 + rs.uniform(0.0, 3e-2 if f32 else 3e-4, n))).astype(dt).astype(np.float64)
    rows = np.concatenate([o, d, tri.reshape(n, 9), s[:, None], np.full((n, 1), 1.0 if f32 else 0.0)], axis=1)
    return rows, t_exact


def tri_hit_float64(rows):
    """tri_hit (lt_device.hpp) restated in NumPy float64 on LT_FN_PLANE_REACH rows: t, NaN for none."""
    o, d, tri = rows[:, 0:3], rows[:, 3:6], rows[:, 6:15].reshape(-1, 3, 3)
    a, ab, ac = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    nn = np.cross(ab, ac)
    nn /= np.linalg.norm(nn, axis=1)[:, None]
    pvec = np.cross(d, ac)
    det = (ab * pvec).sum(axis=1)
    ok = (np.abs((d * nn).sum(axis=1)) > 1e-7) & ~((-1e-7 < det) & (det < 1e-7))
    inv = 1.0 / np.where(det == 0, 1.0, det)
    tvec = o - a
    u = (tvec * pvec).sum(axis=1) * inv
    qvec = np.cross(tvec, ab)
    v = (d * qvec).sum(axis=1) * inv
    t = (ac * qvec).sum(axis=1) * inv
    ok &= (u >= 0) & (u <= 1) & (v >= 0) & (u + v <= 1) & (t > 1e-7)
    return np.where(ok, t, np.nan)


@pytest.mark.parametrize("case", REACH_CASES, ids=REACH_IDS)
def test_reach_queries_are_hits(case):
    """The guard of the device test below, on the generator alone: at least 90 % of a case's queries are hits of the float64
    restatement of the triangle test inside (EPSILON, s).  (A sample of 2^16 per case: the device test counts all 2^20.)"""
    which, f32, _, scale, shift = case
    for j, hop_rel in enumerate(HOP_REL):
        rows, t_exact = reach_queries(which, f32, scale, shift, hop_rel, 1 << 16, 100 + j)
        t = tri_hit_float64(rows)
        hits = (t > 1e-6) & (t < rows[:, 15])
        assert hits.mean() >= 0.9, (hop_rel, hits.mean())
        assert np.allclose(t[hits], t_exact[hits], rtol=1e-5 if shift == 0 else 1e-3, atol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("case", REACH_CASES, ids=REACH_IDS)
def test_plane_pretest_rejects_no_hit(ctx, case):
    """2^20 hops per hop_rel: no query has 1e-6 < t < s (the triangle test's own t, in walk precision) together with
    reach == 0 -- a photon that hops through a facet and keeps the wrong medium."""
    which, f32, _, scale, shift = case
    for j, hop_rel in enumerate(HOP_REL):
        rows, _ = reach_queries(which, f32, scale, shift, hop_rel, 1 << 20, 100 + j)
        out = ctx.eval("PLANE_REACH", rows)
        reach, t = out[:, 0], out[:, 1]
        assert np.all((reach == 0.0) | (reach == 1.0))
        hits = (t > 1e-6) & (t < rows[:, 15])
        lost = int((hits & (reach == 0.0)).sum())
        print("plane pre-test %s hop_rel %g: %d hits of %d, %d of them rejected (share %.3g)"
              % (REACH_IDS[REACH_CASES.index(case)], hop_rel, hits.sum(), len(t), lost, lost / max(1, hits.sum())))
        assert hits.mean() >= 0.9, (hop_rel, hits.mean())
        assert lost == 0, "hop_rel %g: the pre-test rejects %d of %d hits" % (hop_rel, lost, hits.sum())


# ---------------------------------------------------------------- GPU helpers
def launch_fx(ctx, prob, n, mode="atomic", f32=False, **knobs):
    """One launch of `prob` into a fresh u64 tally under the given knobs: (grid, counters, mesh_accel_info or None)."""
    with ctx.tuning(**knobs):
        prob.apply(ctx, "u64fx"); ctx.set_tally_mode(mode)
        ctx.launch(n, seed=SEED, f32_walk=f32); ctx.sync()
        info = ctx.mesh_accel_info() if prob.mesh is not None else None
    return ctx.read_grid_raw(), ctx.read_counters(), info


def assert_variant_ran(info, knobs, default_kind):
    """The acceleration data is what the knobs ask for (as test_surface_query_shortcuts_do_not_change_results checks it)."""
    if "march_cells" in knobs:
        assert max(info["march_dims"]) == knobs["march_cells"] + 2, info
    if "clearance_cells" in knobs:
        assert max(info["clearance_dims"]) == knobs["clearance_cells"], info
    if "no_clearance" in knobs:
        assert info["kind"] == 0, info
    if "no_march" in knobs:
        assert info["kind"] & 2 == 0, info
    if "force_march" in knobs:
        assert info["kind"] & 2, info
    if "no_near_lists" in knobs:
        assert info["kind"] & 1, info
    if not knobs:
        assert info["kind"] == default_kind, info


def assert_same_run(got, ref, what):
    assert got[1]["steps"] == ref[1]["steps"], "%s: photon-step counts differ (%d, %d)" % (what, got[1]["steps"], ref[1]["steps"])
    diff = int((got[0] != ref[0]).sum())
    assert diff == 0, "%s: %d voxels differ in the 2^-40 fixed-point tally" % (what, diff)


# ---------------------------------------------------------------- 2. f64 mesh walks, other scales and offsets
@pytest.mark.gpu
@pytest.mark.parametrize("tf", list(TRANSFORMS))
@pytest.mark.parametrize("name", list(MESH))
def test_f64_mesh_walk_matches_oracle_in_other_units_and_frames(ctx, name, tf):
    prob = mesh_case(name, tf)
    fxo, co = mesh_oracle(name, tf)
    in_lds = MESH[name] == 1
    off = ({"no_near_lists": 1}, {"no_clearance": 1}, {"force_march": 1}) if in_lds else ({"no_march": 1}, {"march_cells": 16})
    try:
        for mode in ("atomic", "log"):
            fx, c, info = launch_fx(ctx, prob, N_MESH, mode)
            assert_variant_ran(info, {}, MESH[name])
            assert_same_run((fx, c), (fxo, co), "%s %s %s against the oracle" % (name, tf, mode))
            check_counters(c, co, N_MESH)
        for knobs in off:
            fx, c, info = launch_fx(ctx, prob, N_MESH, "atomic", **knobs)
            assert_variant_ran(info, knobs, MESH[name])
            assert_same_run((fx, c), (fxo, co), "%s %s %s" % (name, tf, knobs))
    finally:
        ctx.set_tally_mode("auto")


# ---------------------------------------------------------------- 3. f32 mesh walks: every shortcut is exact
@pytest.mark.gpu
@pytest.mark.parametrize("medium", ["plain", "dense"])
@pytest.mark.parametrize("scale", list(F32_SCALES))
@pytest.mark.parametrize("name", list(MESH))
def test_f32_mesh_walk_shortcuts_are_exact(ctx, name, scale, medium):
    """The reference run answers every step's surface query from the BVH (no clearance grid, no near lists, no pre-test, no
    march); every other route must give its u64 grid and step count bit for bit."""
    prob = f32_case(name, scale, medium)
    if MESH[name] == 2:      # beyond LDS in f32 too: walk_kernel_m over the march grid
        ref_knobs = {"no_march": 1}
        routes = ({}, {"march_cells": 16}, {"march_cells": 200}, {"query_min": 1}, {"query_min": 64})
    else:                    # f32 tables in LDS: clearance grid, near lists, plane pre-test
        ref_knobs = {"no_clearance": 1}
        routes = ({}, {"no_near_lists": 1}, {"clearance_cells": 16}, {"clearance_cells": 200}, {"force_march": 1},
                  {"force_march": 1, "march_cells": 16}, {"force_march": 1, "march_cells": 200}, {"query_min": 1}, {"query_min": 64})
    try:
        fx, c, info = launch_fx(ctx, prob, N_F32, "atomic", True, **ref_knobs)
        assert_variant_ran(info, ref_knobs, MESH[name])
        assert info["kind"] == 0, info
        ref = (fx, c)
        assert fx.sum() > 0 and c["steps"] > 10 * N_F32 and c["photons"] == N_F32
        if medium == "dense":      # the beam reached the body, and photons walk inside it
            assert c["w_absorbed"] > 0.1 * N_F32
        for knobs in routes:
            fx, c, info = launch_fx(ctx, prob, N_F32, "atomic", True, **knobs)
            assert_variant_ran(info, knobs, MESH[name])
            assert_same_run((fx, c), ref, "%s %s %s %s" % (name, scale, medium, knobs or "default"))
        fx, c, _ = launch_fx(ctx, prob, N_F32, "log", True)
        assert_same_run((fx, c), ref, "%s %s %s log" % (name, scale, medium))
    finally:
        ctx.set_tally_mode("auto")


# ---------------------------------------------------------------- 4. layered walks: units
def layered_routes(ctx, prob, n, f32):
    """(route, grid, counters) of every slab build: atomic deposits; the deposit log; the log with the bulk / tail split; the
    log with two lanes."""
    yield ("atomic",) + launch_fx(ctx, prob, n, "atomic", f32)[:2]
    yield ("log",) + launch_fx(ctx, prob, n, "log", f32)[:2]
    yield ("log, tail_split=16",) + launch_fx(ctx, prob, n, "log", f32, tail_split=16)[:2]
    ctx.set_overlap(2)
    try:
        yield ("log, two lanes",) + launch_fx(ctx, prob, n, "log", f32)[:2]
    finally:
        ctx.set_overlap(0)


@pytest.mark.gpu
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("name", list(LAYERED))
def test_layered_walk_in_other_units(ctx, name, f32):
    """f64: grid, steps and counters of every route at every scale equal the oracle's UNSCALED run (the oracle's own invariance
    is pinned above).  f32: grid and steps equal the device's own unscaled atomic run -- every f32 slab build does the same
    arithmetic, and none of it has an absolute length."""
    try:
        if f32:
            ref = launch_fx(ctx, LAYERED[name](), N_LAYERED, "atomic", True)[:2]
            assert ref[0].sum() > 0 and ref[1]["steps"] > N_LAYERED
        else:
            ref = layered_oracle(name, N_LAYERED)
        for e in (-20, -10, 0, 10, 20):
            prob = S.transformed(LAYERED[name](), 2.0 ** e)
            for route, fx, c in layered_routes(ctx, prob, N_LAYERED, f32):
                assert_same_run((fx, c), ref, "%s 2^%d %s" % (name, e, route))
                if not f32:
                    check_counters(c, ref[1], N_LAYERED)
    finally:
        ctx.set_tally_mode("auto"); ctx.set_overlap(0)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["atomic", "log"])
def test_layered_walk_in_a_shifted_frame(ctx, mode):
    prob = S.transformed(S.two_layer(n=32), 1.0, SHIFT)
    _, fxo, co = prob.oracle().run(N_LAYERED, seed=SEED, threads=8, want_fx=True, want_f64=False)
    try:
        fx, c, _ = launch_fx(ctx, prob, N_LAYERED, mode)
    finally:
        ctx.set_tally_mode("auto")
    assert_same_run((fx, c), (fxo, co), "two_layer shifted, %s" % mode)
    check_counters(c, co, N_LAYERED)
    assert fxo.sum() > 0 and co["w_escaped_top"] > 0
