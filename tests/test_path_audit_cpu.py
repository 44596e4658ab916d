"""The CPU oracle's captured paths, re-derived event by event from their random draws (tests/path_audit.py).

Almost every walk test compares a kernel with oracle/lt_walk.inc bit for bit; this one ties the ORACLE to the physics with
code that shares nothing with it: np.longdouble, the raw draws (oracle.rng_raw) and textbook laws.  The checks:

  A free path      optical depth between two scatterings = -ln u0, carried through interfaces and clear layers
  B segments       points move along the recorded direction; |direction| = 1
  C deflection     the Henyey-Greenstein CDF of the cosine taken = u1 (sign convention of g included)
  D azimuth        components in the MCML frame = sin t (cos, sin)(2 pi u2)
  E weight         w (1 - mu_a / mu_t), the roulette's 10 x at chance 0.1, pdf_dir = the HG value
  F plane events   snapped onto the bound; angle-form Fresnel R against u3; mirror / Snell directions; layer entered
  G mesh events    on the triangle, the nearest one, facing normal, the same laws; no segment crosses a triangle (leaks)
  H emission       pencil (Snell and 1 - R on entry, tilted too) and cosine quad (point, lobe about the normal, densities)
  I fates, totals  every path ends for a derived reason; the fates sum to the eight w_* counters, steps and photons
  J deposits       the tally rebuilt voxel by voxel within its rounding bound

and mutation tests: a slightly wrong scene or doctored records must produce violations in the named check.  The measured
deviations of the oracle are tabulated in tests/test_gpu_path_audit.py, which runs the same audit on the capture kernels.

What the audit found when it was written: a cosine-quad source whose normal has a negative z emitted into the hemisphere
BEHIND it (kernels and oracle alike); scene i_quad_facing_down keeps that fixed.
"""
import numpy as np
import pytest

from oracle import oracle as O
from tests import path_audit as PA
from tests import path_audit_scenes as PS

def oracle_audit(name, scene=None, vertices=None, draws=None, **changes):
    g, c, v, cnt = PS.oracle_capture(name)
    sc = scene if scene is not None else PS.plain(PS.problem(name), PS.SCENES[name][3], **changes)
    return PA.audit(sc, PS.draws(name) if draws is None else draws, v if vertices is None else vertices, cnt, c, g, tol=PS.tol(name))


@pytest.mark.parametrize("name", list(PS.SCENES))
def test_oracle_paths_follow_the_textbook_laws(name):
    res = oracle_audit(name)
    print(PS.report(res))
    PS.check_result(res, name, PS.oracle_worst(name))


def test_the_pole_rule_is_hit_at_all():
    """|uz| > 0.99999 short of the axis: rare by design, but the scenes do reach it."""
    assert sum(oracle_audit(n)["C"]["pole"] for n in ("a_g09_matched", "b_g0", "b_g03_n14")) >= 3


def test_tolerances_follow_the_rule():
    """16 x the oracle's figure, rounded up to a power of ten, capped at 1e-8."""
    for m, w in PA.ORACLE_WORST.items():
        t = PA.TOL[m]
        assert t <= 1e-8 and 16 * w <= t * (1 + 1e-12) and (t / 10 < 16 * w or t == 1e-8)
        assert abs(np.log10(t) - round(np.log10(t))) < 1e-9
    assert PA.TOL["F.reflect"] == 0.0 and PA.TOL["I.sum"] == 1.0 and PA.TOL["J.voxel"] == 1.0


def test_edge_tolerances_follow_the_rule():
    """The edge scenes' table: the same rule; never tighter than the ordinary scenes' (it starts from their figures)."""
    for m, w in PA.ORACLE_WORST_EDGE.items():
        t = PA.TOL_EDGE[m]
        assert w >= PA.ORACLE_WORST.get(m, 0.0) and 16 * w <= t * (1 + 1e-12) and abs(np.log10(t) - round(np.log10(t))) < 1e-9
        assert t / 10 < 16 * w or t == 1e-8
        assert t <= 1e-8 or m == "E.pdf_roundings"
    assert all(PA.TOL_EDGE[m] == PA.TOL[m] for m in ("F.reflect", "I.sum", "J.voxel"))
    assert PS.EDGE and all(PS.tol(n) is PA.TOL for n in PS.SCENES if n not in PS.EDGE)


def test_cdf_form_has_no_cancellation():
    """The auditor's own CDF: at g = 1e-12 it inverts its exact inverse to long-double roundings (the textbook form, which
    divides by g, is good to 5e-8 there), and it is the textbook form wherever that one is sound."""
    u = (np.arange(1, 2000, dtype=PA.LD) / 2000)
    for g in (1e-12, -1e-9, 1e-6, 1e-3, 0.3, -0.4, 0.9, 0.99, -0.999):
        assert np.abs(PA.hg_cdf(PA.hg_inverse(u, g), g) - u).max() < 1e-15 / (1 - abs(g)), g
    c = np.linspace(-1, 1, 4001).astype(PA.LD)
    for g in (0.3, -0.4, 0.9):
        gl = PA.LD(g)
        text = (1 - gl * gl) / (2 * gl) * ((1 + gl * gl - 2 * gl * c) ** PA.LD(-0.5) - 1 / (1 + gl))
        assert np.abs(PA.hg_cdf(c, g) - text).max() < 1e-17
    assert np.array_equal(PA.hg_cdf(c, 0.0), (1 + c) / 2)


# ---------------------------------------------------------------- the audit is sharp: mutations
def _media(name, **per_medium):
    """The scene with one field of every medium changed: fn(mu_a, mu_s, g, n) -> new tuple."""
    sc = PS.plain(PS.problem(name), PS.SCENES[name][3])
    sc["media"] = [per_medium["fn"](*m) for m in sc["media"]]
    return sc


def _swap_xy(v):
    w = v.copy()
    for f in ("point", "direction", "g_norm"):
        w[f] = v[f][..., [1, 0, 2]]
    return w


def _shift_draws(d):
    """Every group of four draws rotated by one: u0 <- u1 <- u2 <- u3 <- u0."""
    return np.ascontiguousarray(np.roll(d.reshape(d.shape[0], -1, 4), -1, axis=2).reshape(d.shape))


def _swap_indices(sc):
    n_med = sc["media"][0][3]
    sc["media"] = [(m[0], m[1], m[2], sc["layers"]["n_above"]) for m in sc["media"]]
    sc["layers"]["n_above"] = sc["layers"]["n_below"] = n_med
    return sc


def _move_bound(sc):
    sc["layers"]["z_bounds"][1] += 1e-9
    return sc


def _shift_origin(sc):
    o, vx = sc["grid"]["origin"], sc["grid"]["voxel"]
    sc["grid"]["origin"] = (o[0] + vx[0], o[1], o[2])
    return sc


def _busiest_triangle(name):
    return int(np.argmax(oracle_audit(name)["G"]["tri_events"]))


def _drop_triangle(sc, name="h_slab_as_mesh"):
    keep = np.arange(len(sc["mesh"]["verts"])) != _busiest_triangle(name)
    sc["mesh"] = {k: a[keep] for k, a in sc["mesh"].items()}
    return sc


def _reverse_source(sc):
    sc["source"] = dict(sc["source"], dir=tuple(-x for x in sc["source"]["dir"]))
    return sc


MUTATIONS = {      # name: (scene, checks that must report violations, what to change)
    "g_times_1_plus_1e-6": ("a_g09_matched", "C", dict(scene=lambda: _media("a_g09_matched", fn=lambda a, s, g, n: (a, s, g * (1 + 1e-6), n)))),
    "g_times_1_plus_1e-6_at_g0999": ("x_g0999_tilted", "C", dict(scene=lambda: _media("x_g0999_tilted", fn=lambda a, s, g, n: (a, s, g * (1 + 1e-6), n)))),
    # (at g = -1e-9 the factor 1 + 1e-6 moves g by 1e-15 and the CDF by 0.75 |dg| < 1e-15 at most: below the oracle's own
    # C.cdf of 5e-14 there, so no tolerance that the oracle meets can see it.  What the measure resolves at tiny g is an
    # ABSOLUTE error of g from about 1e-10 on, a tenth of the smallest nonzero |g| among the scenes but one; and the sign.)
    "g_plus_1e-10_at_g1e-9": ("t_gneg1e-9", "C", dict(scene=lambda: _media("t_gneg1e-9", fn=lambda a, s, g, n: (a, s, g + 1e-10, n)))),
    "g_other_sign_at_g1e-9": ("t_gneg1e-9", "C", dict(scene=lambda: _media("t_gneg1e-9", fn=lambda a, s, g, n: (a, s, -g, n)))),
    "g_times_1_plus_1e-6_at_gneg099_pdf": ("x_gneg099", "E", dict(scene=lambda: _media("x_gneg099", fn=lambda a, s, g, n: (a, s, g * (1 + 1e-6), n)))),
    # (E.weight_in is in units of the incoming weight: at albedo 1e-10 it resolves a relative error of the albedo from 1e-4 on)
    "mu_s_times_1_plus_1e-3_at_albedo_0": ("w_albedo_to_0", "E", dict(scene=lambda: _media("w_albedo_to_0", fn=lambda a, s, g, n: (a, s * (1 + 1e-3), g, n)))),
    "g_other_sign": ("b_gneg", "C", dict(scene=lambda: _media("b_gneg", fn=lambda a, s, g, n: (a, s, -g, n)))),
    "mu_t_replaced_by_mu_s": ("a_g09_matched", "A", dict(scene=lambda: _media("a_g09_matched", fn=lambda a, s, g, n: (0.0, s, g, n)))),
    "mu_a_times_1_plus_1e-6": ("a_g09_matched", "E", dict(scene=lambda: _media("a_g09_matched", fn=lambda a, s, g, n: (a * (1 + 1e-6), s, g, n)))),
    "n1_and_n2_swapped": ("b_g03_n14", "F", dict(scene=lambda: _swap_indices(PS.plain(PS.problem("b_g03_n14"))))),
    "layer_bound_moved_1e-9": ("d_stack", "F", dict(scene=lambda: _move_bound(PS.plain(PS.problem("d_stack"))))),
    "x_and_y_swapped": ("a_g09_matched", "D", dict(vertices=lambda: _swap_xy(PS.oracle_capture("a_g09_matched")[2]))),
    "draws_shifted_in_group": ("a_g09_matched", "ACD", dict(draws=lambda: _shift_draws(PS.draws("a_g09_matched")))),
    "roulette_factor_9": ("c_albedo_half", "EI", dict(scene=lambda: PS.plain(PS.problem("c_albedo_half"), roulette_factor=9))),
    "voxel_origin_one_voxel_off": ("a_g09_matched", "J", dict(scene=lambda: _shift_origin(PS.plain(PS.problem("a_g09_matched"))))),
    "triangle_missing_from_audited_mesh": ("h_slab_as_mesh", "G", dict(scene=lambda: _drop_triangle(PS.plain(PS.problem("h_slab_as_mesh"))))),
    "quad_lobe_mirrored": ("i_quad_facing_down", "H", dict(scene=lambda: _reverse_source(PS.plain(PS.problem("i_quad_facing_down"))))),
    "tilted_beam_entered_untilted": ("e_tilted_on_top", "H", dict(scene=lambda: PS.plain(
        PS.problem("e_tilted_on_top"), source=dict(PS.problem("e_tilted_on_top").source, dir=(0.0, 0.0, 1.0))))),
}


@pytest.mark.parametrize("mutation", list(MUTATIONS))
def test_mutation_is_caught_in_its_check(mutation):
    name, checks, change = MUTATIONS[mutation]
    res = oracle_audit(name, **{k: f() for k, f in change.items()})
    for k in checks:
        assert res[k]["violations"] > 0, "%s: check %s did not notice\n%s" % (mutation, k, PS.report(res))


def test_walk_through_a_missing_triangle_is_a_leak():
    """The leak check proper: the WALK's mesh lacks the busiest triangle (moved out of reach: its BVH leaf no longer holds
    it), the audited mesh is whole -- segments then cross a triangle, and the events behind it happen in the wrong medium."""
    name = "h_slab_as_mesh"
    prob = PS.problem(name)
    k = _busiest_triangle(name)
    verts = np.array(prob.mesh["verts"], dtype=np.float64).reshape(-1, 3, 3).copy()
    verts[k] += 1000.0
    o = O.OracleScene(prob.media, prob.grid_shape, prob.origin, prob.voxel, mesh=dict(prob.mesh, verts=verts),
                      source=prob.source, max_steps=prob.max_steps)
    n, kk = 300, PS.K
    g, c, v, cnt = o.run_capture(n, kk, seed=PS.SEED)
    res = PA.audit(PS.plain(prob), PS.draws(name)[:n], v, cnt, c, g)
    assert res["G"]["leaks"] > 100 and res["G"]["violations"] >= res["G"]["leaks"]


def test_fixed_point_tally_is_the_sum_of_its_deposits():
    """The oracle's u64 fixed-point tally (2^-40 units) of the same walk: +-1 unit per deposit about the rebuilt sums; one
    unit more or less in a well-filled voxel is noticed."""
    name = "d_stack"
    _, c, v, cnt = PS.oracle_capture(name)
    _, fx, cfx = PS.problem(name).oracle().run(PS.SCENES[name][1], seed=PS.SEED, want_fx=True, want_f64=False)
    assert cfx["steps"] == c["steps"]
    res = PA.audit(PS.plain(PS.problem(name)), PS.draws(name), v, cnt, c, fx, grid_kind="u64fx")
    PS.check_result(res, name)
    bad = fx.copy()
    k = np.unravel_index(np.argmax(fx), fx.shape)
    bad[k] += np.uint64(4000)         # (that voxel holds fewer deposits than that)
    assert PA.audit(PS.plain(PS.problem(name)), PS.draws(name), v, cnt, c, bad, grid_kind="u64fx")["J"]["violations"] == 1
