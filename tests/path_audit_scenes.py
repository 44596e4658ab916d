"""The scenes of the path audit (tests/path_audit.py), shared by its CPU and GPU tests: each one is a scenes.Problem for the
oracle and the device, and the same thing as plain data for the auditor.  2000 photons, K = 40 vertices and max_steps = 39
(every path is captured whole) are the smallest sizes at which every branch named below still occurs.

The pencil beams enter at the centre of a voxel column (never on x = y = 0 of an even grid, which is a voxel face: every first
deposit would be ambiguous), and the grids are small enough that part of the weight falls outside them."""
import functools

import numpy as np

from oracle import oracle as O
from tests import path_audit as PA
from tests import scenes as S

N, K = 2000, 40
SEED = 97
STACK = dict(media=[(0.3, 12.0, 0.8, 1.33), (0.0, 0.0, 0.0, 1.0), (0.5, 9.0, 0.9, 1.5)],       # (d): clear middle layer
             z_bounds=[0.0, 0.1, 0.15, 0.35], medium_idx=[0, 1, 2], n_above=1.0, n_below=1.4)
TILT = (float(np.sin(np.radians(40.0))), 0.0, float(np.cos(np.radians(40.0))))


def layered(media, z_bounds, medium_idx=None, n_above=1.0, n_below=1.0, n=16, voxel=0.1, pos=None, direction=(0.0, 0.0, 1.0),
            dz=None):
    half = n * voxel / 2
    dz = voxel if dz is None else dz
    pos = (voxel / 2, voxel / 2, float(z_bounds[0])) if pos is None else pos
    return S.Problem([tuple(m) for m in media], (n, n, n), (-half, -half, float(z_bounds[0])), (voxel, voxel, dz),
                     layers=dict(z_bounds=list(z_bounds), medium_idx=list(medium_idx or range(len(z_bounds) - 1)),
                                 n_above=n_above, n_below=n_below),
                     source=dict(type=0, pos=pos, dir=direction, extra=(0.0,) * 6, start_medium=0), max_steps=K - 1)


def stack(**kw):
    return layered(STACK["media"], STACK["z_bounds"], STACK["medium_idx"], STACK["n_above"], STACK["n_below"], voxel=0.05,
                   dz=0.025, **kw)


def _sphere():
    prob = S.sphere_in_box(4, n=16)[0]
    prob.max_steps = 23
    return prob


def _cornell_with(source):
    prob = S.cornell(32, max_steps=K - 1)
    prob.source = source
    return prob


def _slab_mesh():
    prob = S.slab_as_mesh(**dict(S.ANCHOR_SCENES["two_layer_tilted"], max_steps=K - 1))[0]
    return prob


# name -> (problem factory, photons, K, quantity)
SCENES = {
    "a_g09_matched": (lambda: layered([(0.1, 10.0, 0.9, 1.0)], [0.0, np.inf]), N, K, 0),
    "b_g0": (lambda: layered([(0.1, 10.0, 0.0, 1.0)], [0.0, np.inf]), N, K, 0),
    "b_gneg": (lambda: layered([(0.1, 10.0, -0.4, 1.0)], [0.0, np.inf]), N, K, 0),
    "b_g03_n14": (lambda: layered([(0.1, 10.0, 0.3, 1.4)], [0.0, np.inf]), N, K, 0),
    "c_albedo_half": (lambda: layered([(5.0, 5.0, 0.5, 1.0)], [0.0, np.inf]), N, K, 0),
    "d_stack": (stack, N, K, 0),
    "d_stack_fluence": (stack, N, K, 1),
    "e_tilted_on_top": (lambda: stack(pos=(0.025, 0.025, 0.0), direction=TILT), N, K, 0),
    "e_tilted_inside": (lambda: stack(pos=(0.025, 0.025, 0.12), direction=TILT), N, K, 0),
    "f_cornell": (lambda: S.cornell(32, max_steps=K - 1), N, K, 0),
    "g_sphere_march": (_sphere, 300, 24, 0),
    # beyond the issue's list: (f) and (g) reach their inner surfaces a handful of times in so few steps, so a thin two-layer
    # slab built as a closed mesh (scenes.slab_as_mesh) supplies the mesh walk's Fresnel events by the thousand, a clear
    # medium under the lid and a pure absorber (weight 0 after one interaction) below
    "h_slab_as_mesh": (_slab_mesh, N, K, 0),
    # a quad source whose normal has a negative z (and |nx| > |ny|: the other branch of the frame construction) in the middle
    # of (f)'s cavity: the emission once mirrored every such source's lobe
    "i_quad_facing_down": (lambda: _cornell_with(dict(type=1, pos=(-1.0, -1.0, 0.0), dir=(0.6, 0.0, -0.8),
                                                      extra=(1.6, 0.0, 1.2, 0.0, 2.0, 0.0), start_medium=0)), 500, K, 0),
}

# ---------------------------------------------------------------- the edges of what lt_set_media accepts
# 500 photons, K = 40, 16^3 grids.  Until these scenes existed the walk sampled Henyey-Greenstein by the quotient form for every
# g != 0, which cancels as g -> 0: on the parent's oracle check C failed in t_g1e-6 (6346 of 7697 scatterings, worst 1.1e-10),
# t_gneg1e-9 (all, 9.7e-8), t_g1e-12 (all, 7.2e-5) and in their cone and fluence twins -- exactly the scenes with |g| <= 1e-6.
NE = 500


def half_space(g, **kw):
    return layered([(0.1, 10.0, g, 1.0)], [0.0, np.inf], **kw)


def _cornell_cone(g):
    """(i)'s source above (f)'s cone, whose medium gets the g: the mesh walk reads it from the medium table, not a layer record."""
    prob = _cornell_with(dict(type=1, pos=(-1.0, -1.0, 0.0), dir=(0.6, 0.0, -0.8), extra=(1.6, 0.0, 1.2, 0.0, 2.0, 0.0),
                              start_medium=0))
    prob.media = [prob.media[0], (1.0, 5.0, g, 1.5)]
    return prob


SCENES.update({
    # tiny g: the sampling's cancellation (fixed: hg_small_g below |g| = 2^-6); one on each side of the switch as well
    "t_g1e-3": (lambda: half_space(1e-3), NE, K, 0),
    "t_g1e-6": (lambda: half_space(1e-6), NE, K, 0),
    "t_gneg1e-9": (lambda: half_space(-1e-9), NE, K, 0),
    "t_g1e-12": (lambda: half_space(1e-12), NE, K, 0),
    "t_g1e-6_cone": (lambda: _cornell_cone(1e-6), NE, K, 0),
    "t_gneg1e-9_fluence": (lambda: half_space(-1e-9), NE, K, 1),
    # extreme g: the CDF is ill-conditioned there (path_audit: C.cos, E.pdf_roundings).  g = +-0.999 under a vertical beam is
    # left out: the reference alone takes the near-pole rule at 13 % / 18.5 % of the scatterings, above its 1 % cap
    "x_g099": (lambda: half_space(0.99), NE, K, 0),
    "x_g0999_tilted": (lambda: half_space(0.999, direction=TILT), NE, K, 0),
    "x_gneg099": (lambda: half_space(-0.99), NE, K, 0),
    # near-matched indices: Fresnel's differences of nearly equal products
    "n_slab_1e-9_in_air": (lambda: layered([(0.1, 10.0, 0.9, 1.0 + 1e-9)], [0.0, 0.3]), NE, K, 0),
    "n_two_layers_1e-7": (lambda: layered([(0.1, 10.0, 0.9, 1.4), (0.1, 10.0, 0.9, 1.4 * (1.0 + 1e-7))], [0.0, 0.1, 0.3],
                                          n_below=1.4), NE, K, 0),
    # a layer 1e-9 thick between two ordinary ones
    "s_sliver": (lambda: layered([(0.1, 10.0, 0.9, 1.4), (0.1, 10.0, 0.9, 1.33), (0.1, 10.0, 0.9, 1.5)],
                                 [0.0, 0.1, 0.1 + 1e-9, 0.3]), NE, K, 0),
    # albedo -> 1 and -> 0
    "w_albedo_to_1": (lambda: layered([(1e-9, 10.0, 0.5, 1.0)], [0.0, np.inf]), NE, K, 0),
    "w_albedo_to_0": (lambda: layered([(10.0, 1e-9, 0.5, 1.0)], [0.0, np.inf]), NE, K, 0),
    # mu_t = 1.01e5 in voxels of 1e-4
    "m_dense": (lambda: layered([(1e3, 1e5, 0.9, 1.4)], [0.0, np.inf], voxel=1e-4), NE, K, 0),
    # a beam 0.1 degrees off grazing
    "z_grazing": (lambda: layered([(0.1, 10.0, 0.9, 1.4)], [0.0, 0.3], pos=(0.05, 0.05, 0.0),
                                  direction=(float(np.sin(np.radians(89.9))), 0.0, float(np.cos(np.radians(89.9))))), NE, K, 0),
})


EDGE = frozenset(n for n in SCENES if n[:2] in ("t_", "x_", "n_", "s_", "w_", "m_", "z_"))


def tol(name):
    """The tolerances of the scene's audit (path_audit.TOL, or TOL_EDGE for the edge scenes)."""
    return PA.TOL_EDGE if name in EDGE else PA.TOL


def oracle_worst(name):
    return PA.ORACLE_WORST_EDGE if name in EDGE else PA.ORACLE_WORST


@functools.lru_cache(maxsize=None)
def problem(name):
    return SCENES[name][0]()


def plain(prob, quantity=0, **changes):
    """The problem as the plain data the auditor takes (no BVH: it tests every triangle)."""
    sc = dict(media=[tuple(m) for m in prob.media], layers=None, mesh=None, source=dict(prob.source),
              grid=dict(shape=tuple(prob.grid_shape), origin=tuple(prob.origin), voxel=tuple(prob.voxel)),
              quantity=quantity, max_steps=prob.max_steps)
    if prob.layers is not None:
        sc["layers"] = dict(prob.layers, z_bounds=list(prob.layers["z_bounds"]), medium_idx=list(prob.layers["medium_idx"]))
    else:
        sc["mesh"] = dict(verts=np.array(prob.mesh["verts"], dtype=np.float64).reshape(-1, 3, 3),
                          med_front=np.array(prob.mesh["med_front"]), med_back=np.array(prob.mesh["med_back"]))
    sc.update(changes)
    return sc


@functools.lru_cache(maxsize=None)
def draws(name, seed=SEED):
    """Raw draws [n, 4 (K + 1)] of every photon of the scene, from the oracle's generator (tests/test_gpu_parity.py and the
    GPU audit compare the device's with it).  Shared, read-only."""
    _, n, k, _ = SCENES[name]
    d = np.stack([O.rng_raw(seed, i, 4 * (k + 1)) for i in range(n)])
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def oracle_capture(name, seed=SEED):
    """(grid, counters, vertices, counts) of the oracle's capturing walk.  Computed once, shared, never written to."""
    _, n, k, quantity = SCENES[name]
    o = problem(name).oracle()
    o.quantity = quantity
    g, c, v, cnt = o.run_capture(n, k, seed=seed)
    for a in (g, v, cnt):
        a.setflags(write=False)
    return g, c, v, cnt


def report(res):
    """One line per check: events, violations, declined and the worst deviation of every measure."""
    lines = []
    for k in sorted(res):
        r = res[k]
        worst = " ".join("%s=%.2e" % kv for kv in sorted(r["worst"].items()))
        rest = {a: b for a, b in r.items() if a not in ("worst", "n", "violations", "declined", "totals", "tri_events")}
        lines.append("%s n=%d viol=%d decl=%d %s %s" % (k, r["n"], r["violations"], r["declined"], worst, rest or ""))
    return "\n".join(lines)


# the events each scene exists for: check -> key of its result -> at least so many
OCCURRED = {
    "a_g09_matched": {"C": dict(pole=1, axis=2000), "F": dict(left=100), "I": dict(capped=100), "J": dict(outside=1000)},
    "b_g0": {"C": dict(axis=2000), "F": dict(left=100)},
    "b_gneg": {"C": dict(axis=2000), "F": dict(left=100)},
    "b_g03_n14": {"F": dict(reflected=50, total_internal=500, left=100), "A": dict(carried=500), "H": dict(specular=0.0277)},
    "c_albedo_half": {"E": dict(roulette_survived=50, roulette_died=500), "I": dict(roulette=500)},
    "d_stack": {"A": dict(carried=1000, through_clear=1000), "F": dict(reflected=500, transmitted=2000, total_internal=500),
                "I": dict(top=100, bottom=1000)},
    "d_stack_fluence": {"A": dict(through_clear=1000), "J": dict(voxels_hit=1000)},
    "e_tilted_on_top": {"H": dict(specular=0.0241), "F": dict(transmitted=2000, total_internal=500)},
    "e_tilted_inside": {"A": dict(through_clear=2000), "F": dict(transmitted=2000)},
    "f_cornell": {"G": dict(left=500, segments=50000), "I": dict(mesh=500)},
    "g_sphere_march": {"G": dict(left=100, transmitted=1, reflected=1)},
    "h_slab_as_mesh": {"G": dict(reflected=1000, transmitted=5000, total_internal=500, left=100), "I": dict(weight0=500),
                       "A": dict(carried=5000, through_clear=2000)},
    "i_quad_facing_down": {"H": dict(n=500), "I": dict(capped=500), "G": dict(reflected=100, transmitted=400)},      # (the cone)
    # the edge scenes (C last_medium: scatterings in the medium the scene is about)
    "t_g1e-3": {"C": dict(axis=500, last_medium=5000)},
    "t_g1e-6": {"C": dict(axis=500, last_medium=5000)},
    "t_gneg1e-9": {"C": dict(axis=500, last_medium=5000)},
    "t_g1e-12": {"C": dict(axis=500, last_medium=5000)},
    "t_g1e-6_cone": {"C": dict(last_medium=1000), "G": dict(transmitted=400)},                     # (scatterings inside the cone)
    "t_gneg1e-9_fluence": {"C": dict(axis=500, last_medium=5000), "J": dict(voxels_hit=1000)},
    "x_g099": {"C": dict(ill_conditioned=15000, pole=1)},
    "x_g0999_tilted": {"C": dict(ill_conditioned=15000)},
    "x_gneg099": {"C": dict(ill_conditioned=4000, pole=1)},
    # crossed = every transmission, those that leave the slab included.  500 photons cross a lone slab once each on entry
    # (there the specular term, ((n - 1) / (n + 1))^2 = 2.5e-19, is the Fresnel event) and once on leaving, which is what F
    # counts: 500, not the 1000 of the two-layer scene.  Reflected may be 0: R is 1e-19 and 1e-15 but for total reflection
    "n_slab_1e-9_in_air": {"F": dict(crossed=500), "H": dict(specular=2.4e-19)},
    # the two-layer scene: 557 transmissions from layer to layer (R = 6e-16 between 1.4 and 1.4 (1 + 1e-7), 1e-15 into the
    # matched ambient below) and 496 exits, 1053 crossings (oracle and device alike); 1000 layer-to-layer ones would take more
    # than the 500 photons every edge scene has
    "n_two_layers_1e-7": {"F": dict(crossed=1000, transmitted=500)},
    "s_sliver": {"A": dict(carried=1000), "F": dict(transmitted=1000)},
    "w_albedo_to_1": {"I": dict(capped=100), "J": dict(deposits=9000)},
    "w_albedo_to_0": {"E": dict(roulette_died=400, roulette_survived=50)},
    "m_dense": {"F": dict(total_internal=50), "J": dict(voxels_hit=100, deposits=15000)},
    "z_grazing": {"H": dict(specular=0.98), "F": dict(total_internal=500)},       # (normal incidence: 0.0278)
}


def check_result(res, name, worst_allowed=None):
    """The conditions every audited run meets: no violation, no declined decision, the designed rules within their caps,
    the scene's events present.  worst_allowed: the oracle's recorded figures (the CPU test keeps that table honest)."""
    for k, r in res.items():
        assert r["violations"] == 0, "%s, check %s: %d violations\n%s" % (name, k, r["violations"], report(res))
        assert r["declined"] == 0, "%s, check %s: %d decisions too close to call" % (name, k, r["declined"])
        for m, w in r["worst"].items():
            assert w <= tol(name)[m], (name, m, w)
            if worst_allowed is not None and m in worst_allowed:
                assert w <= worst_allowed[m], "%s: the oracle's %s = %.3g exceeds the recorded %.3g" % (name, m, w, worst_allowed[m])
    scat = res["C"]["n"]
    assert res["C"]["pole"] < 0.01 * max(scat, 1)                      # the near-pole approximation stays rare
    assert res["J"]["ambiguous"] <= 1e-4 * res["J"]["deposits"]        # deposits on a voxel face
    if "hidden" in res["G"]:
        assert res["G"]["hidden"] == 0 and res["G"]["leaks"] == 0
    for k, want in OCCURRED[name].items():
        for key, least in want.items():
            got = res[k]["fates"][key] if k == "I" else res[k][key]
            assert got >= least, "%s: %s[%s] = %s, the scene exists for at least %s" % (name, k, key, got, least)
