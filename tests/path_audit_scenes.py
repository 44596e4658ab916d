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
}


def check_result(res, name, worst_allowed=None):
    """The conditions every audited run meets: no violation, no declined decision, the designed rules within their caps,
    the scene's events present.  worst_allowed: the oracle's recorded figures (the CPU test keeps that table honest)."""
    for k, r in res.items():
        assert r["violations"] == 0, "%s, check %s: %d violations\n%s" % (name, k, r["violations"], report(res))
        assert r["declined"] == 0, "%s, check %s: %d decisions too close to call" % (name, k, r["declined"])
        for m, w in r["worst"].items():
            assert w <= PA.TOL[m], (name, m, w)
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
