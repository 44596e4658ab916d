"""The capture kernels' paths, re-derived event by event from their random draws (tests/path_audit.py): the audit of
tests/test_path_audit_cpu.py (its docstring lists the checks A..J) on what the DEVICE recorded -- lt_set_vertex_capture,
an f64 walk (capture exists for the f64 XORWOW walk only), lt_read_vertices / _counters / _grid.  The shipping kernels are
tied to the oracle bit for bit elsewhere; the oracle (on the CPU) and the capture kernels (here) are tied to the physics.

Worst deviation per measure over all scenes (seed 97): the CPU oracle's, the tolerance that follows from it (16 x, rounded up
to a power of ten, at most 1e-8; path_audit.ORACLE_WORST / TOL), and the kernels' on an MI355X.

    measure                 oracle     tolerance   kernels (MI355X)
    A.tau                   1.12e-11   1e-09       6.63e-12
    B.perp                  1.68e-15   1e-13       1.47e-15
    B.unit                  3.30e-12   1e-10       1.55e-12
    C.cdf                   6.16e-13   1e-11       5.01e-13
    D.azimuth               1.09e-12   1e-10       5.56e-13
    E.weight                1.18e-16   1e-14       1.18e-16
    E.pdf                   3.40e-12   1e-10       2.50e-12
    F.R                     3.65e-13   1e-11       2.23e-13
    F.reflect               0          0 (exact)   0
    F.snell                 5.47e-15   1e-13       1.09e-14
    F.plane                 5.43e-17   1e-15       5.30e-17
    G.plane                 3.06e-16   1e-14       2.97e-16
    G.inside                0          1e-14 (G.plane's: the same point error, within the plane)   0
    G.nearest               5.57e-14   1e-12       2.08e-14
    G.normal                9.06e-17   1e-14       9.06e-17
    G.R                     8.83e-14   1e-11       1.55e-13
    G.reflect               3.70e-16   1e-14       2.62e-16
    G.snell                 1.49e-14   1e-12       2.36e-14
    G.plane_of_incidence    1.06e-16   1e-14       8.83e-17
    H.point                 4.44e-16   1e-14       4.44e-16
    H.dir                   1.47e-15   1e-13       1.56e-15
    H.weight                4.72e-17   1e-15       4.72e-17
    H.pdf                   3.80e-16   1e-14       3.33e-16
    I.sum (ratio to bound)  0.083      1           0.019
    J.voxel (ratio)         0.255      1           0.494

The same over the EDGE scenes (path_audit_scenes.EDGE: tiny and extreme g, near-matched indices, a sliver layer, albedo -> 1
and -> 0, mu_t = 1e5, a grazing beam; 500 photons each, seed 97), which have a table of their own (path_audit.ORACLE_WORST_EDGE /
TOL_EDGE; C.cos, E.pdf_roundings, E.weight_in exist only there).  Before the walk sampled |g| < 2^-6 by hg_small_g, check C
failed on the oracle in exactly the scenes with |g| <= 1e-6: t_g1e-6 6346 of 7697 scatterings (worst 1.1e-10), t_gneg1e-9 and
its fluence twin 7695 (9.7e-8), t_g1e-12 all 7697 (7.2e-5), t_g1e-6_cone 1576 of the 1918 in the cone (1.1e-10); every other
edge scene passed before and after.

    measure                 oracle     tolerance   kernels (MI355X)
    A.tau                   1.03e-11   1e-09       6.28e-12
    B.perp                  4.26e-16   1e-13       4.27e-16
    B.unit                  2.93e-12   1e-10       1.78e-12
    C.cdf                   6.16e-13   1e-11       4.51e-13
    C.cos                   1.81e-16   1e-14       1.56e-16
    D.azimuth               5.29e-13   1e-10       3.21e-13
    E.pdf                   3.40e-12   1e-10       2.50e-12
    E.pdf_roundings         1.11       100         0.372
    E.weight                1.18e-16   1e-14       1.18e-16
    E.weight_in             7.61e-17   1e-14       7.61e-17
    F.R                     5.03e-13   1e-11       2.64e-13
    F.plane                 6.66e-17   1e-14       6.90e-17
    F.reflect               0          0           0
    F.snell                 5.76e-14   1e-12       3.02e-14
    G.R                     2.37e-14   1e-11       5.03e-14
    G.inside                0          1e-14       0
    G.nearest               7.63e-15   1e-12       3.14e-15
    G.normal                6.29e-17   1e-14       6.29e-17
    G.plane                 4.45e-16   1e-14       3.05e-16
    G.plane_of_incidence    1.06e-16   1e-14       8.76e-17
    G.reflect               2.95e-16   1e-14       2.42e-16
    G.snell                 5.47e-14   1e-12       2.03e-14
    H.dir                   1.01e-15   1e-13       1.12e-15
    H.pdf                   3.80e-16   1e-14       3.33e-16
    H.point                 1.92e-16   1e-14       1.92e-16
    H.weight                7.06e-17   1e-14       7.06e-17
    I.sum                   0.095      1           0.0433
    J.voxel                 0.247      1           0.247

Conditions, not measurements (met by the oracle and by the kernels): no reflect / transmit decision within 1e-12 of R, no
deposit within 1e-9 voxel of a face (cap 1e-4 of the deposits), the near-pole approximation at 4 of 64 587 scatterings in
scene (a) (cap 1 %; edge scenes: 84 of 18 825 at g = 0.99, 31 of 4876 at g = -0.99, 0 of 19 000 at g = 0.999 under the tilted beam),
no triangle hidden by the walk's 1e-6 / 1e-7 rules, no leak.
"""
import numpy as np
import pytest

from oracle import oracle as O
from tests import path_audit as PA
from tests import path_audit_scenes as PS

pytestmark = pytest.mark.gpu


def device_capture(ctx, name, dtype="f64"):
    """(grid, counters, vertices, counts) of the device's capturing f64 walk of the scene; capture is switched off again."""
    _, n, k, quantity = PS.SCENES[name]
    prob = PS.problem(name)
    prob.apply(ctx, dtype)
    try:
        ctx.set_tally_quantity(quantity)
        ctx.set_vertex_capture(k)
        ctx.launch(n, seed=PS.SEED); ctx.sync()
        v, cnt = ctx.read_vertices(n)
        c = ctx.read_counters()
        g = ctx.read_grid_raw() if dtype == "u64fx" else ctx.read_grid()
        info = ctx.mesh_accel_info() if prob.mesh is not None else None
    finally:
        ctx.set_vertex_capture(0)
        ctx.set_tally_quantity("absorbed")
    return g, c, v, cnt, info


def device_draws(ctx, name, first=64):
    """The raw draws of the scene's photons: the first 64 ids from the device's generator, asserted equal to the oracle's;
    the rest from the oracle's (one device call per photon is slow)."""
    d = PS.draws(name)
    for pid in range(first):
        np.testing.assert_array_equal(ctx.rng_raw(PS.SEED, pid, d.shape[1]), d[pid])
    return d


@pytest.mark.parametrize("name", list(PS.SCENES))
def test_device_paths_follow_the_textbook_laws(ctx, name):
    g, c, v, cnt, info = device_capture(ctx, name)
    res = PA.audit(PS.plain(PS.problem(name), PS.SCENES[name][3]), device_draws(ctx, name), v, cnt, c, g, tol=PS.tol(name))
    print(name + "\n" + PS.report(res))
    PS.check_result(res, name)
    if name == "g_sphere_march":
        assert info["kind"] & 2            # beyond LDS: the march grid and its kernel
    if name in ("f_cornell", "h_slab_as_mesh", "i_quad_facing_down"):
        assert not info["kind"] & 2        # the mesh in LDS


def test_device_fixed_point_tally_is_the_sum_of_its_deposits(ctx):
    """The u64 fixed-point tally (2^-40 units) of the same walk: +-1 unit per deposit about the rebuilt sums."""
    name = "d_stack"
    g, c, v, cnt, _ = device_capture(ctx, name, "u64fx")
    assert g.dtype == np.uint64 and g.sum() > 0
    res = PA.audit(PS.plain(PS.problem(name)), device_draws(ctx, name, first=4), v, cnt, c, g, grid_kind="u64fx")
    print(name + " u64fx\n" + PS.report(res))
    PS.check_result(res, name)


def test_device_records_are_the_oracles(ctx):
    """What the two audits compare is the same walk: the device's event kinds, media and step indices equal the oracle's."""
    name = "e_tilted_on_top"
    _, c, v, cnt, _ = device_capture(ctx, name)
    _, co, vo, cnto = PS.oracle_capture(name)
    np.testing.assert_array_equal(cnt, cnto)
    live = np.arange(v.shape[1])[None, :] < cnt[:, None]
    for f in ("kind", "medium", "step"):
        np.testing.assert_array_equal(v[f][live], vo[f][live])
    assert c["steps"] == co["steps"]
    assert abs(O.conservation_residual(c)) < 1e-9 * c["photons"]
