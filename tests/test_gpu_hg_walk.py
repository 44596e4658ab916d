"""The walk's Henyey-Greenstein deflection on the device, one lane per query through LT_FN_HG_WALK (the very hg_sample_walk<R>
of the walk kernels, from the medium table and from the layer record, f64 and f32), over the whole range of g that
lt_set_media accepts; and the f32 walk end to end at tiny g.  Rows, references, criterion and tolerances are those of
tests/test_hg_walk_cpu.py (its docstring derives them); this file adds the device.

Worst deviations over g = +-{1e-12, 1e-9, 1e-6, 1e-4, 1e-3, 1e-2, 0.3, 0.9, 0.99, 0.999}, 20 006 draws per g in f64 and 40 012
in f32 (xi = 1.0f among them).  cdf: |CDF(c) - xi| on the rows the CDF decides; cos: |c - c_exact(xi)| on the rows of
|g| >= 0.99 whose CDF deviation exceeds its tolerance; |c| - 1: the largest excess over 1 (asserted <= 4 ulp).

                            f64 cdf    f64 cos    f64 |c|-1   f32 cdf    f32 cos    f32 |c|-1
    tolerance               1e-11      1e-14      8.9e-16     1e-3       1e-4       4.8e-7
    NumPy restatement       1.8e-14    1.6e-16    0           6.5e-6     7.5e-8     0
    CPU oracle              1.8e-14    1.6e-16    0           6.5e-6     7.5e-8     0
    MI355X                  1.8e-14    1.6e-16    0           6.5e-6     7.5e-8     0

(Over ALL rows of |g| >= 0.99, whichever measure decides them: CDF up to 1.5e-10 in f64 and 6.0e-2 in f32 at the forward peak,
cosine up to 6.4e-13 and 3.9e-4 at the far pole -- why neither measure alone can judge those media.  The device's figures equal
the oracle's to the digits shown: hg_small_g writes its fused multiply-adds out and the oracle takes the same sequence.)

The f32 walk end to end (2e5 photons, seed 1) against the f64 oracle (seed 2), in sigma_d = sqrt((a (1 - a) + b (1 - b)) / n),
bound 5: absorbed -0.05, top +1.45, bottom -1.43 at g = 1e-8 and -1e-6, -0.06 / +1.45 / -1.43 at 1e-4; conservation residual
1.9e-8 n (bound 2e-6 n).  The oracle with cos theta = 0 planted: 9.8 on the absorbed fraction.

The parent's form on the same rows (tests/test_hg_walk_cpu.py::test_the_old_form_fails_these_bounds): f32 cosine 1.2e-4 off at
g = 1e-3, 0.10 at 1e-6 with |c| up to 1.07, cos = 0 for every draw from 1e-8 down; f64 CDF 1.1e-10 off at 1e-6, 7.2e-5 at 1e-12.
"""
import numpy as np
import pytest

from oracle import oracle as O
from tests import test_hg_walk_cpu as H

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("f32", [False, True])
def test_device_walk_form_meets_the_bounds(ctx, f32):
    """Every g of the list in one precision: both overloads agree to the bit, every row meets the criterion and
    |c| <= 1 + 4 ulp.  The worst figures are printed (the table above)."""
    worst = {}
    for g in H.G_ALL:
        r = H.rows(g, f32)
        out = ctx.eval("HG_WALK", r)
        assert np.array_equal(out[:, 0], out[:, 1]), (g, "medium table and layer record disagree")
        w = H.check(out[:, 0], r[:, 0], g, f32, "device")
        worst = {k: max(worst.get(k, -np.inf), v) for k, v in w.items()}
    print("device %s worst: cdf %.2e cos %.2e |c|-1 %.1e" % ("f32" if f32 else "f64", worst["cdf"], worst["cos"], worst["over_one"]))


@pytest.mark.parametrize("f32", [False, True])
def test_device_g_zero_is_two_xi_minus_one(ctx, f32):
    """g = 0 takes the new branch and is 2 xi - 1 to the bit, as it has always been."""
    dt = np.float32 if f32 else np.float64
    r = H.rows(0.0, f32)
    out = ctx.eval("HG_WALK", r)
    want = (dt(2) * r[:, 0].astype(dt) - dt(1)).astype(np.float64)
    assert np.array_equal(out[:, 0], want) and np.array_equal(out[:, 1], want)


@pytest.mark.parametrize("g", [1 - 1e-9, -(1 - 1e-9), 1 - 2.0 ** -26, -(1 - 2.0 ** -26)])
def test_device_f32_g_that_rounds_to_one(ctx, g):
    """The record of a g that rounds to +-1 in float (narrowed by the host: tests/test_hg_walk_cpu.py proves it finite on the
    CPU first), through the query only: finite cosines in [-1, 1], xi = 1.0f included."""
    r = H.rows(g, True)
    out = ctx.eval("HG_WALK", r)
    assert np.all(np.isfinite(out)) and np.abs(out).max() <= 1 and np.array_equal(out[:, 0], out[:, 1])


@pytest.mark.parametrize("g", H.SLAB_G)
def test_f32_walk_at_tiny_g_agrees_with_the_f64_oracle(ctx, g):
    """2e5 photons through the matched slab (0.1, 10, g, 1.0), 0.2 thick: the f32 walk's absorbed, top and bottom fractions
    against the f64 oracle's at the same g within 5 sqrt((a (1 - a) + b (1 - b)) / n) (each photon's share of a fraction lies
    in [0, 1]); conservation to 2e-6 n.  With cos theta = 0 planted the oracle misses this bound by 9.8 sigma_d
    (tests/test_hg_walk_cpu.py), which is what the parent's f32 walk did at g = 1e-8."""
    n = H.N_SLAB
    ref = H.fractions(H.oracle_f64_slab(g))
    prob = H.slab_problem(g)
    prob.apply(ctx, "f32"); ctx.set_tally_mode("auto")
    ctx.zero_tally(); ctx.launch(n, seed=1, f32_walk=True); ctx.sync()
    c = ctx.read_counters()
    assert c["photons"] == n
    got = H.fractions(c)
    sd = H.sigma_d(got, ref, n)
    print("g=%g f32 device vs f64 oracle (absorbed, top, bottom): %s vs %s = %s sigma_d; residual %.2e n"
          % (g, np.round(got, 6), np.round(ref, 6), np.round((got - ref) / sd, 2), abs(O.conservation_residual(c)) / n))
    assert np.all(np.abs(got - ref) <= 5 * sd), (g, got, ref, (got - ref) / sd)
    assert abs(O.conservation_residual(c)) < 2e-6 * n
