"""The walk's Henyey-Greenstein deflection over the whole range of g that lt_set_media accepts, one row per query, in both
precisions -- here through the CPU oracle and through a NumPy restatement of the form the walk has adopted (so that the
bounds are proven reachable without a device); tests/test_gpu_hg_walk.py runs the same rows through LT_FN_HG_WALK.

What this found: the quotient form ((1 + g^2) - t^2) / (2 g) cancels as g -> 0.  In float it is 1e-4 off
at g = 1e-3, leaves [-1, 1] from g = 1e-4 down (|c| reaches 1.07 at 1e-6) and gives cos = 0 for EVERY draw from |g| = 1e-8
down; in double it is 1e-10 off at g = 1e-6 and 7e-5 at 1e-12.  Below |g| = 2^-6 the walk now takes hg_small_g (lt_device.hpp).

The reference is the exact inverse CDF in long double (path_audit.hg_inverse) of the USER's g, so the host's record builder is
covered too.  A row passes on the CDF, |CDF(c) - xi| <= tol_cdf; for |g| >= 0.99, where the CDF is ill-conditioned in the
cosine and the cosine in the CDF, on either that or |c - c_exact(xi)| <= tol_cos (the criterion of path_audit's check C).

    precision   tol_cdf   tol_cos   from
    f64         1e-11     1e-14     path_audit.TOL: C.cdf, C.cos (16 x the oracle's worst over the audit's scenes)
    f32         1e-3      1e-4      16 x the worst of TEXTBOOK_F32 below, rounded up to a power of ten

TEXTBOOK_F32: a plain NumPy float32 restatement of the textbook quotient form over the ordinary g's 0.9, 0.8, 0.5, 0.3, -0.4
and this file's draws -- never the device's figure: cosine 7.7e-7, CDF 7.0e-6.

The worst deviations of this restatement, of the oracle and of an MI355X are tabulated in tests/test_gpu_hg_walk.py.
"""
import numpy as np
import pytest

from oracle import oracle as O
from tests import path_audit as PA
from tests import scenes as S

LD = PA.LD
G_ABS = (1e-12, 1e-9, 1e-6, 1e-4, 1e-3, 1e-2, 0.3, 0.9, 0.99, 0.999)
G_ALL = tuple(s * g for g in G_ABS for s in (1.0, -1.0))
K_EDGE = np.array([0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 2, 2 ** 32 - 1], dtype=np.uint64)
N_RANDOM = 20000
SMALL_G = 0.015625           # kHgSmallG (lt_internal.hpp): |g| below it is sampled by hg_small_g
TEXTBOOK_F32 = {"cos": 7.7e-7, "cdf": 7.0e-6}
def _pow10(x):
    return 10.0 ** int(np.ceil(np.log10(x) - 1e-12))


TOL = {"f64": dict(cdf=PA.TOL["C.cdf"], cos=PA.TOL["C.cos"]),
       "f32": dict(cdf=_pow10(16 * TEXTBOOK_F32["cdf"]), cos=_pow10(16 * TEXTBOOK_F32["cos"]))}


def draws(seed=5):
    """Raw 32-bit draws: the six edge values and N_RANDOM random ones (shared by every g)."""
    rs = np.random.RandomState(seed)
    return np.concatenate([K_EDGE, rs.randint(0, 2 ** 32, size=N_RANDOM, dtype=np.uint64)])


def xis(f32):
    """The uniforms the walk makes of the draws, as doubles: (k + 1) 2^-32 exactly (the f64 walk); in f32 that value rounded
    to float and, beside it, 2^-32 + float(k) 2^-32 in float arithmetic as rocrand_uniform computes it (xi = 1.0f occurs)."""
    k = draws()
    exact = (k.astype(np.float64) + 1.0) * 2.0 ** -32
    if not f32:
        return exact
    p = np.float32(2.0 ** -32)
    rr = p + k.astype(np.float32) * p
    assert rr.dtype == np.float32 and rr.max() == 1.0 and rr.min() > 0
    return np.concatenate([exact.astype(np.float32), rr]).astype(np.float64)


def record(g, f32):
    """The 12-value medium record lt_layer_records builds for the half space (0.1, 10, g, 1.0) in that precision."""
    from light_transport_amd import _lib
    m, _, _ = _lib.layer_records([(0.1, 10.0, g, 1.0)], [0.0, np.inf], [0], f32=f32)
    return m[0]


def rows(g, f32):
    """[n, 14] rows of LT_FN_HG_WALK: xi, the f32 flag, the medium record."""
    xi = xis(f32)
    r = np.empty((xi.size, 14))
    r[:, 0], r[:, 1], r[:, 2:] = xi, 1.0 if f32 else 0.0, record(g, f32).astype(np.float64)
    return r


MED = dict(g=3, one_m_g2=5, one_p_g2=6, inv_2g=7, one_m_g=9, two_g=10)      # fields of the record (tests/test_layer_record.py)


def restated(xi, rec, dt):
    """hg_sample_walk (lt_device.hpp) in plain NumPy arithmetic of the walk's precision, every operation rounded on its own."""
    xi = xi.astype(dt)
    f = {k: dt(rec[i]) for k, i in MED.items()}
    with np.errstate(all="ignore"):
        if f["inv_2g"] == 0:
            g = dt(0.5) * f["two_g"]
            s = dt(2) * xi - dt(1)
            d = g * s + dt(1)
            num = g * (dt(1) - s * s) * (g * (dt(2) * s - g) + dt(3))
            return np.clip(s + num / (dt(2) * (d * d)), dt(-1), dt(1))
        t = f["one_m_g2"] / (f["two_g"] * xi + f["one_m_g"])
        return np.clip((f["one_p_g2"] - t * t) * f["inv_2g"], dt(-1), dt(1))


def textbook_f32(xi, g):
    """The textbook quotient form in float32, nothing precomputed."""
    g, xi, one, two = np.float32(g), xi.astype(np.float32), np.float32(1), np.float32(2)
    t = (one - g * g) / (one - g + two * g * xi)
    return (one + g * g - t * t) / (two * g)


def deviations(c, xi, g):
    """(CDF deviation, cosine deviation) of cosines c taken for uniforms xi in a medium of the user's g, in long double."""
    c, xi = np.asarray(c, dtype=np.float64).astype(LD), np.asarray(xi, dtype=np.float64).astype(LD)
    return np.abs(PA.hg_cdf(np.clip(c, -1, 1), LD(g)) - xi), np.abs(c - PA.hg_inverse(xi, LD(g)))


def check(c, xi, g, f32, what):
    """The assertions of one g: the criterion of the module docstring and |c| <= 1 + 4 ulp.  Returns the worst figures."""
    tol = TOL["f32" if f32 else "f64"]
    cdf_dev, cos_dev = deviations(c, xi, g)
    ulp = 2.0 ** -23 if f32 else 2.0 ** -52
    assert np.all(np.isfinite(c)), (what, g)
    assert np.abs(c).max() <= 1 + 4 * ulp, (what, g, np.abs(c).max() - 1)
    hard = abs(g) >= 0.99
    on_cdf = cdf_dev <= tol["cdf"]
    ok = on_cdf | (cos_dev <= tol["cos"]) if hard else on_cdf
    # the figures the criterion judges: the CDF's for |g| < 0.99, and for |g| >= 0.99 the cosine's on the rows the CDF fails
    worst = dict(cdf=0.0 if hard else float(cdf_dev.max()), cos=float(cos_dev[~on_cdf].max(initial=0.0)) if hard else 0.0,
                 cdf_all=float(cdf_dev.max()), cos_all=float(cos_dev.max()), over_one=float(np.abs(c).max() - 1))
    print("%-10s %s g=%+.3e cdf %.2e cos %.2e (all rows: cdf %.2e cos %.2e) |c|-1 %.1e" % (
        what, "f32" if f32 else "f64", g, worst["cdf"], worst["cos"], worst["cdf_all"], worst["cos_all"], worst["over_one"]))
    assert ok.all(), (what, g, int((~ok).sum()), worst)
    return worst


def test_f32_tolerances_come_from_the_textbook_form_at_ordinary_g():
    """The tabulated TEXTBOOK_F32 figures are what the float32 textbook form gives on this file's draws, and the f32
    tolerances are 16 x them, rounded up to a power of ten."""
    xi = xis(True)
    worst = dict(cos=0.0, cdf=0.0)
    for g in (0.9, 0.8, 0.5, 0.3, -0.4):
        cdf_dev, cos_dev = deviations(textbook_f32(xi, g), xi, float(np.float32(g)))
        worst = dict(cos=max(worst["cos"], float(cos_dev.max())), cdf=max(worst["cdf"], float(cdf_dev.max())))
    print(worst)
    for k in worst:
        assert 0.5 * TEXTBOOK_F32[k] < worst[k] <= TEXTBOOK_F32[k], (k, worst[k])
    assert TOL["f32"] == dict(cdf=1e-3, cos=1e-4) and TOL["f64"] == dict(cdf=1e-11, cos=1e-14)


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("g", G_ALL)
def test_restated_walk_form_meets_the_bounds(g, f32):
    """The form the walk adopted, restated in NumPy: the bounds of the GPU test are reachable."""
    r = rows(g, f32)
    rec = record(g, f32)
    assert (rec[MED["inv_2g"]] == 0) == (abs(g) < SMALL_G) and rec[MED["two_g"]] != 0
    check(restated(r[:, 0], rec, np.float32 if f32 else np.float64).astype(np.float64), r[:, 0], g, f32, "restated")


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("g", G_ALL)
def test_oracle_walk_form_meets_the_bounds(g, f32):
    """The oracle's hg_sample_walk, f64 and f32 (its lto_eval takes the same rows and reads g from the record)."""
    r = rows(g, f32)
    out = O.eval_fn("HG_WALK", r)
    assert np.array_equal(out[:, 0], out[:, 1])
    check(out[:, 0], r[:, 0], g, f32, "oracle")


def test_the_old_form_fails_these_bounds():
    """Not vacuous: the quotient form at every g, as the parent had it, misses them -- in f32 from |g| = 1e-3 down (and
    leaves [-1, 1]), in f64 from 1e-6 down."""
    for f32, gs in ((True, (1e-3, 1e-6, -1e-9)), (False, (1e-6, -1e-9, 1e-12))):
        dt = np.float32 if f32 else np.float64
        for g in gs:
            r = rows(g, f32)
            gg, xi = dt(g), r[:, 0].astype(dt)
            t = (dt(1) - gg * gg) / ((dt(2) * gg) * xi + (dt(1) - gg))
            c = ((dt(1) + gg * gg) - t * t) * (dt(1) / (dt(2) * gg))
            with pytest.raises(AssertionError):
                check(c.astype(np.float64), r[:, 0], g, f32, "old form")
    xi = xis(True).astype(np.float32)
    g = np.float32(1e-9)
    t = (np.float32(1) - g * g) / ((np.float32(2) * g) * xi + (np.float32(1) - g))
    assert np.all(((np.float32(1) + g * g) - t * t) * (np.float32(1) / (np.float32(2) * g)) == 0)     # every draw: 90 degrees


def test_g_zero_and_above_the_switch_are_the_parents_bits():
    """g = 0 is 2 xi - 1 to the bit through the new branch; from |g| = 2^-6 up the record and the form are the parent's."""
    for f32 in (False, True):
        dt = np.float32 if f32 else np.float64
        xi = xis(f32)
        rec0 = record(0.0, f32)
        assert rec0[MED["inv_2g"]] == 0 and rec0[MED["two_g"]] == 0
        assert np.array_equal(restated(xi, rec0, dt), dt(2) * xi.astype(dt) - dt(1))
        r0 = np.empty((xi.size, 14)); r0[:, 0], r0[:, 1], r0[:, 2:] = xi, float(f32), rec0
        assert np.array_equal(O.eval_fn("HG_WALK", r0)[:, 0], (dt(2) * xi.astype(dt) - dt(1)).astype(np.float64))
        for g in (SMALL_G, -SMALL_G, 0.3, -0.4, 0.9):
            rec = record(g, f32)
            assert rec[MED["inv_2g"]] == dt(1) / (dt(2) * dt(g))
        assert record(float(np.nextafter(dt(SMALL_G), dt(0))), f32)[MED["inv_2g"]] == 0      # the next g below the switch


# ---------------------------------------------------------------- a g that rounds to +-1 in float
@pytest.mark.parametrize("g", [1 - 1e-9, -(1 - 1e-9), 1 - 2.0 ** -26, -(1 - 2.0 ** -26)])
def test_f32_record_of_a_g_that_rounds_to_one_gives_finite_cosines(g):
    """lt_set_media accepts |g| < 1 in double; float(0.999999999) is 1.0f, where the record had 1 - g = 0 (and at g = -1.0f a
    denominator 2 - 2 xi = 0 at xi = 1.0f: NaN).  The host narrows such a g to the largest float below 1: the record yields a
    finite cosine in [-1, 1] for every draw."""
    assert abs(g) < 1 and abs(np.float32(g)) == 1
    rec = record(g, True)
    assert abs(rec[MED["g"]]) == np.nextafter(np.float32(1), np.float32(0)) and np.sign(rec[MED["g"]]) == np.sign(g)
    assert rec[MED["one_m_g"]] > 0 and rec[MED["one_m_g2"]] > 0
    c = restated(xis(True), rec, np.float32)
    assert np.all(np.isfinite(c)) and np.abs(c).max() <= 1, (g, c.min(), c.max())
    out = O.eval_fn("HG_WALK", rows(g, True))[:, 0]
    assert np.all(np.isfinite(out)) and np.abs(out).max() <= 1
    assert np.array_equal(record(g, False)[MED["g"]], np.float64(g))          # the f64 record keeps g


# ---------------------------------------------------------------- f32 end to end: the bound of the GPU test is not vacuous
SLAB_G = (1e-8, -1e-6, 1e-4)
N_SLAB = 200000


def slab_problem(g):
    """A matched slab (0.1, 10, g, 1.0), 0.2 thick, 32^3 grid."""
    return S.slab(n=32, voxel=0.05, media=((0.1, 10.0, g, 1.0),), thickness=0.2)


def fractions(c):
    n = float(c["photons"])
    return np.array([c["w_absorbed"] / n, c["w_escaped_top"] / n, c["w_escaped_bottom"] / n])


def sigma_d(a, b, n):
    """Standard error of the difference of two independent n-photon estimates a, b of a fraction: each photon's contribution
    lies in [0, 1], so its variance is at most x (1 - x) (tests/test_slab_as_mesh.py)."""
    return np.sqrt((a * (1 - a) + b * (1 - b)) / n)


_f64_slab = {}


def oracle_f64_slab(g):
    """The f64 oracle's counters of the slab at that g (seed 2), once."""
    if g not in _f64_slab:
        _, _, c = slab_problem(g).oracle().run(N_SLAB, seed=2, threads=8)
        assert abs(O.conservation_residual(c)) < 1e-9 * N_SLAB
        _f64_slab[g] = c
    return _f64_slab[g]


@pytest.mark.parametrize("g", SLAB_G)
def test_oracle_f32_slab_agrees_and_planted_right_angles_do_not(g):
    """The oracle's f32 walk against its f64 walk at the same tiny g: absorbed, top and bottom fractions within 5 sigma_d.
    With the old form's failure planted (cos theta = 0 at every scattering: oracle.plant_cos0) the same comparison misses
    the bound: the absorbed fraction is 9.8 sigma_d off at each of the three g (the top fraction 4.0, the bottom 0.2), where
    the sound f32 walk is 0.06, 1.5 and 1.4 sigma_d off."""
    ref = fractions(oracle_f64_slab(g))
    _, _, c = slab_problem(g).oracle().run(N_SLAB, seed=1, threads=8, walk_f32=True)
    got = fractions(c)
    sd = sigma_d(got, ref, N_SLAB)
    print("g=%g f32 vs f64: %s sigma_d" % (g, np.round((got - ref) / sd, 2)))
    assert np.all(np.abs(got - ref) <= 5 * sd), (g, got, ref)
    assert abs(O.conservation_residual(c)) < 2e-6 * N_SLAB
    O.plant_cos0(True)
    try:
        _, _, cp = slab_problem(g).oracle().run(N_SLAB, seed=1, threads=8, walk_f32=True)
    finally:
        O.plant_cos0(False)
    bad = fractions(cp)
    miss = np.abs(bad - ref) / sigma_d(bad, ref, N_SLAB)
    print("g=%g planted cos = 0: %s sigma_d" % (g, np.round(miss, 2)))
    assert miss.max() > 5, (g, miss)
