"""GPU suite of the finite-beam response: lt_tally_convolve, lt_tally_convolve_sep, lt_tally_convolve_at and the PhotonTracer
methods on top, against NumPy on grids of known (seeded random) contents and against the CPU oracle end to end.

Reference.  NumPy, float64: the grid as weight, zero-padded, shifted and added tap by tap; for the separable call the same two
passes, x first.

Bound.  Every term is non-negative, so ANY order of n products (fused or not) is within n 2^-53 of the exact sum, relative --
the device's and NumPy's alike -- and the two differ by at most (n + 2) 2^-52 ref per voxel: n = kh kw for the 2-D and the _at
form, n = kh + kw + 2 for the separable form (the intermediate's error passes through the second pass unchanged); the + 2 covers
the u64 -> double conversion and second-order terms.  Where ref == 0 the result is exactly 0."""

import numpy as np
import pytest

import light_transport_amd as lt
from light_transport_amd import _lib
from light_transport_amd.src import photon_tracing as PT
from light_transport_amd.src.beam_profiles import GaussianProfile
from tests import scenes as S

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (64, 1, 3), (37, 19, 11), (130, 70, 5), (16, 16, 40)]     # (nx, ny, nz)
DTYPES = ["u64fx", "f64", "f32"]
E_INVALID, E_STATE, E_UNSUPPORTED = -1, -2, -5
TAPS_2D = [(1, 3), (5, 1), (5, 7), (33, 33)]         # (kh, kw); (63, 63) -- larger than the grid in both axes -- on (37, 19, 11)
TAPS_SEP = [(3, 3), (33, 9)]                         # (255, 255) on (130, 70, 5)
_grids = {}


def random_grid(shape, dtype):
    """[nz, ny, nx], seeded: u64 values below 2^40; floats in [0, 1) with a quarter of the voxels zero.  Shared, read-only."""
    key = (shape, dtype)
    if key not in _grids:
        nx, ny, nz = shape
        rs = np.random.RandomState(2000 + 7 * SHAPES.index(shape) + DTYPES.index(dtype))
        if dtype == "u64fx":
            g = rs.randint(0, 2 ** 40, size=(nz, ny, nx), dtype=np.uint64)
        else:
            g = rs.random_sample((nz, ny, nx))
            g[rs.random_sample((nz, ny, nx)) < 0.25] = 0.0
            g = g.astype(np.float32 if dtype == "f32" else np.float64)
        g.setflags(write=False)
        _grids[key] = g
    return _grids[key]


def as_weight(g):
    return g.astype(np.float64) * 2.0 ** -40 if g.dtype == np.uint64 else g.astype(np.float64)


def load(ctx, shape, dtype, grid=None):
    nx, ny, nz = shape
    ctx.set_grid(shape, (-0.5 * nx * 0.1, -0.5 * ny * 0.2, 0.0), (0.1, 0.2, 0.3), dtype)
    g = random_grid(shape, dtype) if grid is None else grid
    ctx.write_grid(g)
    return g


def random_taps(kh, kw, seed=0):
    """Asymmetric, non-negative, a few of them zero."""
    rs = np.random.RandomState(31 * kh + kw + seed)
    t = rs.random_sample((kh, kw)) + 0.01
    if t.size > 4:
        t[rs.random_sample((kh, kw)) < 0.1] = 0.0
    return t


def conv_numpy(w, taps):
    """out[z, y, x] = sum_j,i taps[j, i] w[z, y - (j - kh/2), x - (i - kw/2)], w = 0 outside: zero-padded shifted adds."""
    kh, kw = taps.shape
    nz, ny, nx = w.shape
    p = np.pad(w, ((0, 0), (kh // 2, kh // 2), (kw // 2, kw // 2)))
    out = np.zeros_like(w)
    for j in range(kh):
        for i in range(kw):
            out += taps[j, i] * p[:, kh - 1 - j:kh - 1 - j + ny, kw - 1 - i:kw - 1 - i + nx]
    return out


def conv_numpy_sep(w, tx, ty):
    return conv_numpy(conv_numpy(w, tx[None, :]), ty[:, None])


def assert_within(got, ref, n, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == np.float64, what
    err, bound = np.abs(got - ref), (n + 2) * 2.0 ** -52 * ref
    print("%s: max |got - ref| / ref = %.3g, max err / bound = %.3g" % (
        what, float(np.max(err / np.where(ref > 0, ref, 1.0), initial=0.0)), float(np.max(err / np.where(bound > 0, bound, 1.0), initial=0.0))))
    assert np.all(err <= bound), what
    assert not got[ref == 0].any(), what


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def z_ranges(nz):
    r = [(0, 1), (nz - 1, 1)]
    if nz >= 5:
        r.append((nz // 3, nz // 3 + 1))
    return r


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_convolve_2d_within_bound_repeatable_and_plane_by_plane(ctx, shape, dtype):
    w = as_weight(load(ctx, shape, dtype))
    for kh, kw in TAPS_2D + ([(63, 63)] if shape == (37, 19, 11) else []):
        taps = random_taps(kh, kw)
        got = ctx.tally_convolve(taps)
        assert_within(got, conv_numpy(w, taps), kh * kw, "%s %s %dx%d" % (shape, dtype, kh, kw))
        assert same_bits(got, ctx.tally_convolve(taps)), "a second call gave other bits"
        for z0, n in z_ranges(shape[2]):
            assert same_bits(ctx.tally_convolve(taps, (z0, n)), got[z0:z0 + n]), "planes %d + %d differ from the full result" % (z0, n)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_convolve_separable_within_bound_repeatable_and_plane_by_plane(ctx, shape, dtype):
    w = as_weight(load(ctx, shape, dtype))
    for kh, kw in TAPS_SEP + ([(255, 255)] if shape == (130, 70, 5) else []):
        tx, ty = random_taps(1, kw, 1)[0], random_taps(kh, 1, 2)[:, 0]
        got = ctx.tally_convolve((tx, ty))
        assert_within(got, conv_numpy_sep(w, tx, ty), kh + kw + 2, "%s %s separable %d+%d" % (shape, dtype, kh, kw))
        assert same_bits(got, ctx.tally_convolve([tx, ty])), "a second call gave other bits"
        for z0, n in z_ranges(shape[2]):
            assert same_bits(ctx.tally_convolve((tx, ty), (z0, n)), got[z0:z0 + n]), "planes %d + %d differ from the full result" % (z0, n)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_the_single_tap_one_returns_the_grid(ctx, shape, dtype):
    load(ctx, shape, dtype)
    g = ctx.read_grid()
    assert same_bits(ctx.tally_convolve(np.array([[1.0]])), g)
    assert same_bits(ctx.tally_convolve((np.array([1.0]), np.array([1.0]))), g)


def _delta_cases(shape):
    nx, ny, nz = shape
    return [(0, 0, 0), (nz - 1, ny - 1, nx - 1), (nz // 2, 0, nx // 2), (1, ny // 2, nx - 1), (nz // 2, ny // 2, nx // 2)]     # corners, edges, interior


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_voxel_is_answered_by_the_kernel_laid_about_it(ctx, dtype):
    """Centring, orientation and edges, bit for bit: a grid of zeros with the one value 1.0 convolved with distinct taps is the
    kernel laid about that voxel -- tap (j, i) lands (j - kh/2, i - kw/2) from it -- clipped at the grid's edge, exactly zero
    elsewhere.  A correlation would lay the kernel down mirrored, a centre off by one would shift it."""
    shape = (37, 19, 11)
    nx, ny, nz = shape
    k2 = 1.0 + np.arange(35, dtype=np.float64).reshape(7, 5)                    # kh = 7, kw = 5, asymmetric under both flips
    tx, ty = np.array([1.0, 2, 3, 4, 5, 6, 7]), np.array([11.0, 13, 17, 19, 23])
    one = {"u64fx": np.uint64(2 ** 40), "f64": np.float64(1.0), "f32": np.float32(1.0)}[dtype]
    for z, y, x in _delta_cases(shape):
        g = np.zeros((nz, ny, nx), dtype=_lib.TALLY_NP[_lib.TALLY[dtype]])
        g[z, y, x] = one
        load(ctx, shape, dtype, g)
        for taps, form in ((k2, k2), (np.outer(ty, tx), (tx, ty))):
            assert same_bits(ctx.tally_convolve(form), want2d(taps, (nz, ny, nx), (z, y, x))), "voxel (%d, %d, %d), %s" % (z, y, x, "2-D" if form is k2 else "separable")
        cols = np.array([[x, y], [min(x + 1, nx - 1), y], [x, max(y - 2, 0)]], dtype=np.int32)
        at = ctx.tally_convolve_at(k2, cols)
        assert same_bits(at, want2d(k2, (nz, ny, nx), (z, y, x))[:, cols[:, 1], cols[:, 0]])


def want2d(taps, dims, at):
    """The kernel laid about the voxel ``at`` = (z, y, x) of a grid of ``dims`` = (nz, ny, nx), clipped."""
    nz, ny, nx = dims
    z, y, x = at
    kh, kw = taps.shape
    out = np.zeros(dims)
    for j in range(kh):
        for i in range(kw):
            yy, xx = y + (j - kh // 2), x + (i - kw // 2)
            if 0 <= yy < ny and 0 <= xx < nx:
                out[z, yy, xx] = taps[j, i]
    return out


@pytest.mark.parametrize("dtype", DTYPES)
def test_convolve_at_listed_columns(ctx, dtype):
    for shape, cols in (((37, 19, 11), np.array([[0, 0], [36, 0], [0, 18], [36, 18], [18, 9], [1, 17], [35, 3], [20, 0]], dtype=np.int32)),
                        ((130, 70, 5), None), ((1, 1, 1), np.array([[0, 0]], dtype=np.int32))):
        nx, ny, nz = shape
        if cols is None:
            rs = np.random.RandomState(5)
            cols = np.stack([rs.randint(0, nx, 4096), rs.randint(0, ny, 4096)], axis=1).astype(np.int32)
        w = as_weight(load(ctx, shape, dtype))
        for kh, kw in ((5, 7), (33, 33)) + (((63, 63),) if shape == (37, 19, 11) else ()):
            taps = random_taps(kh, kw)
            got = ctx.tally_convolve_at(taps, cols)
            assert got.shape == (nz, len(cols))
            assert_within(got, conv_numpy(w, taps)[:, cols[:, 1], cols[:, 0]], kh * kw, "%s %s at %d columns, %dx%d" % (shape, dtype, len(cols), kh, kw))
            assert same_bits(got, ctx.tally_convolve_at(taps, cols)), "a second call gave other bits"
        tx, ty = random_taps(1, 9, 1)[0], random_taps(5, 1, 2)[:, 0]
        assert same_bits(ctx.tally_convolve_at((tx, ty), cols), ctx.tally_convolve_at(np.outer(ty, tx), cols))


def test_the_grid_and_the_counters_are_left_alone(ctx):
    g = load(ctx, (37, 19, 11), "u64fx")
    c0 = ctx.read_counters()
    ctx.tally_convolve(random_taps(5, 7))
    ctx.tally_convolve((random_taps(1, 9)[0], random_taps(3, 1)[:, 0]), (2, 3))
    ctx.tally_convolve_at(random_taps(5, 7), np.array([[3, 4]]))
    assert np.array_equal(ctx.read_grid_raw(), g) and ctx.read_counters() == c0


def test_argument_errors_at_the_c_level(ctx):
    g = load(ctx, (37, 19, 11), "f64")
    nz, ny, nx = g.shape
    L, dp = _lib.lib(), _lib._dp
    out = np.empty(g.shape)
    ok = np.ones((65, 65))
    msg = lambda: L.lt_last_error(ctx._h)      # noqa: E731
    conv = lambda t, kh, kw, z0=0, n=nz, o=out: L.lt_tally_convolve(ctx._h, dp(t), kh, kw, z0, n, dp(o) if o is not None else None)      # noqa: E731
    sep = lambda a, kw, b, kh, z0=0, n=nz, o=out: L.lt_tally_convolve_sep(ctx._h, dp(a), kw, dp(b), kh, z0, n, dp(o) if o is not None else None)      # noqa: E731
    cols = np.zeros((4097, 2), dtype=np.int32)
    out_at = np.empty((nz, 4097))      # [nz][n_columns]: larger than a plane of this grid
    at = lambda t, kh, kw, c=cols, n=1, o=out_at: L.lt_tally_convolve_at(ctx._h, dp(t), kh, kw, _lib._ip(c), n, dp(o) if o is not None else None)      # noqa: E731
    line = np.ones(257)
    assert conv(ok, 3, 5) == 0 and sep(line, 5, line, 3) == 0 and at(ok, 3, 5) == 0 and conv(ok, 63, 63, 0, 1) == 0 and sep(line, 255, line, 255, 0, 1) == 0
    for bad in (-1e-300, -1.0, np.nan, np.inf, -np.inf):
        t = np.ones((3, 5))
        t[2, 4] = bad
        assert conv(t, 3, 5) == E_INVALID and at(t, 3, 5) == E_INVALID
        assert sep(t[2], 5, line, 3) == E_INVALID and sep(line, 5, t[2], 5) == E_INVALID
    for kh, kw in ((2, 3), (3, 4), (0, 3), (3, 0), (-1, 3), (64, 3)):
        assert conv(ok, kh, kw) == E_INVALID and at(ok, kh, kw) == E_INVALID and sep(line, kw, line, kh) == E_INVALID
    assert conv(ok, 65, 3) == E_UNSUPPORTED and b"65" in msg()
    assert conv(ok, 3, 65) == E_UNSUPPORTED and b"65" in msg()
    assert at(ok, 65, 3) == E_UNSUPPORTED and b"65" in msg()
    assert sep(line, 65, line, 65, 0, 1) == 0
    assert sep(line, 257, line, 3) == E_UNSUPPORTED and b"257" in msg()
    assert sep(line, 3, line, 257) == E_UNSUPPORTED and b"257" in msg()
    assert at(ok, 3, 5, cols, 4096) == 0
    assert at(ok, 3, 5, cols, 4097) == E_UNSUPPORTED and b"4097" in msg()
    assert at(ok, 3, 5, cols, 0) == E_INVALID and at(ok, 3, 5, None, 1) == E_INVALID
    for bad in ((nx, 0), (0, ny), (-1, 0), (0, -1)):
        c = np.array([[1, 1], bad], dtype=np.int32)
        assert at(ok, 3, 5, c, 2) == E_INVALID and at(ok, 3, 5, c, 1) == 0
    for z0, n in ((-1, 1), (0, 0), (0, nz + 1), (nz, 1), (nz - 1, 2), (2 ** 31 - 1, 2 ** 31 - 1)):
        assert conv(ok, 3, 5, z0, n) == E_INVALID and sep(line, 5, line, 3, z0, n) == E_INVALID
    assert conv(ok, 3, 5, o=None) == E_INVALID and sep(line, 5, line, 3, o=None) == E_INVALID and at(ok, 3, 5, o=None) == E_INVALID
    assert conv(None, 3, 5) == E_INVALID and sep(None, 5, line, 3) == E_INVALID and sep(line, 5, None, 3) == E_INVALID and at(None, 3, 5) == E_INVALID


def test_argument_errors_through_the_context(ctx):
    load(ctx, (37, 19, 11), "f32")
    good = np.ones((3, 5))
    bad_values = [np.where(np.arange(15).reshape(3, 5) == 7, v, 1.0) for v in (-1.0, np.nan)]
    for t in bad_values + [np.ones((2, 3)), np.ones((3, 4)), np.ones((65, 3)), np.ones((3, 65))]:
        with pytest.raises(lt.LtError):
            ctx.tally_convolve(t)
        with pytest.raises(lt.LtError):
            ctx.tally_convolve_at(t, np.array([[0, 0]]))
    for pair in ((np.ones(4), np.ones(3)), (np.ones(3), np.ones(257)), (np.ones(257), np.ones(3)), (np.array([1.0, -1.0, 1.0]), np.ones(3))):
        with pytest.raises(lt.LtError):
            ctx.tally_convolve(pair)
    # wrong shapes and dtypes never reach the library
    for t in (np.ones(3), np.ones((1, 3, 3)), np.ones((3, 3), dtype=complex), np.array([["a"]]), np.ones((0, 3)), (np.ones((3, 3)), np.ones(3))):
        with pytest.raises((lt.LtError, ValueError)):
            ctx.tally_convolve(t)
    for z in ((-1, 1), (0, 0), (0, 12), (11, 1), (10, 2)):
        with pytest.raises((lt.LtError, ValueError)):
            ctx.tally_convolve(good, z)
    for c in (np.zeros((4097, 2), dtype=np.int32), np.array([[37, 0]]), np.array([[0, 19]]), np.array([[0.0, 0.0]]), np.array([0, 0]), np.zeros((0, 2), dtype=np.int32)):
        with pytest.raises((lt.LtError, ValueError)):
            ctx.tally_convolve_at(good, c)
    assert ctx.tally_convolve(good, (10, 1)).shape == (1, 19, 37) and ctx.tally_convolve_at(good, [[36, 18]]).shape == (11, 1)


def test_calls_before_set_grid_give_state_error():
    with lt.Context(0) as fresh:
        L, dp = _lib.lib(), _lib._dp
        t, out, cols = np.ones((3, 3)), np.empty(8), np.zeros((1, 2), dtype=np.int32)
        assert L.lt_tally_convolve(fresh._h, dp(t), 3, 3, 0, 1, dp(out)) == E_STATE
        assert L.lt_tally_convolve_sep(fresh._h, dp(t), 3, dp(t), 3, 0, 1, dp(out)) == E_STATE
        assert L.lt_tally_convolve_at(fresh._h, dp(t), 3, 3, _lib._ip(cols), 1, dp(out)) == E_STATE
        for f in (lambda: fresh.tally_convolve(t), lambda: fresh.tally_convolve((t[0], t[0])), lambda: fresh.tally_convolve_at(t, cols)):
            with pytest.raises(lt.LtError):
                f()


def test_beam_response_of_a_traced_slab_matches_the_oracle(ctx):
    """S.slab(n=32, voxel=0.8), 4096 photons, u64fx -- with the pencil moved from the corner shared by four columns (x = y = 0
    on this even grid) to the centre of column (16, 16): the medium is laterally uniform, and beam_response insists on a
    centred pencil."""
    src = dict(type=0, pos=(0.4, 0.4, 0.0), dir=(0.0, 0.0, 1.0), extra=(0.0,) * 6, start_medium=0)
    prob = S.slab(n=32, voxel=0.8, source=src)
    tr = PT.PhotonTracer(ctx=ctx)
    tr.configure(PT.LayeredSlab([PT.OpticalMedium(*prob.media[0])], [np.inf]), PT.VoxelGrid(prob.grid_shape, prob.origin, 0.8, dtype="u64fx"),
                 PT.PencilBeam(src["pos"], src["dir"]))
    tr.run(4096, seed=123)
    _, fxo, _ = prob.oracle().run(4096, seed=123, want_fx=True, want_f64=False, threads=4)
    assert np.array_equal(tr.absorbed_raw(), fxo)                  # the existing parity: both convolutions see the same grid
    w = as_weight(fxo)
    prof = GaussianProfile(1.6)
    tx, ty = prof.taps((0.8, 0.8))
    assert tx.size == ty.size == 11
    ref = conv_numpy_sep(w, tx, ty)
    resp = tr.beam_response(prof)
    assert_within(resp, ref, tx.size + ty.size + 2, "beam_response")
    assert same_bits(tr.beam_response(prof, (3, 4)), resp[3:7])
    # on the axis, through the _at form (the outer product as a 2-D kernel: kh kw terms)
    axis = tr.beam_profile_at(prof)
    assert axis.shape == (32, 1)
    assert_within(axis[:, 0], conv_numpy(w, np.outer(ty, tx))[:, 16, 16], tx.size * ty.size, "beam_profile_at")
    lateral = tr.beam_profile_at(prof, np.array([[x, 16] for x in range(32)]))
    assert same_bits(lateral[:, 16], axis[:, 0])
    # the edges only lose weight.  Slack: the bound of every voxel of resp, and the roundings of the two 32^3-term sums
    total, taps_sum = w.sum(), tx.sum() * ty.sum()
    assert 0.0 < resp.sum() <= total * taps_sum * (1.0 + (tx.size + ty.size + 4 + 2 * 32 ** 3) * 2.0 ** -52)
