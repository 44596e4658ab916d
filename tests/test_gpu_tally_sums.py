"""GPU suite of the tally sums: lt_write_grid, lt_tally_sum_axes, lt_tally_sum_columns and the PhotonTracer methods on top,
against NumPy on grids of known (seeded random) contents and against the CPU oracle end to end.

Bounds.  The u64 fixed-point sums are integers: exact.  Float tallies are widened to f64 and summed in f64; every term is
non-negative, so ANY summation order of n terms is within (n - 1) 2^-53 of the true sum, relative -- the device's and
NumPy's alike -- and the two differ by at most n 2^-52 ref."""
import ctypes as C

import numpy as np
import pytest

import light_transport_amd as lt
from light_transport_amd import _lib
from light_transport_amd.src import photon_tracing as PT
from tests import scenes as S

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (64, 1, 3), (37, 19, 11), (130, 70, 33), (16, 16, 600)]     # (nx, ny, nz)
DTYPES = ["u64fx", "f64", "f32"]
E_INVALID, E_STATE, E_UNSUPPORTED = -1, -2, -5
_grids = {}


def random_grid(shape, dtype):
    """[nz, ny, nx], seeded: u64 values below 2^40; floats in [0, 1) with a quarter of the voxels zero.  Shared, read-only."""
    key = (shape, dtype)
    if key not in _grids:
        nx, ny, nz = shape
        rs = np.random.RandomState(1000 + 7 * SHAPES.index(shape) + DTYPES.index(dtype))
        if dtype == "u64fx":
            g = rs.randint(0, 2 ** 40, size=(nz, ny, nx), dtype=np.uint64)
        else:
            g = rs.random_sample((nz, ny, nx))
            g[rs.random_sample((nz, ny, nx)) < 0.25] = 0.0
            g = g.astype(np.float32 if dtype == "f32" else np.float64)
        g.setflags(write=False)
        _grids[key] = g
    return _grids[key]


def load(ctx, shape, dtype):
    nx, ny, nz = shape
    ctx.set_grid(shape, (-0.5 * nx * 0.1, -0.5 * ny * 0.2, 0.0), (0.1, 0.2, 0.3), dtype)
    g = random_grid(shape, dtype)
    ctx.write_grid(g)
    return g


def sum_axes_of(mask):
    return tuple(ax for ax, bit in ((0, 4), (1, 2), (2, 1)) if not mask & bit)


def assert_float_sums(got, ref, n_terms, what):
    """|got - ref| <= n_terms 2^-52 ref per output (module docstring); n_terms: a number or an array shaped like ref."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == np.float64, what
    err, bound = np.abs(got - ref), np.asarray(n_terms, dtype=np.float64) * 2.0 ** -52 * ref
    print("%s: max |got - ref| / ref = %.3g, max err / bound = %.3g" % (
        what, float(np.max(err / np.where(ref > 0, ref, 1.0), initial=0.0)), float(np.max(err / np.where(bound > 0, bound, 1.0), initial=0.0))))
    assert np.all(err <= bound), what


def column_sums_numpy(g, bins, n_bins, dtype):
    """np.add.at restatement: out[z, bins[y, x]] += g[z, y, x] for every column with a bin >= 0."""
    nz = g.shape[0]
    flat, keep = bins.ravel(), bins.ravel() >= 0
    out = np.zeros((nz, n_bins), dtype=dtype)
    vals = g.reshape(nz, -1)[:, keep].astype(dtype)
    zi = np.broadcast_to(np.arange(nz)[:, None], vals.shape)
    np.add.at(out, (zi, np.broadcast_to(flat[keep][None, :], vals.shape)), vals)
    return out


def column_tables(shape):
    """(name, bins [ny, nx], n_bins) of the tables a shape is summed with."""
    nx, ny, _ = shape
    org, vox = (-0.5 * nx * 0.1, -0.5 * ny * 0.2), (0.1, 0.2)
    tabs = [("radial nr=7", _lib.radial_bins((nx, ny), org, vox, (0.03, -0.07), 0.9, 7), 8)]
    if shape == (130, 70, 33):
        tabs.append(("radial nr=300", _lib.radial_bins((nx, ny), org, vox, (0.03, -0.07), 0.031, 300), 301))
    rs = np.random.RandomState(77 + nx)
    b = rs.randint(0, 4096, size=(ny, nx)).astype(np.int32)
    b[rs.random_sample((ny, nx)) < 0.1] = -1
    tabs.append(("random 4096 bins, a tenth left out", b, 4096))
    return tabs


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_write_grid_round_trip(ctx, shape, dtype):
    g = load(ctx, shape, dtype)
    back = ctx.read_grid_raw()
    assert back.dtype == g.dtype and np.array_equal(back.view(np.uint8), g.view(np.uint8))          # identical bits
    ctx.write_grid(np.zeros_like(g))
    assert not ctx.read_grid_raw().any()


def test_write_grid_leaves_counters_and_resumes_a_run(ctx):
    """A saved tally put back onto the device continues to accumulate: photons [0, 1500) traced, the grid saved and the device
    grid overwritten, the save restored and photons [1500, 4096) traced on top equal one run of all 4096, bit for bit."""
    prob = S.slab(n=32, voxel=0.8)
    prob.apply(ctx, "u64fx")
    ctx.launch(1500, seed=123)
    ctx.sync()
    saved, c0 = ctx.read_grid_raw(), ctx.read_counters()
    assert c0["photons"] == 1500 and saved.any()
    ctx.write_grid(np.full_like(saved, 12345))
    assert ctx.read_counters() == c0
    assert np.all(ctx.read_grid_raw() == 12345)
    ctx.write_grid(saved)
    assert ctx.read_counters() == c0
    ctx.launch(4096 - 1500, seed=123, photon_offset=1500)
    ctx.sync()
    _, fxo, co = prob.oracle().run(4096, seed=123, want_fx=True, want_f64=False, threads=4)
    assert np.array_equal(ctx.read_grid_raw(), fxo)
    assert ctx.read_counters()["steps"] == co["steps"]


@pytest.mark.parametrize("shape", SHAPES)
def test_axis_sums_u64fx_exact(ctx, shape):
    g = load(ctx, shape, "u64fx")
    for mask in range(7):
        ref = g.sum(axis=sum_axes_of(mask), dtype=np.uint64)
        raw = ctx.tally_sum(mask, raw=True)
        assert raw.dtype == np.uint64 and raw.shape == ref.shape and np.array_equal(raw, ref), "mask %d" % mask
        out = ctx.tally_sum(mask)
        assert out.dtype == np.float64 and np.array_equal(out, ref.astype(np.float64) * 2.0 ** -40), "mask %d" % mask
    assert np.array_equal(ctx.tally_sum("zx", raw=True), g.sum(axis=1, dtype=np.uint64))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("shape", SHAPES)
def test_axis_sums_float_within_bound_and_repeatable(ctx, shape, dtype):
    g = load(ctx, shape, dtype)
    wide = g.astype(np.float64)
    for mask in range(7):
        axes = sum_axes_of(mask)
        got = ctx.tally_sum(mask)
        assert_float_sums(got, wide.sum(axis=axes), int(np.prod([g.shape[a] for a in axes])), "%s %s mask %d" % (shape, dtype, mask))
        again = ctx.tally_sum(mask)
        assert np.array_equal(got.view(np.uint64), again.view(np.uint64)), "mask %d: a second call gave other bits" % mask


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_column_sums(ctx, shape, dtype):
    g = load(ctx, shape, dtype)
    total = ctx.tally_sum(0, raw=True) if dtype == "u64fx" else None
    for name, bins, n_bins in column_tables(shape):
        what = "%s %s %s" % (shape, dtype, name)
        count = np.bincount(bins.ravel()[bins.ravel() >= 0], minlength=n_bins)
        left_out = bins < 0
        if dtype == "u64fx":
            ref = column_sums_numpy(g, bins, n_bins, np.uint64)
            raw = ctx.tally_sum_columns(bins, n_bins, raw=True)
            assert raw.dtype == np.uint64 and raw.shape == ref.shape and np.array_equal(raw, ref), what
            assert np.array_equal(ctx.tally_sum_columns(bins, n_bins), ref.astype(np.float64) * 2.0 ** -40), what
            # left-out columns are counted nowhere; with none left out (the radial tables) nothing is lost
            assert raw.sum(dtype=np.uint64) == total - g[:, left_out].sum(dtype=np.uint64), what
            assert not raw[:, count == 0].any()
        else:
            ref = column_sums_numpy(g, bins, n_bins, np.float64)
            got = ctx.tally_sum_columns(bins, n_bins)
            assert_float_sums(got, ref, count[None, :], what)         # an empty bin: bound 0, exactly 0
            assert not got[:, count == 0].any()


def test_column_sums_reject_bad_tables(ctx):
    g = load(ctx, (37, 19, 11), "u64fx")
    nz, ny, nx = g.shape
    bins = np.zeros((ny, nx), dtype=np.int32)
    out = np.empty((nz, 4097))
    call = lambda b, n: _lib.lib().lt_tally_sum_columns(ctx._h, _lib._ip(b), C.c_int(n), _lib._dp(out), None)      # noqa: E731
    assert call(bins, 4096) == 0 and call(bins, 1) == 0
    assert call(bins, 4097) == E_UNSUPPORTED and b"4097" in _lib.lib().lt_last_error(ctx._h)
    assert call(bins, 0) == E_INVALID
    for bad, n_bins in ((5, 5), (-2, 5), (4096, 4096)):
        b = bins.copy()
        b[ny - 1, nx - 1] = bad
        assert call(b, n_bins) == E_INVALID
        with pytest.raises(lt.LtError):
            ctx.tally_sum_columns(b, n_bins)
    with pytest.raises(lt.LtError):
        ctx.tally_sum_columns(bins[:, :-1], 4)


def test_argument_errors(ctx):
    for dtype in ("f64", "f32"):
        g = load(ctx, (37, 19, 11), dtype)
        out, raw = np.empty(g.shape), np.empty(g.shape, dtype=np.uint64)
        rp = raw.ctypes.data_as(C.POINTER(C.c_uint64))
        assert _lib.lib().lt_tally_sum_axes(ctx._h, C.c_int(4), _lib._dp(out), rp) == E_INVALID            # raw_out on a float tally
        bins = np.zeros(g.shape[1:], dtype=np.int32)
        assert _lib.lib().lt_tally_sum_columns(ctx._h, _lib._ip(bins), C.c_int(1), _lib._dp(out), rp) == E_INVALID
        with pytest.raises(lt.LtError):
            ctx.tally_sum("z", raw=True)
    for mask in (7, 8, 15, -1):
        assert _lib.lib().lt_tally_sum_axes(ctx._h, C.c_int(mask), _lib._dp(out), None) == E_INVALID
    assert _lib.lib().lt_tally_sum_axes(ctx._h, C.c_int(4), None, None) == E_INVALID                       # out is required
    with pytest.raises(ValueError):
        ctx.tally_sum("xyz")
    # write_grid: size, dtype and shape are checked
    assert _lib.lib().lt_write_grid(ctx._h, g.ctypes.data_as(C.c_void_p), C.c_size_t(g.nbytes - 4)) == E_INVALID
    for bad in (g.astype(np.float64), g[:-1], g.reshape(g.shape[::-1])):
        with pytest.raises(lt.LtError):
            ctx.write_grid(bad)


def test_calls_before_set_grid_give_state_error():
    with lt.Context(0) as fresh:
        out, bins = np.empty(8), np.zeros((2, 2), dtype=np.int32)
        L = _lib.lib()
        assert L.lt_tally_sum_axes(fresh._h, C.c_int(4), _lib._dp(out), None) == E_STATE
        assert L.lt_tally_sum_columns(fresh._h, _lib._ip(bins), C.c_int(1), _lib._dp(out), None) == E_STATE
        assert L.lt_write_grid(fresh._h, out.ctypes.data_as(C.c_void_p), C.c_size_t(out.nbytes)) == E_STATE
        for f in (lambda: fresh.tally_sum("z"), lambda: fresh.tally_sum_columns(bins, 1), lambda: fresh.write_grid(out)):
            with pytest.raises(lt.LtError):
                f()


@pytest.mark.parametrize("scene", ["slab", "cornell"])
def test_profiles_of_a_traced_scene_match_the_oracle(ctx, scene):
    prob = S.slab(n=32, voxel=0.8) if scene == "slab" else S.cornell(24)
    prob.apply(ctx, "u64fx")
    ctx.launch(4096, seed=123)
    ctx.sync()
    _, fxo, _ = prob.oracle().run(4096, seed=123, want_fx=True, want_f64=False, threads=4)
    assert np.array_equal(ctx.tally_sum("z", raw=True), fxo.sum(axis=(1, 2), dtype=np.uint64))
    assert np.array_equal(ctx.tally_sum("xy", raw=True), fxo.sum(axis=0, dtype=np.uint64))
    nx, ny, _ = prob.grid_shape
    nr = 9
    bins = _lib.radial_bins((nx, ny), prob.origin[:2], prob.voxel[:2], (0.1, -0.3), 1.1, nr)
    rz = ctx.tally_sum_columns(bins, nr + 1, raw=True)
    total = ctx.tally_sum("", raw=True)
    assert total.shape == () and total > 0 and rz.sum(dtype=np.uint64) == total == fxo.sum(dtype=np.uint64)
    assert np.array_equal(rz, column_sums_numpy(fxo, bins, nr + 1, np.uint64))


def _slab_tracer(ctx, dtype, quantity):
    tr = PT.PhotonTracer(ctx=ctx)
    tr.configure(PT.LayeredSlab([PT.OpticalMedium(0.1, 10.0, 0.9, 1.0)], [np.inf]),
                 PT.VoxelGrid((32, 32, 32), (-12.8, -12.8, 0.0), 0.8, dtype=dtype), PT.PencilBeam((0, 0, 0), (0, 0, 1)), quantity=quantity)
    return tr.run(4096, seed=123)


def test_tracer_depth_profile_and_projections(ctx):
    tr = _slab_tracer(ctx, "u64fx", "absorbed")
    a = tr.absorbed()
    assert a.sum() > 1000
    assert_float_sums(tr.depth_profile(), a.sum((1, 2)), 32 * 32, "depth_profile")
    for axis, name in ((0, "z"), (1, "y"), (2, "x")):
        assert_float_sums(tr.projection(name), a.sum(axis), 32, "projection " + name)
        assert np.array_equal(tr.projection(axis), tr.projection(name))
    m, edges = tr.rz_map((0.0, 0.0), 0.8, 12)
    assert m.shape == (32, 13) and edges.shape == (14,) and edges[0] == 0 and edges[12] == 0.8 * 12 and np.isinf(edges[13])
    assert_float_sums(m.sum(), a.sum(), 32 ** 3, "rz_map total")
    with pytest.raises(ValueError):
        tr.projection("w")


def test_tracer_fluence_rz_map_is_the_ring_mean(ctx):
    """Rings of 0.05 on a grid of 0.8 voxels: most of them hold no column (NaN).  Tolerance: the reference divides every voxel by
    dV x photons (one rounding each, 2^-53 relative) before the mean's sum and division, the map divides the sum once by a
    rounded product -- four more roundings than the bare sums: (n + 4) 2^-52 ref."""
    tr = _slab_tracer(ctx, "f64", "fluence")
    nr, dr = 60, 0.05
    m, _ = tr.rz_map((0.1, -0.3), dr, nr)
    fl = tr.fluence()
    bins = _lib.radial_bins((32, 32), (-12.8, -12.8), (0.8, 0.8), (0.1, -0.3), dr, nr)
    count = np.bincount(bins.ravel(), minlength=nr + 1)
    assert (count == 0).sum() > 3 and (count > 0).sum() > 10
    assert np.array_equal(np.isnan(m), np.broadcast_to(count == 0, m.shape))
    for k in np.flatnonzero(count):
        assert_float_sums(m[:, k], fl[:, bins == k].mean(axis=1), count[k] + 4, "ring %d" % k)
    assert np.nansum(m) > 0
    dp = tr.depth_profile()
    assert_float_sums(dp, fl.mean(axis=(1, 2)), 32 * 32 + 4, "fluence depth profile")
    tr.ctx.set_tally_quantity("absorbed")
