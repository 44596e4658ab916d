"""GPU suite of lt_tally_box and the PhotonTracer methods on top (region, slice, coarse, run_batches(regions=)): boxes, slices
and coarser voxels of seeded random grids against the NumPy restatement (tests.test_tally_box_cpu.box_sums_numpy), and of a
traced slab end to end.  Grids: the shapes and contents of the tally-sums suite.

Bounds.  The u64 fixed-point sums are integers: exact.  Float tallies are widened to f64 and summed in f64; every term is
non-negative, so any summation order of n terms is within (n - 1) 2^-53 of the true sum, relative -- the device's and NumPy's
alike -- and the two differ by at most n 2^-52 ref, n the voxels of the block (the bound of the tally-sums suite).  No voxel is
excepted.

The two kernels (lt_tallybox.hip): a block of min(bin, size) = (bx, by, bz) voxels goes to the workgroup-per-output kernel when
bx by bz >= 512 or bx > 16, to the lanes-along-x kernel otherwise; the (130, 70, 33) grid has a case on either side of both."""
import ctypes as C

import numpy as np
import pytest

import light_transport_amd as lt
from light_transport_amd import _lib
from light_transport_amd.src import photon_tracing as PT
from tests import scenes as S
from tests.test_gpu_tally_sums import DTYPES, SHAPES, assert_float_sums, load
from tests.test_tally_box_cpu import block_voxels, box_sums_numpy

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -2


def is_large(size, bin):
    b = [min(bin[a], size[a]) for a in range(3)]
    return b[0] * b[1] * b[2] >= 512 or b[0] > 16


def boxes_of(shape):
    """(lo, size, bin), x, y, z order: the calls a grid of ``shape`` is read with."""
    nx, ny, nz = shape
    zero = (0, 0, 0)
    cases = [(zero, shape, b) for b in ((1, 1, 1), (2, 2, 2), (3, 5, 7), (4, 1, 1), (1, 4, 1), (1, 1, 4))]
    cases.append((zero, shape, shape))                                       # one output: the grid total
    cases.append((zero, shape, (nx + 3, ny + 1, nz + 5)))                     # a bin larger than the box on every axis
    lo = (nx // 3, ny // 3, nz // 3)
    size = tuple(max(1, (n - l) // 2) for n, l in zip(shape, lo))
    cases.append((lo, size, tuple(s + 1 for s in size)))                      # ... of a box inside the grid
    ly = min(1, ny - 1)
    for lx in (1, 2, 3):                                                      # boxes that start off every 16-byte boundary, odd width
        sx = (nx - lx) - (1 - (nx - lx) % 2)
        if sx >= 1:
            for b in ((1, 1, 1), (2, 1, 1), (3, 2, 2), (32, 4, 4)):
                cases.append(((lx, ly, 0), (sx, ny - ly, nz), b))
    cases.append(((nx - 1, ny - 1, nz - 1), (1, 1, 1), (1, 1, 1)))            # the last voxel of the grid
    for a in range(3):                                                        # full slices: first, a middle and the last index
        for index in sorted({0, shape[a] // 2, shape[a] - 1}):
            lo, size = [0, 0, 0], list(shape)
            lo[a], size[a] = index, 1
            cases.append((tuple(lo), tuple(size), (1, 1, 1)))
    if shape == (16, 16, 600):
        cases += [(zero, shape, (16, 16, 600)), (zero, shape, (1, 1, 600))]   # large blocks: one output, and 256 of them
    if shape == (130, 70, 33):
        cases.append((zero, shape, (2, 2, 1)))                                # small blocks across many workgroups
        cases += [(zero, shape, b) for b in ((8, 8, 7), (8, 8, 8), (16, 4, 7), (16, 4, 8), (16, 1, 1), (17, 1, 1))]
    return cases


def test_the_cases_reach_both_kernels_on_either_side_of_the_rule():
    big = boxes_of((130, 70, 33))
    regime = {b: is_large(s, b) for _, s, b in big}
    assert not regime[(8, 8, 7)] and regime[(8, 8, 8)] and not regime[(16, 4, 7)] and regime[(16, 4, 8)]
    assert not regime[(16, 1, 1)] and regime[(17, 1, 1)] and not regime[(2, 2, 1)]
    assert all(is_large(s, b) for _, s, b in boxes_of((16, 16, 600))[-2:])
    for shape in SHAPES:
        nx, ny, nz = shape
        for lo, size, _ in boxes_of(shape):
            assert all(l >= 0 and s >= 1 for l, s in zip(lo, size)) and all(l + s <= n for l, s, n in zip(lo, size, shape))


@pytest.mark.parametrize("shape", SHAPES)
def test_boxes_u64fx_exact(ctx, shape):
    g = load(ctx, shape, "u64fx")
    for lo, size, bin in boxes_of(shape):
        what = "%s lo %s size %s bin %s" % (shape, lo, size, bin)
        ref = box_sums_numpy(g, lo, size, bin, np.uint64)
        raw = ctx.tally_box(lo, size, bin, raw=True)
        assert raw.dtype == np.uint64 and raw.shape == ref.shape == _lib.box_shape(size, bin), what
        assert np.array_equal(raw, ref), what
        out = ctx.tally_box(lo, size, bin)
        assert out.dtype == np.float64 and np.array_equal(out, ref.astype(np.float64) * 2.0 ** -40), what
    assert ctx.tally_box((0, 0, 0), shape, shape, raw=True)[0, 0, 0] == ctx.tally_sum("", raw=True)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("shape", SHAPES)
def test_boxes_float_within_bound_and_repeatable(ctx, shape, dtype):
    g = load(ctx, shape, dtype)
    for lo, size, bin in boxes_of(shape):
        what = "%s %s lo %s size %s bin %s" % (shape, dtype, lo, size, bin)
        got = ctx.tally_box(lo, size, bin)
        assert_float_sums(got, box_sums_numpy(g, lo, size, bin, np.float64), block_voxels(size, bin), what)
        again = ctx.tally_box(lo, size, bin)
        assert np.array_equal(got.view(np.uint64), again.view(np.uint64)), what + ": a second call gave other bits"
        if bin == (1, 1, 1):       # the voxels themselves, converted exactly
            sub = g[lo[2]:lo[2] + size[2], lo[1]:lo[1] + size[1], lo[0]:lo[0] + size[0]].astype(np.float64)
            assert np.array_equal(got.view(np.uint64), sub.view(np.uint64)), what


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_the_whole_grid_at_bin_one_is_read_grid(ctx, shape, dtype):
    load(ctx, shape, dtype)
    got, ref = ctx.tally_box((0, 0, 0), shape), ctx.read_grid()
    assert got.shape == ref.shape and np.array_equal(got.view(np.uint64), ref.view(np.uint64))


def test_a_call_leaves_grid_counters_and_statistics_as_they_are(ctx):
    prob = S.slab(n=32, voxel=0.8)
    prob.apply(ctx, "u64fx")
    try:
        ctx.stats_enable(True)
        for b in range(2):
            ctx.launch(2000, seed=5, photon_offset=2000 * b)
            ctx.stats_fold()
        ctx.sync()
        before = (ctx.read_grid_raw(), ctx.read_counters(), ctx.stats_m2(), ctx.stats_batches())
        assert before[0].any() and before[2].any() and before[3] == 2
        for lo, size, bin in (((0, 0, 0), (32, 32, 32), (2, 2, 2)), ((0, 0, 0), (32, 32, 32), (8, 8, 8)), ((3, 16, 0), (29, 1, 32), (1, 1, 1))):
            ctx.tally_box(lo, size, bin)
            ctx.tally_box(lo, size, bin, raw=True)
        after = (ctx.read_grid_raw(), ctx.read_counters(), ctx.stats_m2(), ctx.stats_batches())
        assert np.array_equal(before[0], after[0]) and before[1] == after[1]
        assert np.array_equal(before[2].view(np.uint64), after[2].view(np.uint64)) and after[3] == 2
    finally:
        ctx.stats_enable(False)


def _call(ctx, lo, size, bin, out, raw=None):
    arr = [None if v is None else (C.c_int32 * 3)(*v) for v in (lo, size, bin)]
    rp = None if raw is None else raw.ctypes.data_as(C.POINTER(C.c_uint64))
    return _lib.lib().lt_tally_box(ctx._h, arr[0], arr[1], arr[2], None if out is None else _lib._dp(out), rp)


def test_argument_errors(ctx):
    g = load(ctx, (37, 19, 11), "u64fx")
    out, raw = np.empty(g.shape), np.empty(g.shape, dtype=np.uint64)
    lo, size, bin = (0, 0, 0), (37, 19, 11), (1, 1, 1)
    err = lambda: _lib.lib().lt_last_error(ctx._h).decode()      # noqa: E731
    assert _call(ctx, lo, size, bin, out, raw) == 0
    assert _call(ctx, None, size, bin, out) == E_INVALID
    assert _call(ctx, lo, None, bin, out) == E_INVALID
    assert _call(ctx, lo, size, None, out) == E_INVALID
    assert _call(ctx, lo, size, bin, None) == E_INVALID
    assert _call(ctx, (0, -1, 0), (37, 19, 11), bin, out) == E_INVALID and "along y" in err() and "-1" in err()
    assert _call(ctx, lo, (37, 19, 0), bin, out) == E_INVALID and "along z" in err() and "size" in err()
    assert _call(ctx, lo, size, (0, 1, 1), out) == E_INVALID and "along x" in err() and "bin" in err()
    assert _call(ctx, (1, 0, 0), size, bin, out) == E_INVALID and "along x" in err() and "37" in err()        # leaves the grid: 1 .. 37
    assert _call(ctx, (0, 19, 0), (37, 1, 11), bin, out) == E_INVALID and "along y" in err() and "19" in err()
    assert _call(ctx, (0, 0, 5), (37, 19, 7), bin, out) == E_INVALID and "along z" in err() and "11" in err()
    assert _call(ctx, (0, 0, 0), (2 ** 31 - 1, 1, 1), bin, out) == E_INVALID
    with pytest.raises(lt.LtError):
        ctx.tally_box((0, 0, 10), (1, 1, 2))
    with pytest.raises(ValueError):
        ctx.tally_box((0, 0), (1, 1, 1))
    for dtype in ("f64", "f32"):
        load(ctx, (37, 19, 11), dtype)
        assert _call(ctx, lo, size, bin, out) == 0
        assert _call(ctx, lo, size, bin, out, raw) == E_INVALID                  # raw_out on a float tally
        with pytest.raises(lt.LtError):
            ctx.tally_box(lo, size, raw=True)


def test_a_call_before_set_grid_gives_a_state_error():
    with lt.Context(0) as fresh:
        assert _call(fresh, (0, 0, 0), (1, 1, 1), (1, 1, 1), np.empty(1)) == E_STATE
        with pytest.raises(lt.LtError):
            fresh.tally_box((0, 0, 0), (1, 1, 1))


def _slab_tracer(ctx, quantity):
    prob = S.slab(n=32)
    tr = PT.PhotonTracer(ctx=ctx)
    tr.configure(PT.LayeredSlab([PT.OpticalMedium(*prob.media[0])], [np.inf]),
                 PT.VoxelGrid(prob.grid_shape, prob.origin, prob.voxel, dtype="u64fx"), PT.PencilBeam((0, 0, 0), (0, 0, 1)), quantity=quantity)
    return tr


def test_tracer_coarse_and_slice_of_a_traced_slab(ctx):
    tr = _slab_tracer(ctx, "absorbed").run(20000, seed=123)
    raw = tr.absorbed_raw()
    assert raw.any()
    blocks = raw.reshape(8, 4, 8, 4, 8, 4).sum(axis=(1, 3, 5), dtype=np.uint64)
    assert np.array_equal(tr.ctx.tally_box((0, 0, 0), (32, 32, 32), (4, 4, 4), raw=True), blocks)
    assert np.array_equal(tr.coarse(4), blocks.astype(np.float64) * 2.0 ** -40)
    a = tr.absorbed()
    assert np.array_equal(tr.slice("y", 16), a[:, 16, :]) and a[:, 16, :].any()
    assert np.array_equal(tr.slice("x", 31), a[:, :, 31]) and np.array_equal(tr.slice(0, 0), a[0])
    got, (ze, ye, xe) = tr.region((8, 8, 0), (16, 16, 12), (4, 4, 5))
    assert got.shape == (3, 4, 4) and np.array_equal(got, box_sums_numpy(raw, (8, 8, 0), (16, 16, 12), (4, 4, 5), np.uint64) * 2.0 ** -40)
    vz, oz = tr.grid.voxel[2], tr.grid.origin[2]
    assert np.array_equal(ze, oz + vz * np.array([0, 5, 10, 12])) and xe.shape == (5,) and xe[0] == tr.grid.origin[0] + tr.grid.voxel[0] * 8


def test_tracer_fluence_coarse_is_the_mean_over_the_clipped_blocks(ctx):
    """1e-14 relative: one division and the 2^-40 scaling on the device's side, the host's roundings of a 27-term mean on the
    other."""
    tr = _slab_tracer(ctx, "fluence").run(20000, seed=123)
    try:
        fl = tr.fluence()
        ref = box_sums_numpy(fl, (0, 0, 0), (32, 32, 32), (3, 3, 3), np.float64) / block_voxels((32, 32, 32), (3, 3, 3))
        got = tr.coarse((3, 3, 3))
        assert got.shape == ref.shape == (11, 11, 11) and ref.max() > 0
        err = np.abs(got - ref)
        print("fluence coarse((3, 3, 3)): max relative difference %.3g" % float(np.max(err[ref > 0] / ref[ref > 0])))
        assert np.all(err <= 1e-14 * ref)
    finally:
        tr.ctx.set_tally_quantity("absorbed")


def test_region_error_of_run_batches_is_the_host_computation(ctx):
    box = ((0, 0, 0), (32, 32, 32), (4, 4, 4))
    tr = _slab_tracer(ctx, "absorbed")
    try:
        tr.run_batches(20000, 4, seed=9, regions=(box,))
        got = tr.region_error(*box)
        total = tr.absorbed_raw()
    finally:
        ctx.stats_enable(False)
    tr = _slab_tracer(ctx, "absorbed")                    # the same four batches by hand: a coarse read (raw) after each
    s1, s2, last = 0.0, 0.0, np.zeros((8, 8, 8), dtype=np.uint64)
    for b in range(4):
        tr.run(5000, seed=9, photon_offset=5000 * b)
        now = tr.ctx.tally_box(*box, raw=True)
        d = (now - last).astype(np.float64) * 2.0 ** -40
        s1, s2, last = s1 + d, s2 + d * d, now
    assert np.array_equal(tr.absorbed_raw(), total)
    assert np.array_equal(tr.coarse(4), last.astype(np.float64) * 2.0 ** -40)
    ref = _lib.relative_error(4, s1, s2)
    assert got.shape == (8, 8, 8) and np.array_equal(got, ref, equal_nan=True)
    seen = ~np.isnan(ref)
    assert seen.sum() > 100 and np.all(ref[seen] >= 0) and ref[seen].max() > 0
