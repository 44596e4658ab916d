"""GPU suite of the batch statistics of the tally (lt_stats_*): the fold, the per-voxel relative error and the class summary
against their NumPy restatements on grids of known contents, against the CPU oracle batch by batch on traced scenes, the
PhotonTracer methods on top, and the error codes.

Bounds.
  m2, N, the voxel counts and every u64 fixed-point sum: the restatement does the same IEEE operations (or integer sums) --
    identical bits, equal integers.
  Relative error.  q = (N m2) / (S1 S1) is three rounded operations, so the device's q and the restatement's are both within
    3 u q of the exact quotient of the same inputs (u = 2^-53), a divide that is faithful rather than correctly rounded costs
    one u more.  R^2 follows from q by three more roundings -- v = q - 1 (|v| <= q), v / (N - 1), the square root (squared
    again by the test) -- each at most u q / (N - 1) in R^2, again with one u of slack for a faithful divide or root.  Two
    results that both obey this differ by less than  |R^2 - R_ref^2| <= 8 u q_ref / (N - 1).
  Float weights per class: non-negative terms widened to f64 and summed in f64 in any order, device and NumPy alike:
    count 2^-52 ref (tests/test_gpu_tally_sums.py)."""
import ctypes as C

import numpy as np
import pytest

import light_transport_amd as lt
from light_transport_amd import _lib
from light_transport_amd.src import photon_tracing as PT
from tests import scenes as S

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (64, 1, 3), (37, 19, 11), (130, 70, 33)]      # (nx, ny, nz): vector tails, odd rows, several workgroups
DTYPES = ["u64fx", "f64", "f32"]
EDGES = [0.05, 0.1, 0.2, 0.3, 0.5, 0.8, 1.0]
TRACED_EDGES = [0.05, 0.1, 0.2, 0.5]
E_INVALID, E_STATE, E_UNSUPPORTED = -1, -2, -5
N_SYN = 5
_U64P = C.POINTER(C.c_uint64)
_oracle = {}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def as_weight(raw):
    """A raw tally in the units of read_grid: what lt_read_grid_f64 does."""
    return raw.astype(np.float64) * 2.0 ** -40 if raw.dtype == np.uint64 else raw.astype(np.float64)


def fold_numpy(m2, grid, prev):
    """The three lines of the fold."""
    d = (grid - prev).astype(np.float64) * 2.0 ** -40 if grid.dtype == np.uint64 else grid.astype(np.float64) - prev.astype(np.float64)
    return m2 + d * d


def increments(shape, dtype, b):
    """Batch b of a shape: values as in test_gpu_tally_sums.random_grid (u64 below 2^40, floats in [0, 1)), a quarter of the
    voxels -- chosen voxel by voxel, so inside 16-byte groups -- get nothing."""
    nx, ny, nz = shape
    rs = np.random.RandomState(5000 + 100 * SHAPES.index(shape) + 10 * DTYPES.index(dtype) + b)
    if dtype == "u64fx":
        inc = rs.randint(0, 2 ** 40, size=(nz, ny, nx), dtype=np.uint64)
    else:
        inc = rs.random_sample((nz, ny, nx)).astype(np.float32 if dtype == "f32" else np.float64)
    inc[rs.random_sample((nz, ny, nx)) < 0.25] = 0
    return inc


def summary_numpy(R, raw_grid, edges):
    """(voxels, weight in the grid's accumulator type) per class from an R grid: np.searchsorted(side="right") = the number
    of edges <= R; NaN (nothing in the voxel) is the last class, whose weight is 0."""
    n_cls = len(edges) + 2
    cls = np.searchsorted(np.asarray(edges, dtype=np.float64), R.ravel(), side="right")
    cls[np.isnan(R.ravel())] = n_cls - 1
    vox = np.bincount(cls, minlength=n_cls).astype(np.uint64)
    w = raw_grid.ravel() if raw_grid.dtype == np.uint64 else raw_grid.ravel().astype(np.float64)
    weight = np.zeros(n_cls, dtype=w.dtype)
    np.add.at(weight, cls, w)
    return vox, weight


def assert_relerr(R, n, s1, m2, what):
    ref = _lib.relative_error(n, s1, m2)
    assert R.shape == ref.shape and R.dtype == np.float64, what
    assert np.array_equal(np.isnan(R), np.isnan(ref)) and np.array_equal(np.isnan(ref), s1 == 0), what
    ok = ~np.isnan(ref)
    q = (np.float64(n) * m2[ok]) / (s1[ok] * s1[ok])
    err, bound = np.abs(R[ok] * R[ok] - ref[ok] * ref[ok]), 8 * 2.0 ** -53 * q / (n - 1)
    print("%s: %d estimates, %d identical to NumPy's, max err / bound = %.3g" % (
        what, int(ok.sum()), int((R[ok] == ref[ok]).sum()), float(np.max(err / bound, initial=0.0))))
    assert np.all(err <= bound), what
    return ref


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_fold_relerr_and_summary_of_written_batches(ctx, shape, dtype):
    what = "%s %s" % (shape, dtype)
    nx, ny, nz = shape
    ctx.set_grid(shape, (0.0, 0.0, 0.0), (0.1, 0.2, 0.3), dtype)
    ctx.stats_enable()
    assert ctx.stats_batches() == 0
    total = np.zeros((nz, ny, nx), dtype=_lib.TALLY_NP[_lib.TALLY[dtype]])
    m2 = np.zeros((nz, ny, nx))
    for b in range(N_SYN):
        new = total + increments(shape, dtype, b)
        assert new.dtype == total.dtype
        ctx.write_grid(new)
        ctx.stats_fold()
        m2, total = fold_numpy(m2, new, total), new
    got_m2 = ctx.stats_m2()
    assert same_bits(got_m2, m2), what
    assert ctx.stats_batches() == N_SYN
    s1 = as_weight(total)
    R = ctx.stats_relerr()
    assert_relerr(R, N_SYN, s1, got_m2, what)
    if nx * ny * nz > 1000:
        assert (R == 1.0).sum() > 3 and (R[~np.isnan(R)] < 0.5).sum() > 100, what      # single-batch voxels sit ON the last edge

    n_cls = len(EDGES) + 2
    vox_ref, w_ref = summary_numpy(R, total, EDGES)
    vox, w = ctx.stats_summary(EDGES)
    assert vox.dtype == np.uint64 and vox.shape == (n_cls,) and w.dtype == np.float64 and w.shape == (n_cls,), what
    assert np.array_equal(vox, vox_ref), what
    assert int(vox.sum()) == nx * ny * nz and int(vox[-1]) == int((s1 == 0).sum()) and w[-1] == 0, what
    if dtype == "u64fx":
        vox2, raw = ctx.stats_summary(EDGES, raw=True)
        assert np.array_equal(vox2, vox_ref) and raw.dtype == np.uint64 and np.array_equal(raw, w_ref), what
        assert np.array_equal(w, w_ref.astype(np.float64) * 2.0 ** -40), what
    else:
        err, bound = np.abs(w - w_ref), vox_ref.astype(np.float64) * 2.0 ** -52 * w_ref
        print("%s: class weights max err / bound = %.3g" % (what, float(np.max(err / np.where(bound > 0, bound, 1.0), initial=0.0))))
        assert np.all(err <= bound), what
    # one edge: the smallest summary
    vox1, _ = ctx.stats_summary([0.3])
    assert np.array_equal(vox1, summary_numpy(R, total, [0.3])[0]), what

    ctx.stats_fold()                         # nothing written since: a batch of zeros
    assert ctx.stats_batches() == N_SYN + 1 and same_bits(ctx.stats_m2(), m2), what
    ctx.zero_tally()
    assert ctx.stats_batches() == 0 and not ctx.stats_m2().any() and not ctx.read_grid_raw().any(), what
    ctx.write_grid(total)                    # prev was zeroed too: the whole grid is the first batch again
    ctx.stats_fold()
    assert same_bits(ctx.stats_m2(), fold_numpy(np.zeros_like(m2), total, np.zeros_like(total))), what
    ctx.stats_enable(False)


def test_summary_takes_63_edges(ctx):
    shape, dtype = (37, 19, 11), "u64fx"
    ctx.set_grid(shape, (0.0, 0.0, 0.0), (0.1, 0.2, 0.3), dtype)
    ctx.stats_enable()
    total = np.zeros(shape[::-1], dtype=np.uint64)
    for b in range(N_SYN):
        total = total + increments(shape, dtype, b)
        ctx.write_grid(total)
        ctx.stats_fold()
    R = ctx.stats_relerr()
    edges = np.linspace(0.0, 1.0, 63)        # the first edge 0: every estimate is in class >= 1; the last 1: single-batch voxels
    vox, raw = ctx.stats_summary(edges, raw=True)
    vox_ref, w_ref = summary_numpy(R, total, edges)
    assert vox.shape == (65,) and np.array_equal(vox, vox_ref) and np.array_equal(raw, w_ref)
    assert vox[0] == 0 and vox[63] == (R >= 1.0).sum() > 0 and (vox[1:63] > 0).sum() > 20


def oracle_batches(scene):
    """The CPU oracle on the scene, batch by batch (8 x 512 photons, seed 123) and in one run of all 4096, computed once:
    dict(prob, batches [8] u64 grids, whole u64 grid)."""
    if scene not in _oracle:
        prob = S.slab(n=32, voxel=0.8) if scene == "slab" else S.cornell(24)
        orc = prob.oracle()
        batches = [orc.run(512, seed=123, photon_offset=512 * b, want_fx=True, want_f64=False, threads=4)[1] for b in range(8)]
        whole = orc.run(4096, seed=123, want_fx=True, want_f64=False, threads=4)[1]
        for g in batches + [whole]:
            g.setflags(write=False)
        _oracle[scene] = dict(prob=prob, batches=batches, whole=whole)
    return _oracle[scene]


@pytest.mark.parametrize("scene", ["slab", "cornell"])
def test_traced_batches_match_the_oracle_bit_for_bit(ctx, scene):
    o = oracle_batches(scene)
    o["prob"].apply(ctx, "u64fx")
    ctx.stats_enable()
    total, m2 = np.zeros_like(o["whole"]), np.zeros(o["whole"].shape)
    for b in range(8):
        ctx.launch(512, seed=123, photon_offset=512 * b)
        ctx.stats_fold()
        new = total + o["batches"][b]
        m2, total = fold_numpy(m2, new, total), new
    assert np.array_equal(total, o["whole"])             # the oracle itself does not depend on the split
    assert np.array_equal(ctx.read_grid_raw(), total)
    assert ctx.stats_batches() == 8
    assert same_bits(ctx.stats_m2(), m2)
    R_ref = _lib.relative_error(8, as_weight(total), m2)
    vox_ref, w_ref = summary_numpy(R_ref, total, TRACED_EDGES)
    vox, raw = ctx.stats_summary(TRACED_EDGES, raw=True)
    print("%s: voxels per class %s, R == 1 in %d voxels" % (scene, vox.tolist(), int((R_ref == 1.0).sum())))
    assert np.array_equal(vox, vox_ref) and np.array_equal(raw, w_ref)
    assert np.all(vox[:5] >= 10)                         # every class is populated: nothing above passed vacuously
    assert int(raw.sum()) == int(total.sum(dtype=np.uint64))
    assert_relerr(ctx.stats_relerr(), 8, as_weight(total), m2, scene)
    ctx.stats_enable(False)


def slab_tracer(ctx, dtype):
    """S.slab(n=32, voxel=0.8) through the object API."""
    tr = PT.PhotonTracer(ctx=ctx)
    return tr.configure(PT.LayeredSlab([PT.OpticalMedium(0.1, 10.0, 0.9, 1.0)], [np.inf]),
                        PT.VoxelGrid((32, 32, 32), (-12.8, -12.8, 0.0), 0.8, dtype=dtype), PT.PencilBeam((0, 0, 0), (0, 0, 1)))


def test_tracer_run_batches_leaves_the_grid_of_one_run(ctx):
    o = oracle_batches("slab")
    tr = slab_tracer(ctx, "u64fx")
    one_run = tr.run(4096, seed=123).absorbed_raw()
    tr.reset()
    assert tr.run_batches(4096, 8, seed=123, profiles=("z",)) is tr
    assert tr.photons == 4096 and ctx.stats_batches() == 8
    assert np.array_equal(tr.absorbed_raw(), one_run) and np.array_equal(one_run, o["whole"])
    R = tr.relative_error()
    assert R.shape == (32, 32, 32) and same_bits(R, ctx.stats_relerr())
    vox, w = tr.error_summary(TRACED_EDGES)
    assert int(vox.sum()) == 32 ** 3 and np.array_equal(vox, summary_numpy(R, one_run, TRACED_EDGES)[0])
    assert w[:5].sum() == pytest.approx(tr.absorbed().sum(), rel=1e-12)
    # the depth profile's error bars, from the oracle's per-batch depth profiles
    s1, s2 = np.zeros(32), np.zeros(32)
    for g in o["batches"]:
        d = g.sum(axis=(1, 2), dtype=np.uint64).astype(np.float64) * 2.0 ** -40
        s1, s2 = s1 + d, s2 + d * d
    pe = tr.profile_error("z")
    assert pe.shape == tr.depth_profile().shape and same_bits(pe, _lib.relative_error(8, s1, s2))
    assert np.nanmax(pe) < 1.0 and np.nanmin(pe) > 0.0
    with pytest.raises(ValueError):
        tr.profile_error("xy")                           # no moments were kept for it
    tr.reset()
    assert ctx.stats_batches() == 0
    ctx.stats_enable(False)


@pytest.mark.parametrize("dtype,f32_walk", [("f64", False), ("f32", True)])
def test_tracer_run_batches_float_moments_follow_the_grid(ctx, monkeypatch, dtype, f32_walk):
    tr = slab_tracer(ctx, dtype)
    snaps, fold = [], ctx.stats_fold

    def fold_and_look():
        fold()
        snaps.append(ctx.read_grid_raw())
    monkeypatch.setattr(ctx, "stats_fold", fold_and_look)
    tr.run_batches(2048, 4, seed=7, f32_walk=f32_walk)
    assert len(snaps) == 4 and ctx.stats_batches() == 4 and snaps[-1].sum() > 500
    m2, prev = np.zeros(snaps[0].shape), np.zeros_like(snaps[0])
    for g in snaps:
        m2, prev = fold_numpy(m2, g, prev), g
    assert same_bits(ctx.stats_m2(), m2)
    assert_relerr(tr.relative_error(), 4, as_weight(prev), m2, "%s f32_walk=%s" % (dtype, f32_walk))
    ctx.stats_enable(False)


def test_error_codes(ctx):
    L = _lib.lib()
    S.slab(n=32, voxel=0.8).apply(ctx, "u64fx")
    n = 32 ** 3
    out, vox, raw = np.empty(n), np.empty(66, dtype=np.uint64), np.empty(66, dtype=np.uint64)
    w, nb = np.empty(66), C.c_uint64()
    vp, rp = vox.ctypes.data_as(_U64P), raw.ctypes.data_as(_U64P)
    edges = np.array(TRACED_EDGES)

    def every_call():
        return [L.lt_stats_fold(ctx._h), L.lt_stats_batches(ctx._h, C.byref(nb)), L.lt_stats_read_m2(ctx._h, _lib._dp(out), n),
                L.lt_stats_read_relerr(ctx._h, _lib._dp(out), n), L.lt_stats_summary(ctx._h, _lib._dp(edges), 4, vp, _lib._dp(w), rp)]
    assert every_call() == [E_STATE] * 5                                      # statistics are off
    assert b"lt_stats_enable" in L.lt_last_error(ctx._h)
    with pytest.raises(lt.LtError):
        ctx.stats_m2()
    assert L.lt_stats_enable(ctx._h, 0) == 0                                  # turning off what is off is no error

    ctx.launch(64, seed=1)
    assert L.lt_stats_enable(ctx._h, 1) == E_STATE                            # launched into since set_grid
    ctx.zero_tally()
    ctx.write_grid(np.ones((32, 32, 32), dtype=np.uint64))
    assert L.lt_stats_enable(ctx._h, 1) == E_STATE                            # written to since zero_tally
    ctx.zero_tally()
    assert L.lt_stats_enable(ctx._h, 1) == 0

    assert every_call() == [0, 0, 0, E_STATE, E_STATE] and nb.value == 1      # N = 1: no estimate yet
    ctx.launch(64, seed=1)
    assert every_call() == [0, 0, 0, 0, 0] and nb.value == 2
    assert L.lt_stats_read_m2(ctx._h, None, n) == E_INVALID and L.lt_stats_read_m2(ctx._h, _lib._dp(out), n - 1) == E_INVALID
    assert L.lt_stats_read_relerr(ctx._h, None, n) == E_INVALID and L.lt_stats_read_relerr(ctx._h, _lib._dp(out), n + 1) == E_INVALID
    assert L.lt_stats_batches(ctx._h, None) == E_INVALID

    def summary(e, n_edges=None, raw_p=None, vox_p=vp, w_p=_lib._dp(w)):
        e = np.asarray(e, dtype=np.float64)
        return L.lt_stats_summary(ctx._h, _lib._dp(e), len(e) if n_edges is None else n_edges, vox_p, w_p, raw_p)
    assert summary([0.1, 0.2]) == 0 and summary([0.0]) == 0 and summary(np.linspace(0, 1, 63)) == 0
    for bad in ([0.2, 0.1], [0.1, 0.1], [0.1, np.nan], [np.nan], [-0.1, 0.2], [0.1, np.inf]):
        assert summary(bad) == E_INVALID, bad
    assert summary([0.1], n_edges=0) == E_INVALID and summary([0.1], n_edges=-1) == E_INVALID
    assert summary(np.linspace(0, 1, 64)) == E_UNSUPPORTED and b"64" in L.lt_last_error(ctx._h)
    assert L.lt_stats_summary(ctx._h, None, 2, vp, _lib._dp(w), None) == E_INVALID
    assert summary([0.1], vox_p=None) == E_INVALID and summary([0.1], w_p=None) == E_INVALID
    with pytest.raises(lt.LtError):
        ctx.stats_summary([0.3, 0.2])

    S.slab(n=32, voxel=0.8).apply(ctx, "f64")                                 # set_grid: statistics are off again
    assert every_call() == [E_STATE] * 5
    ctx.stats_enable()
    ctx.stats_fold(); ctx.stats_fold()
    assert summary([0.1]) == 0 and summary([0.1], raw_p=rp) == E_INVALID      # raw weights need the fixed-point tally
    with pytest.raises(lt.LtError):
        ctx.stats_summary([0.1], raw=True)
    vox0, w0 = ctx.stats_summary([0.1])
    assert vox0.tolist() == [0, 0, n] and not w0.any()                        # nothing traced: every voxel has no estimate
    assert np.isnan(ctx.stats_relerr()).all()
    ctx.stats_enable(False)
    assert every_call() == [E_STATE] * 5


def test_calls_on_a_fresh_context_give_state_error():
    with lt.Context(0) as fresh:
        assert _lib.lib().lt_stats_enable(fresh._h, 1) == E_STATE             # no grid
        for f in (fresh.stats_fold, fresh.stats_batches, fresh.stats_enable):
            with pytest.raises(lt.LtError):
                f()
