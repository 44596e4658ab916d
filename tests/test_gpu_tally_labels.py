"""GPU suite of the results by region: lt_set_labels, lt_tally_label_sums, lt_tally_histogram and the PhotonTracer methods on
top, against the NumPy restatements of tests/test_tally_labels_cpu.py on grids of known (seeded random) contents, and
label_volume of a mesh against the analytic sphere, end to end.

Bounds.  Voxel counts, filled counts, peaks, peak indices and every u64 fixed-point sum are integers or single values: exact.
The class of a voxel is decided on its exactly converted value (u64: one rounding, as NumPy's astype), so the counts are exact
for float tallies too.  Float weights are sums of n non-negative f64 terms in some order: within n 2^-52 ref of NumPy's, n the
voxels of the bin (assert_float_sums, the bound the tally-sums suite derives)."""
import ctypes as C

import numpy as np
import pytest

import light_transport_amd as lt
from light_transport_amd import _lib
from light_transport_amd.src import photon_tracing as PT
from tests import scenes as S
from tests.test_gpu_tally_sums import DTYPES, SHAPES, assert_float_sums, load
from tests.test_tally_labels_cpu import as_weight, histogram_numpy, label_sums_numpy

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE, E_UNSUPPORTED = -1, -2, -5
NONE = 255
_U8P, _U64P, _I64P = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64), C.POINTER(C.c_int64)


def label_volumes(shape):
    """(name, labels [nz, ny, nx] or None, n_labels) of the volumes a shape is read with; seeded per shape."""
    nx, ny, nz = shape
    rs = np.random.RandomState(500 + SHAPES.index(shape))
    dims = (nz, ny, nx)
    vols = [("no labels", None, 1), ("one label everywhere", np.zeros(dims, dtype=np.uint8), 1)]
    for n in (1, 3, 64):
        lab = rs.randint(0, n, size=dims).astype(np.uint8)
        vols.append(("random %d" % n, lab, n))
        holes = lab.copy()
        holes[rs.random_sample(dims) < 0.2] = NONE
        vols.append(("random %d, a fifth left out" % n, holes, n))
    vols.append(("z slabs", np.ascontiguousarray(np.broadcast_to((np.arange(nz) * 5 // max(nz, 1)).astype(np.uint8)[:, None, None], dims)), 5))
    runs = ((np.arange(nx * ny * nz) // 7) % 11).astype(np.uint8).reshape(dims)           # runs of 7 along x, across rows and groups
    vols.append(("runs of 7", runs, 11))
    vols.append(("everything left out", np.full(dims, NONE, dtype=np.uint8), 3))
    return vols


def edge_sets(g):
    """(name, edges) for a raw grid: one edge 0 (every voxel is class 1), one above every value, 63 edges, and five taken from
    the grid's own values (fewer on a grid with fewer values): a voxel ON an edge belongs to the class above it."""
    w = as_weight(g).ravel()
    top = float(w.max())
    own = np.unique(w)
    own = own[np.linspace(0, own.size - 1, min(5, own.size)).astype(int)]
    return [("edge 0", [0.0]), ("edge above all", [2.0 * top + 1.0]), ("63 edges", list(np.linspace(0.0, top + 1.0, 63))),
            ("own values", list(np.unique(own)))]


def apply_labels(ctx, labels, n_labels):
    ctx.set_labels(labels, n_labels if labels is not None else None)
    assert ctx.labels_info() == (n_labels if labels is not None else 0)


def check_label_sums(ctx, g, labels, n_labels, dtype, what):
    ref = label_sums_numpy(g, labels, n_labels, np.uint64 if dtype == "u64fx" else np.float64)
    got = ctx.tally_label_sums(raw=dtype == "u64fx")
    for key in ("voxels", "filled", "peak_index"):
        assert got[key].dtype == ref[key].dtype and np.array_equal(got[key], ref[key]), "%s: %s" % (what, key)
    assert np.array_equal(got["peak"], as_weight(ref["peak"])), what
    if dtype == "u64fx":
        assert got["raw"].dtype == np.uint64 and np.array_equal(got["raw"], ref["sum"]), what
        assert np.array_equal(got["weight"], ref["sum"].astype(np.float64) * 2.0 ** -40), what
    else:
        assert_float_sums(got["weight"], ref["sum"], ref["voxels"].astype(np.float64), what)
    return got


def check_histogram(ctx, g, labels, n_labels, edges, dtype, what):
    ref_v, ref_w = histogram_numpy(g, labels, n_labels, edges, np.uint64 if dtype == "u64fx" else np.float64)
    if dtype == "u64fx":
        vox, raw = ctx.tally_histogram(edges, raw=True)
        assert raw.dtype == np.uint64 and np.array_equal(raw, ref_w), what
        vox2, w = ctx.tally_histogram(edges)
        assert np.array_equal(w, ref_w.astype(np.float64) * 2.0 ** -40) and np.array_equal(vox2, vox), what
    else:
        vox, w = ctx.tally_histogram(edges)
        assert_float_sums(w, ref_w, ref_v.astype(np.float64), what)
        again, _ = ctx.tally_histogram(edges)
        assert np.array_equal(again, vox), "%s: a second call gave other counts" % what
    assert vox.dtype == np.uint64 and vox.shape == ref_v.shape and np.array_equal(vox, ref_v), what
    return vox


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_label_sums_and_histograms_match_the_restatement(ctx, shape, dtype):
    g = load(ctx, shape, dtype)
    c0 = ctx.read_counters()
    total = ctx.tally_sum("", raw=True) if dtype == "u64fx" else None
    sets = edge_sets(g)
    for name, labels, n_labels in label_volumes(shape):
        what = "%s %s %s" % (shape, dtype, name)
        apply_labels(ctx, labels, n_labels)
        got = check_label_sums(ctx, g, labels, n_labels, dtype, what)
        left_out = 0 if labels is None else int(np.count_nonzero(labels == NONE))
        assert int(got["voxels"].sum()) == g.size - left_out
        if labels is not None and left_out == g.size:
            assert not got["weight"].any() and not got["filled"].any() and not got["peak"].any() and np.all(got["peak_index"] == -1)
        if dtype == "u64fx" and left_out == 0 and n_labels == 1:
            assert got["raw"][0] == total                                        # one label, the whole grid: the grid total
        for ename, edges in sets:
            vox = check_histogram(ctx, g, labels, n_labels, edges, dtype, what + ", " + ename)
            assert int(vox.sum()) == g.size - left_out
            if ename == "edge 0":
                assert not vox[:, 0].any()
            if ename == "edge above all":
                assert not vox[:, 1].any()
    back = ctx.read_grid_raw()
    assert np.array_equal(back.view(np.uint8), g.view(np.uint8)) and ctx.read_counters() == c0      # nothing but the outputs is written
    ctx.set_labels(None)
    assert ctx.labels_info() == 0


def test_peak_index_is_the_lowest_and_the_class_uses_one_rounding(ctx):
    shape = (37, 19, 11)
    nx, ny, nz = shape
    g = load(ctx, shape, "u64fx").copy()
    labels = label_volumes(shape)[4][1]                                            # random, 3 labels
    flat, lab = g.reshape(-1), labels.reshape(-1)
    ones = np.flatnonzero(lab == 1)
    a, b = int(ones[ones.size // 3]), int(ones[2 * ones.size // 3])                # the same maximum twice in label 1, far apart
    flat[a] = flat[b] = np.uint64(2 ** 41)
    ctx.write_grid(g)
    ctx.set_labels(labels, 3)
    got = check_label_sums(ctx, g, labels, 3, "u64fx", "planted maximum")
    assert got["peak_index"][1] == a < b and got["peak"][1] == 2.0
    # values that do not fit a double: 2^53 + 1 rounds down to 2^53 (a tie, to even), 2^53 + 3 up to 2^53 + 4, 2^63 + 2^10 + 1
    # up to 2^63 + 2^11.  With the rounded doubles as edges every planted voxel sits ON an edge -- class = edges <= v -- which a
    # conversion through a truncation or two roundings would put one class lower
    big = [2 ** 53 + 1, 2 ** 53 + 3, 2 ** 63 + 2 ** 10 + 1]
    spots = [0, 1, nx, nx * ny - 1, nx * ny * 5 + 3, flat.size - 3, flat.size - 2, flat.size - 1]      # both ends: the first group and the tail
    for k, s in enumerate(spots):
        flat[s] = np.uint64(big[k % 3])
    edges = sorted(float(np.uint64(v).astype(np.float64)) * 2.0 ** -40 for v in big)
    assert edges == [2.0 ** 13, (2.0 ** 53 + 4) * 2.0 ** -40, (2.0 ** 63 + 2.0 ** 11) * 2.0 ** -40]
    ctx.write_grid(g)
    for labels_, n in ((labels, 3), (None, 1)):
        apply_labels(ctx, labels_, n)
        vox = check_histogram(ctx, g, labels_, n, edges, "u64fx", "values beyond 2^53")
        assert int(vox[:, 1:].sum()) == 8 and int(vox[:, 3].sum()) == 2              # the eight planted; all else is below 2^13
        check_label_sums(ctx, g, labels_, n, "u64fx", "values beyond 2^53")          # the raw sum wraps modulo 2^64, as NumPy's
    ctx.set_labels(None)


def test_error_codes(ctx):
    L = _lib.lib()
    with lt.Context(0) as fresh:
        lab = np.zeros(8, dtype=np.uint8)
        out, u = np.zeros(8), np.zeros(8, dtype=np.uint64)
        i64 = np.zeros(8, dtype=np.int64)
        assert L.lt_set_labels(fresh._h, lab.ctypes.data_as(_U8P), 8, 1) == E_STATE
        assert L.lt_tally_label_sums(fresh._h, _lib._dp(out), None, u.ctypes.data_as(_U64P), u.ctypes.data_as(_U64P), _lib._dp(out),
                                     i64.ctypes.data_as(_I64P)) == E_STATE
        assert L.lt_tally_histogram(fresh._h, _lib._dp(out), 1, u.ctypes.data_as(_U64P), _lib._dp(out), None) == E_STATE
        n = C.c_int(-1)
        assert L.lt_labels_info(fresh._h, C.byref(n)) == 0 and n.value == 0
    g = load(ctx, (37, 19, 11), "f64")
    lab = np.zeros(g.shape, dtype=np.uint8)
    p = lambda a: a.ctypes.data_as(_U8P)      # noqa: E731
    assert L.lt_set_labels(ctx._h, p(lab), lab.size - 1, 1) == E_INVALID
    assert L.lt_set_labels(ctx._h, p(lab), lab.size, 0) == E_INVALID and L.lt_set_labels(ctx._h, p(lab), lab.size, 65) == E_INVALID
    assert L.lt_set_labels(ctx._h, p(lab), lab.size, 64) == 0 and ctx.labels_info() == 64
    bad = lab.copy()
    bad.reshape(-1)[4321] = 3
    bad.reshape(-1)[5000] = 200
    assert L.lt_set_labels(ctx._h, p(bad), bad.size, 3) == E_INVALID
    msg = L.lt_last_error(ctx._h)
    assert b"4321" in msg and b"label 3" in msg
    assert ctx.labels_info() == 64                                                 # a refused volume leaves the one in force
    with pytest.raises(lt.LtError):
        ctx.set_labels(lab.astype(np.int32))
    with pytest.raises(lt.LtError):
        ctx.set_labels(lab[:-1])
    ctx.set_labels(None)
    n_cls = 65
    vox, w, raw = np.zeros(n_cls, dtype=np.uint64), np.zeros(n_cls), np.zeros(n_cls, dtype=np.uint64)
    hist = lambda e, n, r=None: L.lt_tally_histogram(ctx._h, _lib._dp(np.asarray(e, dtype=np.float64)), n, vox.ctypes.data_as(_U64P),      # noqa: E731
                                                     _lib._dp(w), r)
    assert hist([0.1, 0.2], 2) == 0
    for e in ([0.2, 0.1], [0.1, 0.1], [-0.1, 0.2], [0.1, np.nan], [0.1, np.inf]):
        assert hist(e, 2) == E_INVALID
    assert hist([0.1], 0) == E_INVALID
    assert hist(np.arange(64.0), 64) == E_UNSUPPORTED and b"64" in L.lt_last_error(ctx._h)
    assert hist(np.arange(63.0), 63) == 0
    assert hist([0.1], 1, raw.ctypes.data_as(_U64P)) == E_INVALID                  # raw sums of a float tally
    assert L.lt_tally_histogram(ctx._h, None, 1, vox.ctypes.data_as(_U64P), _lib._dp(w), None) == E_INVALID
    i64 = np.zeros(1, dtype=np.int64)
    sums = lambda wp, rp, ip: L.lt_tally_label_sums(ctx._h, wp, rp, vox.ctypes.data_as(_U64P), raw.ctypes.data_as(_U64P), _lib._dp(w), ip)      # noqa: E731
    assert sums(_lib._dp(w), None, i64.ctypes.data_as(_I64P)) == 0
    assert sums(_lib._dp(w), raw.ctypes.data_as(_U64P), i64.ctypes.data_as(_I64P)) == E_INVALID
    assert sums(None, None, i64.ctypes.data_as(_I64P)) == E_INVALID and sums(_lib._dp(w), None, None) == E_INVALID
    with pytest.raises(lt.LtError):
        ctx.tally_label_sums(raw=True)


def test_labels_and_statistics_keep_out_of_each_others_way(ctx):
    shape = (37, 19, 11)
    prob = S.slab(n=16, voxel=0.8)
    prob.apply(ctx, "u64fx")
    ctx.stats_enable(True)
    for b in range(2):
        ctx.launch(1024, seed=5, photon_offset=1024 * b)
        ctx.stats_fold()
    g, m2, c0 = ctx.read_grid_raw(), ctx.stats_m2(), ctx.read_counters()
    labels = (np.arange(g.size) % 3).astype(np.uint8).reshape(g.shape)
    ctx.set_labels(labels, 3)
    check_label_sums(ctx, g, labels, 3, "u64fx", "traced slab")
    check_histogram(ctx, g, labels, 3, [1e-3, 1e-1], "u64fx", "traced slab")
    assert np.array_equal(ctx.read_grid_raw(), g) and ctx.read_counters() == c0
    assert np.array_equal(ctx.stats_m2(), m2) and ctx.stats_batches() == 2
    ctx.zero_tally()                                                               # zero_tally and write_grid leave the labels alone
    assert ctx.labels_info() == 3
    ctx.write_grid(g)
    assert ctx.labels_info() == 3 and np.array_equal(ctx.tally_label_sums(raw=True)["raw"], label_sums_numpy(g, labels, 3, np.uint64)["sum"])
    g2 = load(ctx, shape, "u64fx")                                                 # set_grid drops them: one label again
    assert ctx.labels_info() == 0
    got = ctx.tally_label_sums(raw=True)
    assert got["raw"].shape == (1,) and got["raw"][0] == g2.sum(dtype=np.uint64) and got["voxels"][0] == g2.size


def _mesh_tracer(ctx, prob, dtype="u64fx"):
    """A PhotonTracer on a context a tests.scenes Problem was applied to."""
    prob.apply(ctx, dtype)
    tr = PT.PhotonTracer(ctx=ctx)
    tr.grid = PT.VoxelGrid(prob.grid_shape, prob.origin, prob.voxel, dtype=dtype)
    tr.geometry = PT.MeshVolume([PT.OpticalMedium(*m) for m in prob.media], start_medium=prob.source["start_medium"])
    tr.quantity, tr.photons = "absorbed", 0
    return tr


def _voxel_of(prob, point):
    k = np.floor((np.asarray(point) - np.asarray(prob.origin)) / np.asarray(prob.voxel)).astype(int)
    k = np.clip(k, 0, np.asarray(prob.grid_shape) - 1)
    return int(k[2]), int(k[1]), int(k[0])


def test_mesh_labels_of_the_cornell_cone(ctx):
    prob = S.cornell(24)                                                           # voxels of 0.625: centres at +-0.3125, ...
    tr = _mesh_tracer(ctx, prob)
    lab = tr.set_regions()
    assert lab.shape == (24, 24, 24) and ctx.labels_info() == 3 and set(np.unique(lab)) <= {0, 1, 2}
    # the cone's axis is x, from its base at x = -2.5 (radius 2) to the apex at x = +2.5: half height is x = 0
    assert lab[_voxel_of(prob, (0.3, 0.3, 0.3))] == 1                              # on the axis (0.44 off it, the hexagon's inradius there is 0.76)
    assert lab[_voxel_of(prob, (0.3, 4.0, 0.3))] == 0                              # beside the cone at the same height: the cube's medium
    assert lab[_voxel_of(prob, (0.0, 7.4, 0.0))] == prob.source["start_medium"]    # under the ceiling light
    assert 0 < np.count_nonzero(lab == 1) < 0.02 * lab.size                        # the cone is 21 of the cube's 3375 volume units


def test_mesh_labels_of_a_sphere_and_totals_by_region_end_to_end(ctx):
    prob, _, _ = S.sphere_in_box()
    tr = _mesh_tracer(ctx, prob)
    lab = tr.set_regions()
    n = prob.grid_shape[0]
    radius, centre = 1.5, np.array([0.3, -0.2, 0.1])
    ball = prob.mesh["verts"].reshape(-1, 3, 3)[prob.mesh["med_back"] == 1]
    assert ball.shape[0] == 5120
    sagitta = radius - np.min(np.linalg.norm(ball.mean(axis=1) - centre, axis=1)) + 1e-9
    c = prob.origin[0] + prob.voxel[0] * (np.arange(n) + 0.5)
    dist = np.sqrt((c[None, None, :] - centre[0]) ** 2 + (c[None, :, None] - centre[1]) ** 2 + (c[:, None, None] - centre[2]) ** 2)
    clear = np.abs(dist - radius) > sagitta
    inside = dist < radius
    print("sagitta %.3g of the radius; %d of %d voxels inside the sphere lie within it of the surface" % (
        sagitta / radius, np.count_nonzero(~clear), np.count_nonzero(inside)))
    assert np.count_nonzero(~clear) <= 0.01 * np.count_nonzero(inside)
    assert np.array_equal(lab[clear], np.where(inside, 1, 0)[clear].astype(np.uint8))
    assert lab[_voxel_of(prob, (0.0, 4.0, 0.0))] == prob.source["start_medium"] == 0     # the middle of the ceiling light
    assert not np.any(lab == 2) and ctx.labels_info() == 3                           # every centre lies inside the box
    # 20 000 photons in four batches; label totals after every fold
    ctx.zero_tally()
    tr.run_batches(20000, 4, seed=9, labels=True)
    g = ctx.read_grid_raw()
    ref = label_sums_numpy(g, lab, 3, np.uint64)
    got = ctx.tally_label_sums(raw=True)
    assert got["raw"].sum(dtype=np.uint64) == ctx.tally_sum("", raw=True) == g.sum(dtype=np.uint64) and got["raw"][1] > 0
    for key, rkey in (("raw", "sum"), ("voxels", "voxels"), ("filled", "filled"), ("peak_index", "peak_index")):
        assert np.array_equal(got[key], ref[rkey]), key
    assert np.array_equal(got["peak"], as_weight(ref["peak"]))
    r = tr.region_totals()
    assert np.array_equal(r["weight"], as_weight(ref["sum"])) and np.array_equal(r["share"], as_weight(ref["sum"]) / 20000.0)
    z, y, x = np.unravel_index(ref["peak_index"][1], g.shape)
    assert np.array_equal(r["peak_position"][1], np.asarray(prob.origin) + np.asarray(prob.voxel) * (np.array([x, y, z]) + 0.5))
    dv = tr.dose_volume([0.0, float(r["peak"][1])])
    assert np.all(dv["volume"][:2, 0] == 1.0) and dv["volume"][1, 1] == np.count_nonzero(g.reshape(-1)[lab.reshape(-1) == 1] == ref["peak"][1]) / float(ref["voxels"][1])
    err = tr.region_totals_error()
    # the same four batches, traced apart and read back: the per-batch label sums, then the estimator
    ctx.stats_enable(False)
    ctx.zero_tally()
    last, per_batch = np.zeros_like(g), []
    for b in range(4):
        ctx.launch(5000, seed=9, photon_offset=5000 * b)
        ctx.sync()
        now = ctx.read_grid_raw()
        per_batch.append(as_weight(label_sums_numpy(now - last, lab, 3, np.uint64)["sum"]))
        last = now
    assert np.array_equal(last, g)
    s1, s2 = sum(per_batch), sum(d * d for d in per_batch)
    assert np.array_equal(err, _lib.relative_error(4, s1, s2), equal_nan=True) and np.all(err[:2] > 0)
    ctx.set_labels(None)
