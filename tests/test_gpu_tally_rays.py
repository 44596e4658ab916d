"""GPU suite of the tally along rays: lt_tally_rays, lt_tally_view and the PhotonTracer methods on top, against the brute-force
NumPy reference of tests/test_tally_rays_cpu.py (every ray intersected with every voxel's box, no traversal) on seeded grids and
seeded ray families, and against anchors that need no reference.

Bounds.  With t_far the largest plane parameter of a ray, S the sum of the voxels the reference ray meets and ref the reference's
integral:  |got - ref| <= 2^-46 (t_far |d| S + ref), for EVERY ray.  Each chord end is a directly computed quotient, good to a
few units of 2^-53 t_far; all terms are non-negative, so summing n of them adds n 2^-53 ref; 2^-46 leaves a factor of about 100
over that.  Maximum, its index and the first crossing's index are compared exactly, first_t within 2^-46 t_far, for every ray that
is not grazing (the CPU suite's docstring; at most 1 % of a family may be, and those are held to the integral bound alone)."""
import ctypes as C

import numpy as np
import pytest

import light_transport_amd as lt
from light_transport_amd import _lib
from light_transport_amd.src import photon_tracing as PT
from light_transport_amd.src.scene import Scene
from tests import scenes as S
from tests.test_gpu_tally_sums import DTYPES, load
from tests.test_tally_rays_cpu import (FAMILIES, as_weight, family_reference, grid_geometry, ray_results_numpy, ray_voxels_numpy)

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -2
_I64P = C.POINTER(C.c_int64)
BOUND = 2.0 ** -46


def thresholds_of(g):
    """0 (the entry into the grid), a median value, and one above the maximum -- as weight."""
    w = as_weight(g)
    return [0.0, float(np.median(w[w > 0])) if np.any(w > 0) else 0.5, float(w.max()) * 2.0 + 1.0]


def check_rays(got, ref, vox, what, exact_parameters=False):
    """got (a dict from Context.tally_rays with everything asked for) against the reference's results for the same rays.
    exact_parameters: every plane parameter of these rays is exact in f64, so which voxels have a chord > 0 does not hang on
    rounding -- no ray is set aside as grazing (rays that run IN a face plane touch the layer next door by definition)."""
    n = len(vox)
    t_far, length = np.array([v["t_far"] for v in vox]), np.array([v["length"] for v in vox])
    grazing = np.array([v["grazing"] and not exact_parameters for v in vox])
    err, bound = np.abs(got["integral"] - ref["integral"]), BOUND * (t_far * length * ref["met_sum"] + ref["integral"])
    print("%s: %d rays, %d grazing, worst |integral - ref| / bound = %.3g" % (what, n, grazing.sum(), float(np.max(err / np.where(bound > 0, bound, 1.0), initial=0.0))))
    assert np.all(err <= bound), what
    assert grazing.sum() <= 0.01 * n, what
    ok = ~grazing
    assert np.array_equal(got["max"][ok], ref["max"][ok]) and np.array_equal(got["max_index"][ok], ref["max_index"][ok]), what
    assert np.array_equal(got["first_index"][ok], ref["first_index"][ok]), what
    hit = ok & (ref["first_index"] >= 0)
    assert np.all(np.isinf(got["first_t"][ok & ~hit])) and np.all(got["first_t"][ok & ~hit] > 0), what
    terr = np.abs(got["first_t"][hit] - ref["first_t"][hit])
    print("%s: worst |first_t - ref| / (2^-46 t_far) = %.3g" % (what, float(np.max(terr / (BOUND * t_far[hit]), initial=0.0))))
    assert np.all(terr <= BOUND * t_far[hit]), what


def same_bits(a, b):
    return all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a) and set(a) == set(b)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,n", FAMILIES)
def test_rays_against_the_reference(ctx, shape, n, dtype):
    g = load(ctx, shape, dtype)
    o, d, tr, vox = family_reference(shape, n)
    for thr in thresholds_of(g):
        got = ctx.tally_rays(o, d, tr, threshold=thr)
        assert set(got) == {"integral", "max", "max_index", "first_t", "first_index"} and all(a.shape == (n,) for a in got.values())
        check_rays(got, ray_results_numpy(g, vox, thr), vox, "%s %s threshold %.3g" % (shape, dtype, thr))
    # a second call returns identical bits; the forms that compute part of the outputs walk the same voxels in the same order
    thr = thresholds_of(g)[1]
    got = ctx.tally_rays(o, d, tr, threshold=thr)
    assert same_bits(ctx.tally_rays(o, d, tr, threshold=thr), got)
    groups = dict(integral=("integral",), max=("max", "max_index"), first=("first_t", "first_index"))
    for want in ("integral", "max", "first", ("max", "first"), ("integral", "first")):
        keys = [k for w in ((want,) if isinstance(want, str) else want) for k in groups[w]]
        assert same_bits(ctx.tally_rays(o, d, tr, threshold=thr, want=want), {k: got[k] for k in keys}), want


def box_chord(shape, o, d, tr):
    """The geometric length of each ray inside the grid's box: the slab test on that one box."""
    origin, voxel = (np.asarray(v) for v in grid_geometry(shape))
    hi = origin + np.asarray(shape) * voxel
    with np.errstate(divide="ignore", invalid="ignore"):
        a, b = (origin - o) / d, (hi - o) / d
    t0 = np.maximum(np.max(np.minimum(a, b), axis=1), tr[:, 0])
    t1 = np.minimum(np.min(np.maximum(a, b), axis=1), tr[:, 1])
    return np.where(t1 > t0, t1 - t0, 0.0) * np.linalg.norm(d, axis=1)


@pytest.mark.parametrize("shape,n", FAMILIES)
def test_a_grid_of_ones_gives_the_chord_through_the_box(ctx, shape, n):
    """The chords of a ray add up to its chord through the whole grid: the n <= nx + ny + nz differences of plane parameters
    telescope, each rounded to 2^-53 t_far, the sum once more per term."""
    nx, ny, nz = shape
    origin, voxel = grid_geometry(shape)
    ctx.set_grid(shape, origin, voxel, "f64")
    ctx.write_grid(np.ones((nz, ny, nx)))
    o, d, tr, vox = family_reference(shape, n)
    got = ctx.tally_rays(o, d, tr, want="integral")["integral"]
    ref = box_chord(shape, o, d, tr)
    bound = (nx + ny + nz + 2) * 2.0 ** -52 * np.array([v["t_far"] * v["length"] for v in vox])
    print("%s: worst |integral - box chord| / bound = %.3g" % (shape, float(np.max(np.abs(got - ref) / bound))))
    assert np.all(np.abs(got - ref) <= bound) and np.count_nonzero(got) == np.count_nonzero(ref) > n // 2


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [s for s, _ in FAMILIES])
def test_axis_parallel_rays_through_every_column_centre(ctx, shape, dtype):
    """Along an axis, through a column's centre, |d| = 1, starting half a voxel outside: integral = the column's sum x the voxel
    size, maximum and first crossing are the column's -- no reference involved (u64fx: against the exact raw sums).
    The bound on the integral, for a column of n voxels of size v: a plane parameter t_k = (origin + k v) - o carries the
    roundings of k v and of the sum, at most 2^-53 2 n v together, and that of the difference, at most 2^-53 t_far = 2^-53 (n +
    1/2) v: |error of t_k| <= 1.5 2^-52 (n + 1/2) v.  A chord is the rounded difference of two of them: v (1 + e), |e| <= 2^-52 (3 n
    + 2).  The n products and n - 1 additions of either side add n 2^-52 as in the sums suite, projection x voxel one rounding
    more:  |got - ref| <= (4 n + 3) 2^-52 ref.  (A single wrong or missing voxel is an error of order ref / n.  The ratio to the
    plain n 2^-52 ref is printed beside it: on an MI355X at most 0.97 for the columns of three voxels or more, 1.02 .. 1.16 for
    columns of one voxel, where six roundings meet one term.)"""
    g = load(ctx, shape, dtype)
    w = as_weight(g)
    origin, voxel = (np.asarray(v) for v in grid_geometry(shape))
    thr = thresholds_of(g)[1]
    flat = np.arange(g.size, dtype=np.int64).reshape(g.shape)
    for axis, keep in ((0, "yz"), (1, "xz"), (2, "xy")):                       # rays along x, y, z; numpy axis of [nz, ny, nx]: 2 - axis
        na = 2 - axis
        others = [a for a in (2, 1, 0) if a != axis]                           # the kept axes in (z, y, x) order, as tally_sum shapes them
        centres = [origin[a] + (np.arange(shape[a]) + 0.5) * voxel[a] for a in others]
        c0, c1 = np.meshgrid(*centres, indexing="ij")
        n_terms = shape[axis]
        proj = ctx.tally_sum(keep)
        if dtype == "u64fx":
            proj = ctx.tally_sum(keep, raw=True).astype(np.float64) * 2.0 ** -40     # the exact raw sums (each below 2^53 here)
        for sign in (1.0, -1.0):
            o = np.empty(c0.shape + (3,))
            o[..., others[0]], o[..., others[1]] = c0, c1
            o[..., axis] = origin[axis] - 0.5 * voxel[axis] if sign > 0 else origin[axis] + (shape[axis] + 0.5) * voxel[axis]
            d = np.zeros(c0.shape + (3,))
            d[..., axis] = sign
            got = ctx.tally_rays(o.reshape(-1, 3), d.reshape(-1, 3), threshold=thr)
            ref = proj * voxel[axis]
            err = np.abs(got["integral"].reshape(c0.shape) - ref)
            what = "%s %s along %s%s" % (shape, dtype, "+" if sign > 0 else "-", "xyz"[axis])
            rel = float(np.max(err / np.where(ref > 0, 2.0 ** -52 * ref, 1.0)))
            print("%s: worst |integral - projection x voxel| / ((4 n + 3) 2^-52 ref) = %.3g, / (n 2^-52 ref) = %.3g" % (what, rel / (4 * n_terms + 3), rel / n_terms))
            assert np.all(err <= (4 * n_terms + 3) * 2.0 ** -52 * ref), what
            ordered = w if sign > 0 else np.flip(w, axis=na)
            ordered_flat = flat if sign > 0 else np.flip(flat, axis=na)
            assert np.array_equal(got["max"].reshape(c0.shape), w.max(axis=na)), what
            first_max = np.take_along_axis(ordered_flat, np.expand_dims(np.argmax(ordered, axis=na), na), na).squeeze(na)
            assert np.array_equal(got["max_index"].reshape(c0.shape), first_max), what
            above = ordered >= thr
            first = np.take_along_axis(ordered_flat, np.expand_dims(np.argmax(above, axis=na), na), na).squeeze(na)
            assert np.array_equal(got["first_index"].reshape(c0.shape), np.where(above.any(axis=na), first, -1)), what


def test_rays_on_face_planes_follow_the_floor_rule(ctx):
    """Origin (0, 0, 0), voxel (1, 1, 1): every plane coordinate and every parameter below is an integer or a half, exact in f64."""
    nx, ny, nz = shape = (5, 4, 3)
    ctx.set_grid(shape, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), "f64")
    g = np.random.RandomState(9).randint(1, 100, size=(nz, ny, nx)).astype(np.float64)
    ctx.write_grid(g)
    rows = []                                                                   # (o, d, the voxels in order, or None for a miss)
    for m in range(ny + 1):                                                     # two zero components: y = m on a plane, z = k on a plane
        for k in range(nz + 1):
            hit = m < ny and k < nz
            rows.append(((-1.0, float(m), float(k)), (1.0, 0.0, 0.0), (k * ny + m) * nx + np.arange(nx) if hit else None))
            rows.append(((nx + 1.0, float(m), float(k)), (-2.0, 0.0, 0.0), (k * ny + m) * nx + np.arange(nx)[::-1] if hit else None))
    for m in range(nx + 1):
        rows.append(((float(m), 1.5, -0.5), (0.0, 0.0, 1.0), (np.arange(nz) * ny + 1) * nx + m if m < nx else None))
    o, d = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    got = ctx.tally_rays(o, d, threshold=0.0)
    for k, (_, dk, idx) in enumerate(rows):
        if idx is None:
            assert got["integral"][k] == 0 and got["max_index"][k] == -1 and got["first_index"][k] == -1 and np.isinf(got["first_t"][k]) and got["max"][k] == 0
            continue
        vals = g.ravel()[idx]
        assert got["integral"][k] == vals.sum() and got["max"][k] == vals.max() and got["max_index"][k] == idx[np.argmax(vals)], k
        assert got["first_index"][k] == idx[0] and got["first_t"][k] == (1.0 if dk[0] == 1.0 else 0.5), k
    # one zero component: z = m on a plane belongs to layer m, z = nz misses; the ray runs obliquely in x and y
    o = np.array([(-1.0, 0.25, float(m)) for m in range(nz + 1)] + [(-1.0, 0.25, 0.0)])
    d = np.array([(1.0, 0.5, 0.0)] * (nz + 1) + [(1.0, 0.5, -0.0)])
    got = ctx.tally_rays(o, d, threshold=0.0)
    vox = ray_voxels_numpy(shape, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), o, d)
    check_rays(got, ray_results_numpy(g, vox, 0.0), vox, "oblique rays in the planes z = m", exact_parameters=True)      # t = p + 1 and 2 q - 1/2
    assert np.array_equal(got["max_index"] // (nx * ny), [0, 1, 2, -1, 0]) and np.array_equal(got["first_index"] // (nx * ny), [0, 1, 2, -1, 0])


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_single_voxel(ctx, dtype):
    shape = (1, 1, 1)
    g = load(ctx, shape, dtype)
    if not g.ravel()[0]:
        g = np.full((1, 1, 1), 3 << 38 if dtype == "u64fx" else 0.75, dtype=g.dtype)
        ctx.write_grid(g)
    o, d, tr, vox = family_reference(shape, 600)
    w = float(as_weight(g).ravel()[0])
    got = ctx.tally_rays(o, d, tr, threshold=w)
    chord = box_chord(shape, o, d, tr)
    t_far, length = np.array([v["t_far"] for v in vox]), np.array([v["length"] for v in vox])
    err = np.abs(got["integral"] - w * chord)
    assert np.all(err <= BOUND * (t_far * length * w + w * chord))
    crossed = chord > 0
    assert np.array_equal(got["max_index"], np.where(crossed, 0, -1)) and np.array_equal(got["first_index"], np.where(crossed, 0, -1))
    assert np.array_equal(got["max"], np.where(crossed, w, 0.0)) and crossed.sum() > 300


def view_setup(shape):
    origin, voxel = (np.asarray(v) for v in grid_geometry(shape))
    size = np.asarray(shape) * voxel
    camera = origin + 0.5 * size + np.array([0.3, -0.2, -2.5]) * size           # in front of the z = 0 face, off the axis
    f_distance = camera[2] + 1.0
    return camera, f_distance


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("width,height", [(16, 16), (9, 5)])
def test_view_equals_rays_built_on_the_host(ctx, width, height, dtype):
    shape = (37, 19, 11)
    g = load(ctx, shape, dtype)
    camera, f = view_setup(shape)
    xs, ys = camera[0] + np.linspace(-0.61, 0.29, width), camera[1] + np.linspace(0.51, -0.29, height)      # screen coordinates: d = xs - camera.x
    thr = thresholds_of(g)[1]
    view = ctx.tally_view(camera, f, xs, ys, threshold=thr)
    o, d = _lib.camera_rays(camera, f, xs, ys)
    rays = ctx.tally_rays(o.reshape(-1, 3), d.reshape(-1, 3), threshold=thr)
    assert all(a.shape == (height, width) for a in view.values())
    assert same_bits({k: a.reshape(-1) for k, a in view.items()}, rays)
    assert same_bits(ctx.tally_view(camera, f, xs, ys, threshold=thr), view)    # a second call: identical bits
    for want, keys in (("integral", ("integral",)), ("max", ("max", "max_index")), ("first", ("first_t", "first_index"))):
        assert same_bits(ctx.tally_view(camera, f, xs, ys, threshold=thr, want=want), {k: view[k] for k in keys}), want
    assert np.count_nonzero(view["integral"]) > 0.2 * width * height and (view["max_index"] < 0).any()      # some pixels see the grid, some miss
    vox = ray_voxels_numpy(shape, *grid_geometry(shape), o.reshape(-1, 3), d.reshape(-1, 3))
    check_rays(rays, ray_results_numpy(g, vox, thr), vox, "camera rays %dx%d %s" % (width, height, dtype))


def test_side_effects(ctx):
    prob = S.slab(n=16, voxel=0.8)
    prob.apply(ctx, "u64fx")
    ctx.stats_enable(True)
    for b in range(2):
        ctx.launch(1024, seed=5, photon_offset=1024 * b)
        ctx.stats_fold()
    labels = (np.arange(16 ** 3) % 3).astype(np.uint8).reshape(16, 16, 16)
    ctx.set_labels(labels, 3)
    g, m2, c0, sums = ctx.read_grid_raw(), ctx.stats_m2(), ctx.read_counters(), ctx.tally_label_sums(raw=True)["raw"]
    rs = np.random.RandomState(3)
    o, d = rs.standard_normal((200, 3)) * 10.0, rs.standard_normal((200, 3))
    first = ctx.tally_rays(o, d, threshold=1e-3)
    view = ctx.tally_view((0.5, 0.25, -20.0), -19.0, np.linspace(-1, 1, 20), np.linspace(1, -1, 12), threshold=1e-3)
    assert np.count_nonzero(first["integral"]) > 20 and np.count_nonzero(view["integral"]) > 20
    assert np.array_equal(ctx.read_grid_raw(), g) and ctx.read_counters() == c0
    assert np.array_equal(ctx.stats_m2(), m2) and ctx.stats_batches() == 2
    assert ctx.labels_info() == 3 and np.array_equal(ctx.tally_label_sums(raw=True)["raw"], sums)
    assert same_bits(ctx.tally_rays(o, d, threshold=1e-3), first)
    ctx.set_labels(None)
    ctx.stats_enable(False)


def test_error_codes(ctx):
    L = _lib.lib()
    n = 4
    o, d = np.zeros((n, 3)), np.tile([0.0, 0.0, 1.0], (n, 1))
    out, idx = np.zeros(n), np.zeros(n, dtype=np.int64)
    p, ip = _lib._dp, lambda a: a.ctypes.data_as(_I64P)      # noqa: E731
    cam, xs, ys = (C.c_double * 3)(0.0, 0.0, -5.0), np.linspace(-1, 1, 2), np.linspace(1, -1, 2)

    def rays(h, o_=o, d_=d, tr=None, n_=n, thr=0.0, outs=None):
        a = (p(out), None, None, None, None) if outs is None else outs
        return L.lt_tally_rays(h, None if o_ is None else p(o_), None if d_ is None else p(d_), None if tr is None else p(tr), n_, thr, *a)

    def view(h, w=2, hgt=2, cam_=cam, f=-4.0, xs_=xs, ys_=ys, thr=0.0, outs=None):
        a = (p(out), None, None, None, None) if outs is None else outs
        return L.lt_tally_view(h, w, hgt, cam_, f, None if xs_ is None else p(xs_), None if ys_ is None else p(ys_), thr, *a)

    with lt.Context(0) as fresh:
        assert rays(fresh._h) == E_STATE and view(fresh._h) == E_STATE
    load(ctx, (37, 19, 11), "f64")
    h = ctx._h
    assert rays(h) == 0 and view(h) == 0
    assert rays(h, outs=(None,) * 5) == E_INVALID and b"no output" in L.lt_last_error(h)
    assert view(h, outs=(None,) * 5) == E_INVALID
    assert rays(h, o_=None) == E_INVALID and rays(h, d_=None) == E_INVALID and rays(h, n_=0) == E_INVALID
    assert view(h, cam_=None) == E_INVALID and view(h, xs_=None) == E_INVALID and view(h, ys_=None) == E_INVALID
    assert view(h, w=0) == E_INVALID and view(h, hgt=0) == E_INVALID
    for bad in (np.nan, np.inf):
        o2 = o.copy()
        o2[2, 1] = bad
        assert rays(h, o_=o2) == E_INVALID and b"ray 2" in L.lt_last_error(h)
        d2 = d.copy()
        d2[3, 0] = bad
        assert rays(h, d_=d2) == E_INVALID and b"ray 3" in L.lt_last_error(h)
    d2 = d.copy()
    d2[1] = 0.0
    assert rays(h, d_=d2) == E_INVALID and b"ray 1" in L.lt_last_error(h)
    good = np.tile([0.0, np.inf], (n, 1))
    assert rays(h, tr=good) == 0
    for k, pair in enumerate(((-0.5, 1.0), (np.nan, 1.0), (np.inf, np.inf), (1.0, 1.0), (2.0, 1.0), (0.0, np.nan))):
        tr = good.copy()
        tr[k % n] = pair
        assert rays(h, tr=tr) == E_INVALID and ("ray %d" % (k % n)).encode() in L.lt_last_error(h), pair
    first = (None, None, None, p(out), None)
    for thr in (-1.0, np.nan, np.inf):
        assert rays(h, thr=thr, outs=first) == E_INVALID and view(h, thr=thr, outs=(None, None, None, None, ip(idx))) == E_INVALID
        assert rays(h, thr=thr) == 0 and view(h, thr=thr, outs=(None, p(out), ip(idx), None, None)) == 0      # nobody asked for a crossing
    # camera rays: pixel (1, 1) of xs = (-1, 0), ys = (1, 0) seen from (0, 0, z) with f_distance = z is the zero vector
    xs0, ys0 = np.array([-1.0, 0.0]), np.array([1.0, 0.0])
    assert view(h, cam_=(C.c_double * 3)(0.0, 0.0, -5.0), f=-5.0, xs_=xs0, ys_=ys0) == E_INVALID and b"ray 3" in L.lt_last_error(h)
    assert view(h, f=np.inf) == E_INVALID and view(h, cam_=(C.c_double * 3)(0.0, np.nan, -5.0)) == E_INVALID
    assert view(h, xs_=np.array([0.0, np.nan])) == E_INVALID and b"ray 1" in L.lt_last_error(h)
    assert view(h, ys_=np.array([0.0, np.inf])) == E_INVALID and b"ray 2" in L.lt_last_error(h)
    with pytest.raises(lt.LtError):
        ctx.tally_rays(o, d[:-1])
    with pytest.raises(ValueError):
        ctx.tally_rays(o, d, want="depth")


def slab_tracer(ctx, quantity="absorbed"):
    """S.slab(n=32, voxel=0.8) through the object API, 4096 photons into a u64 fixed-point grid."""
    tr = PT.PhotonTracer(ctx=ctx)
    tr.configure(PT.LayeredSlab([PT.OpticalMedium(0.1, 10.0, 0.9, 1.0)], [np.inf]),
                 PT.VoxelGrid((32, 32, 32), (-12.8, -12.8, 0.0), 0.8, dtype="u64fx"), PT.PencilBeam((0, 0, 0), (0, 0, 1)), quantity=quantity)
    return tr.run(4096, seed=123)


@pytest.mark.parametrize("quantity", ["absorbed", "fluence"])
def test_end_to_end_parallel_projection_along_z(ctx, quantity):
    tr = slab_tracer(ctx, quantity)
    got = tr.parallel_projection((0, 0, 1), (0.0, 0.0, 5.0), (0, -1, 0), 32, 32, 25.6)
    proj = ctx.tally_sum("xy")                                                  # weight per column
    ref = proj * 0.8 / (0.8 ** 3 * (4096.0 if quantity == "fluence" else 1.0))
    if quantity == "fluence":
        assert np.allclose(ref, tr.projection("z") * 32 * 0.8, rtol=1e-14, atol=0)      # the mean fluence x the path through the grid
    o, _ = tr.parallel_rays((0, 0, 1), (0.0, 0.0, 5.0), (0, -1, 0), 32, 32, 25.6)
    t_far = 25.6 - o[0, 0, 2]
    err, bound = np.abs(got - ref), BOUND * (t_far * proj + proj * 0.8) / (0.8 ** 3 * (4096.0 if quantity == "fluence" else 1.0))
    print("parallel projection along z (%s): worst err / bound = %.3g" % (quantity, float(np.max(err / np.where(bound > 0, bound, 1.0)))))
    assert got.shape == (32, 32) and np.all(err <= bound) and got.max() > 0
    assert tr.line_integral((0.4, 0.4, -1.0), (0.4, 0.4, 30.0)) == pytest.approx(got[16, 16], rel=1e-12)


def test_end_to_end_depth_seen_through_a_camera(ctx):
    tr = slab_tracer(ctx)
    g = ctx.read_grid_raw()
    scene = Scene(np.array([0.31, -0.17, -30.3, 1.0]), [], width=24, height=16, max_depth=1, f_distance=-26.2, number_of_samples=1)      # (round numbers send rays through voxel edges)
    w = as_weight(g)
    thr = float(np.sort(w[w > 0])[-200])                                        # the 200 hottest voxels: a small core under the beam
    depth, peak = tr.view(scene, "depth", threshold=thr), tr.view(scene, "max")
    assert depth.shape == peak.shape == (16, 24) and np.isfinite(depth).any() and np.isinf(depth).any()
    assert np.array_equal(np.isfinite(depth), peak >= thr)                       # a depth exactly where the ray meets a voxel above the threshold
    xs, ys = np.linspace(scene.left, scene.right, 24), np.linspace(scene.top, scene.bottom, 16)
    o, d = _lib.camera_rays(scene.camera[:3], scene.f_distance, xs, ys)
    vox = ray_voxels_numpy((32, 32, 32), (-12.8, -12.8, 0.0), (0.8, 0.8, 0.8), o.reshape(-1, 3), d.reshape(-1, 3))
    ref = ray_results_numpy(g, vox, thr)
    ok = ~np.array([v["grazing"] for v in vox])
    assert np.array_equal(np.isfinite(depth).ravel()[ok], (ref["first_index"] >= 0)[ok]) and ok.mean() >= 0.99
    hit = ok & (ref["first_index"] >= 0)
    length = np.linalg.norm(d.reshape(-1, 3), axis=1)
    assert np.allclose(depth.ravel()[hit], (ref["first_t"] * length)[hit], rtol=1e-12, atol=0)
    assert np.all(depth.ravel()[hit] >= 30.3)                                    # the grid begins 30.3 below the camera
    # the integral seen through the camera, against the reference
    view = tr.view(scene)
    full = ray_results_numpy(g, vox, 0.0)
    t_far = np.array([v["t_far"] for v in vox])
    assert np.all(np.abs(view.ravel() * 0.8 ** 3 - full["integral"]) <= BOUND * (t_far * length * full["met_sum"] + full["integral"]) * (1 + 2.0 ** -50))
