"""CPU suite of the tally along rays: the two entry points exist at every layer; ray_chords_numpy is the brute-force REFERENCE of
lt_tally_rays (the GPU suite imports it, with the ray families and the reductions below): every (ray, voxel) pair is intersected by
the slab method on that voxel's own box -- no traversal, no neighbour relation, nothing shared with the device code but the
definitions of lt.h.  The reference is pinned on cases worked by hand; the PhotonTracer methods on top -- view, line_integral,
parallel_projection -- are driven by a stub context whose methods are the reference.

Grazing.  lt.h leaves open whether a voxel that a ray only grazes is visited.  A ray is called grazing here if some voxel has a
chord (in the ray's parameter) of at most delta = 2^-40 x the ray's far parameter while its box, inflated by 2^-40 x the grid's
diagonal, is still met: then "which voxels have a chord > 0" depends on the last bits.  The seeded families the GPU suite uses
hold no such ray (at most 1 % may be), so that maxima, indices and first crossings can be compared exactly."""
import ctypes
import os
import re

import numpy as np
import pytest

import light_transport_amd as lt
from light_transport_amd import _lib
from light_transport_amd.src import photon_tracing as PT
from light_transport_amd.src.scene import Scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("lt_tally_rays", "lt_tally_view")
GRAZE = 2.0 ** -40
CHUNK_ELEMENTS = 1 << 21          # (ray, voxel) pairs of one chunk of the reference


def as_weight(g):
    """A raw tally as lt_read_grid_f64 converts it: u64 -> (double)raw * 2^-40 (one rounding), floats widened."""
    g = np.asarray(g)
    return g.astype(np.float64) * 2.0 ** -40 if g.dtype == np.uint64 else g.astype(np.float64)


def _axis_interval(n, origin, voxel, o, d, inflate):
    """(enter, exit) [rays, n]: the parameter interval in which each ray lies inside each of the n slabs [origin + i voxel, origin +
    (i + 1) voxel) of one axis, widened by ``inflate`` on both sides.  d == 0: the ray lies in the slab floor((o - origin) / voxel)
    for every t (-inf, +inf) and in no other (+inf, -inf)."""
    planes = origin + np.arange(n + 1, dtype=np.float64) * voxel
    lo, hi = planes[None, :-1] - inflate, planes[None, 1:] + inflate
    oo, dd = o[:, None], d[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        t_lo, t_hi = (lo - oo) / dd, (hi - oo) / dd
    enter, leave = np.where(dd > 0, t_lo, t_hi), np.where(dd > 0, t_hi, t_lo)
    if inflate == 0.0:
        inside = np.floor((oo - origin) / voxel) == np.arange(n, dtype=np.float64)[None, :]
    else:
        inside = (oo >= lo) & (oo <= hi)
    still = dd == 0
    enter = np.where(still, np.where(inside, -np.inf, np.inf), enter)
    leave = np.where(still, np.where(inside, np.inf, -np.inf), leave)
    return enter, leave


def ray_chords_numpy(shape, origin, voxel, o, d, t_range=None, inflate=0.0):
    """THE REFERENCE.  shape = (nx, ny, nz); o, d [rays, 3]; t_range [rays, 2] or None = [0, inf).  For every (ray, voxel) pair the
    slab method on that voxel's box: dict of [rays, nz * ny * nx] arrays --
        t_in     max(enters, t_lo), the parameter at which the ray enters the voxel
        chord_t  max(0, min(exits, t_hi) - t_in), chord = chord_t |d| the geometric length inside the voxel
        met      min(exits, t_hi) >= t_in (with ``inflate`` > 0: the box widened by that much on every side is still touched)
    and ``length`` [rays] = |d|.  Dense: the caller keeps rays x voxels within memory (ray_voxels_numpy cuts it into chunks)."""
    o, d = np.asarray(o, dtype=np.float64).reshape(-1, 3), np.asarray(d, dtype=np.float64).reshape(-1, 3)
    n = o.shape[0]
    tr = np.broadcast_to(np.array([0.0, np.inf]) if t_range is None else np.asarray(t_range, dtype=np.float64), (n, 2))
    ex, lx = _axis_interval(shape[0], origin[0], voxel[0], o[:, 0], d[:, 0], inflate)
    ey, ly = _axis_interval(shape[1], origin[1], voxel[1], o[:, 1], d[:, 1], inflate)
    ez, lz = _axis_interval(shape[2], origin[2], voxel[2], o[:, 2], d[:, 2], inflate)
    t_in = np.maximum(np.maximum(ex[:, None, None, :], ey[:, None, :, None]), np.maximum(ez[:, :, None, None], tr[:, 0, None, None, None]))
    t_out = np.minimum(np.minimum(lx[:, None, None, :], ly[:, None, :, None]), np.minimum(lz[:, :, None, None], tr[:, 1, None, None, None]))
    with np.errstate(invalid="ignore"):
        chord_t = np.where(t_out > t_in, t_out - t_in, 0.0)
    length = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    return dict(t_in=t_in.reshape(n, -1), chord_t=chord_t.reshape(n, -1), chord=(chord_t * length[:, None, None, None]).reshape(n, -1),
                met=(t_out >= t_in).reshape(n, -1), length=length)


def far_parameter(shape, origin, voxel, o, d):
    """[rays]: the largest |parameter| of the grid's bounding planes along each ray (axes the ray does not move along left out)."""
    o, d = np.asarray(o, dtype=np.float64).reshape(-1, 3), np.asarray(d, dtype=np.float64).reshape(-1, 3)
    far = np.zeros(o.shape[0])
    for a in range(3):
        for plane in (origin[a], origin[a] + shape[a] * voxel[a]):
            with np.errstate(divide="ignore", invalid="ignore"):
                t = np.abs((plane - o[:, a]) / d[:, a])
            far = np.maximum(far, np.where(d[:, a] != 0, t, 0.0))
    return far


def ray_voxels_numpy(shape, origin, voxel, o, d, t_range=None):
    """The reference per ray, from ray_chords_numpy in chunks of rays: a list of dicts -- ``index`` (flat indices of the voxels with
    chord > 0, in the order the ray enters them), ``chord``, ``t_in``, ``length`` = |d|, ``t_far`` and ``grazing`` (module docstring)."""
    o, d = np.asarray(o, dtype=np.float64).reshape(-1, 3), np.asarray(d, dtype=np.float64).reshape(-1, 3)
    n, n_vox = o.shape[0], shape[0] * shape[1] * shape[2]
    tr = np.broadcast_to(np.array([0.0, np.inf]) if t_range is None else np.asarray(t_range, dtype=np.float64), (n, 2))
    far = far_parameter(shape, origin, voxel, o, d)
    diagonal = float(np.linalg.norm(np.asarray(shape, dtype=np.float64) * np.asarray(voxel, dtype=np.float64)))
    per, out = max(1, CHUNK_ELEMENTS // n_vox), []
    for r0 in range(0, n, per):
        sl = slice(r0, min(n, r0 + per))
        c = ray_chords_numpy(shape, origin, voxel, o[sl], d[sl], tr[sl])
        wide = ray_chords_numpy(shape, origin, voxel, o[sl], d[sl], tr[sl], inflate=GRAZE * diagonal)
        grazing = np.any(wide["met"] & (c["chord_t"] <= GRAZE * far[sl, None]), axis=1)
        for k in range(c["chord"].shape[0]):
            idx = np.flatnonzero(c["chord"][k] > 0)
            idx = idx[np.argsort(c["t_in"][k, idx], kind="stable")]
            out.append(dict(index=idx.astype(np.int64), chord=c["chord"][k, idx], t_in=c["t_in"][k, idx], length=float(c["length"][k]),
                            t_far=float(far[r0 + k]), grazing=bool(grazing[k])))
    return out


def ray_results_numpy(raw, voxels, threshold):
    """What lt_tally_rays returns, from the reference's voxels per ray and a raw tally [nz, ny, nx]: dict of [rays] arrays integral,
    met_sum (the sum of the voxels the ray meets, as weight), max (as weight), max_index, first_t, first_index."""
    flat = np.asarray(raw).ravel()
    n = len(voxels)
    res = dict(integral=np.zeros(n), met_sum=np.zeros(n), max=np.zeros(n), max_index=np.full(n, -1, dtype=np.int64),
               first_t=np.full(n, np.inf), first_index=np.full(n, -1, dtype=np.int64))
    for k, v in enumerate(voxels):
        if not v["index"].size:
            continue
        w = flat[v["index"]]
        wd = as_weight(w)
        res["integral"][k], res["met_sum"][k] = float(np.sum(wd * v["chord"])), float(np.sum(wd))
        top = int(np.argmax(w))                                  # the raw values are compared; argmax: the first of equal maxima
        res["max"][k], res["max_index"][k] = wd[top], v["index"][top]
        above = np.flatnonzero(wd >= threshold)
        if above.size:
            res["first_t"][k], res["first_index"][k] = v["t_in"][above[0]], v["index"][above[0]]
    return res


def grid_geometry(shape):
    """(origin, voxel) of tests.test_gpu_tally_sums.load for a grid of shape (nx, ny, nz)."""
    nx, ny, _ = shape
    return (-0.5 * nx * 0.1, -0.5 * ny * 0.2, 0.0), (0.1, 0.2, 0.3)


RAY_KINDS = ("outside to inside", "starting inside", "t_lo > 0", "ending at the target", "missing the grid", "pointing away")


def ray_family(shape, n, seed):
    """(o [n, 3], d [n, 3], t_range [n, 2]), seeded, ray r of kind RAY_KINDS[r % 6], in the geometry of grid_geometry: origins
    normally distributed about the grid (a few fall inside), aimed at points uniform inside it, |d| scaled by 0.1 .. 10;
    "starting inside" starts at a uniform point inside; "t_lo > 0" starts part of the way to its target (t = 1); "ending at the
    target" has t_hi = 1; "missing the grid" passes two grid diagonals from the centre; "pointing away" runs backwards."""
    rs = np.random.RandomState(seed)
    origin, voxel = (np.asarray(v) for v in grid_geometry(shape))
    size = np.asarray(shape, dtype=np.float64) * voxel
    centre, diagonal = origin + 0.5 * size, np.linalg.norm(size)
    kind = np.arange(n) % 6
    target = origin + rs.random_sample((n, 3)) * size
    o = centre + rs.standard_normal((n, 3)) * 1.5 * size
    o[kind == 1] = (origin + rs.random_sample((n, 3)) * size)[kind == 1]
    d = (target - o) * (10.0 ** rs.uniform(-1, 1, size=n))[:, None]
    scale = np.linalg.norm(d, axis=1) / np.linalg.norm(target - o, axis=1)
    d[kind == 5] *= -1.0
    u = rs.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    p = np.cross(u, rs.standard_normal((n, 3)))
    p /= np.linalg.norm(p, axis=1)[:, None]
    miss = kind == 4
    o[miss] = (centre + 2.0 * diagonal * p - 3.0 * diagonal * u)[miss]
    d[miss] = u[miss]
    tr = np.tile(np.array([0.0, np.inf]), (n, 1))
    tr[kind == 2, 0] = (rs.uniform(0.1, 0.9, size=n) / scale)[kind == 2]
    tr[kind == 3, 1] = (1.0 / scale)[kind == 3]
    return np.ascontiguousarray(o), np.ascontiguousarray(d), tr


FAMILIES = [((1, 1, 1), 600), ((64, 1, 3), 600), ((37, 19, 11), 600), ((130, 70, 33), 64), ((16, 16, 600), 64)]
_family_cache = {}


def family_reference(shape, n):
    """(o, d, t_range, ray_voxels_numpy of them) of a GPU-suite family; computed once, shared, read-only."""
    if (shape, n) not in _family_cache:
        o, d, tr = ray_family(shape, n, 4242 + shape[0])
        origin, voxel = grid_geometry(shape)
        for a in (o, d, tr):
            a.setflags(write=False)
        _family_cache[(shape, n)] = (o, d, tr, ray_voxels_numpy(shape, origin, voxel, o, d, tr))
    return _family_cache[(shape, n)]


class StubContext:
    """Stands where the Context would: a raw grid [nz, ny, nx] in a geometry, tally_rays as the reference, tally_view as tally_rays
    on _lib.camera_rays; every call is recorded."""

    def __init__(self, grid, shape, origin, voxel):
        self.grid, self.shape, self.origin, self.voxel, self.calls = grid, shape, origin, voxel, []

    def tally_rays(self, origins, dirs, t_range=None, threshold=None, want=_lib.RAY_WANTS):
        o, d = np.asarray(origins, dtype=np.float64).reshape(-1, 3), np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
        self.calls.append(("tally_rays", o.shape[0], None if t_range is None else tuple(np.asarray(t_range).ravel()[:2]), threshold, _lib.ray_wants(want)))
        r = ray_results_numpy(self.grid, ray_voxels_numpy(self.shape, self.origin, self.voxel, o, d, t_range), 0.0 if threshold is None else threshold)
        keys = dict(integral=("integral",), max=("max", "max_index"), first=("first_t", "first_index"))
        return {k: r[k] for w in _lib.ray_wants(want) for k in keys[w]}

    def tally_view(self, camera, f_distance, xs, ys, threshold=None, want=_lib.RAY_WANTS):
        o, d = _lib.camera_rays(camera, f_distance, xs, ys)
        self.calls.append(("tally_view", tuple(np.asarray(camera).tolist()), f_distance, len(xs), len(ys)))
        return {k: a.reshape(d.shape[:2]) for k, a in self.tally_rays(o, d, None, threshold, want).items()}


SHAPE, ORIGIN, VOXEL = (6, 5, 4), (-0.3, -0.5, 0.0), (0.1, 0.2, 0.3)


def stub_tracer(grid, quantity="absorbed", photons=1000):
    tr = PT.PhotonTracer(ctx=StubContext(grid, SHAPE, ORIGIN, VOXEL))
    tr.grid = PT.VoxelGrid(SHAPE, ORIGIN, VOXEL)
    tr.quantity, tr.photons = quantity, photons
    return tr


def whole_weights(seed=8):
    rs = np.random.RandomState(seed)
    g = rs.randint(1, 1000, size=SHAPE[::-1]).astype(np.float64)
    g[rs.random_sample(g.shape) < 0.3] = 0.0
    return g


def test_the_symbols_are_declared_exported_and_bound():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lt.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lt_[a-z0-9_]+)\s*\(", txt))
    assert os.path.exists(lt.LIB_PATH), "liblt_hip.so not built: run __graft_entry__.build()"
    for name in NEW_SYMBOLS:
        assert name in declared, "%s is not declared in lt.h" % name
        assert getattr(_lib.lib(), name) is not None                   # resolves in the built library
        assert name in _lib.SYMBOLS and name in _lib.PROTOTYPES
    assert re.search(r"#define\s+LT_ABI_VERSION\s+3\b", txt) and ctypes.CDLL(lt.LIB_PATH).lt_abi_version() == 3
    for name in ("tally_rays", "tally_view"):
        assert callable(getattr(_lib.Context, name))
    for name in ("view", "line_integral", "parallel_projection", "parallel_rays"):
        assert callable(getattr(PT.PhotonTracer, name))


def one(shape, origin, voxel, o, d, t_range=None):
    return ray_voxels_numpy(shape, origin, voxel, [o], [d], None if t_range is None else [t_range])[0]


def test_the_reference_on_an_axis_parallel_ray_through_voxel_centres():
    v = one((5, 3, 2), (0.0, 0.0, 0.0), (0.5, 1.0, 2.0), (-1.0, 1.5, 3.0), (1.0, 0.0, 0.0))
    assert np.array_equal(v["index"], (1 * 3 + 1) * 5 + np.arange(5))              # row y = 1, z = 1, ascending x
    assert np.array_equal(v["chord"], [0.5] * 5) and np.array_equal(v["t_in"], [1.0, 1.5, 2.0, 2.5, 3.0])
    assert v["t_far"] == 3.5 and not v["grazing"]
    back = one((5, 3, 2), (0.0, 0.0, 0.0), (0.5, 1.0, 2.0), (9.0, 1.5, 3.0), (-2.0, 0.0, 0.0))
    assert np.array_equal(back["index"], v["index"][::-1]) and np.array_equal(back["chord"], [0.5] * 5)       # lengths are geometric
    g = np.arange(30, dtype=np.float64).reshape(2, 3, 5)
    r = ray_results_numpy(g, [v, back], 22.0)
    assert np.array_equal(r["integral"], [0.5 * (20 + 21 + 22 + 23 + 24)] * 2) and np.array_equal(r["max"], [24.0, 24.0])
    assert np.array_equal(r["max_index"], [24, 24]) and np.array_equal(r["first_index"], [22, 24])
    assert np.array_equal(r["first_t"], [2.0, (9.0 - 2.5) / 2.0])                 # the ray going back enters voxel 24 at x = 2.5


def test_the_reference_on_the_body_diagonal_of_a_cube_grid():
    v = one((4, 4, 4), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    assert np.array_equal(v["index"], [0, 21, 42, 63])                             # only the four voxels on the diagonal have a chord
    assert np.allclose(v["chord"], np.sqrt(3.0), rtol=1e-15) and np.array_equal(v["t_in"], [1.0, 2.0, 3.0, 4.0])
    assert v["grazing"]                                                            # it touches twelve more at their edges and corners


def test_the_reference_on_misses_starts_inside_and_finite_ends():
    shape, origin, voxel = (4, 3, 2), (1.0, 1.0, 1.0), (1.0, 1.0, 1.0)
    assert one(shape, origin, voxel, (0.0, 0.0, 0.0), (1.0, 0.0, 0.0))["index"].size == 0          # y, z outside their slabs
    assert one(shape, origin, voxel, (0.0, 1.5, 1.5), (-1.0, 0.1, 0.0))["index"].size == 0         # pointing away
    assert one(shape, origin, voxel, (0.0, 1.5, 1.5), (1.0, 0.0, 0.0), (6.0, 9.0))["index"].size == 0   # t_lo beyond the grid
    r = ray_results_numpy(np.ones((2, 3, 4)), [one(shape, origin, voxel, (0.0, 0.0, 0.0), (1.0, 0.0, 0.0))], 0.0)
    assert r["max"][0] == 0 and r["max_index"][0] == -1 and r["first_index"][0] == -1 and np.isinf(r["first_t"][0]) and r["integral"][0] == 0
    inside = one(shape, origin, voxel, (2.25, 1.5, 1.5), (1.0, 0.0, 0.0))          # starts inside voxel x = 1
    assert np.array_equal(inside["index"], [1, 2, 3]) and np.array_equal(inside["chord"], [0.75, 1.0, 1.0])
    assert np.array_equal(inside["t_in"], [0.0, 0.75, 1.75])                       # never below t_lo
    ends = one(shape, origin, voxel, (0.0, 1.5, 1.5), (1.0, 0.0, 0.0), (0.0, 3.25))   # ends a quarter into voxel x = 2
    assert np.array_equal(ends["index"], [0, 1, 2]) and np.array_equal(ends["chord"], [1.0, 1.0, 0.25])
    late = one(shape, origin, voxel, (0.0, 1.5, 1.5), (1.0, 0.0, 0.0), (1.5, np.inf))
    assert np.array_equal(late["index"], [0, 1, 2, 3]) and np.array_equal(late["chord"], [0.5, 1.0, 1.0, 1.0]) and late["t_in"][0] == 1.5


def test_the_reference_with_a_zero_direction_component_on_a_face_plane():
    shape, origin, voxel = (3, 4, 2), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    for m in range(4):                                                             # y = m exactly: column m (the floor rule)
        v = one(shape, origin, voxel, (-1.0, float(m), 0.5), (1.0, 0.0, 0.0))
        assert np.array_equal(v["index"], m * 3 + np.arange(3))
    assert one(shape, origin, voxel, (-1.0, 4.0, 0.5), (1.0, 0.0, 0.0))["index"].size == 0          # y = ny misses
    assert one(shape, origin, voxel, (-1.0, -1e-300, 0.5), (1.0, 0.0, 0.0))["index"].size == 0


def test_the_reference_under_a_scaled_direction():
    shape = (7, 5, 3)
    origin, voxel = grid_geometry(shape)
    o, d = np.array([-1.3, 0.9, -0.4]), np.array([0.7, -0.45, 0.31])
    g = np.random.RandomState(2).random_sample(shape[::-1])
    base = ray_results_numpy(g, [one(shape, origin, voxel, o, d)], 0.5)
    assert base["first_index"][0] >= 0 and base["integral"][0] > 0
    for k in (7.0, 1e-3):
        r = ray_results_numpy(g, [one(shape, origin, voxel, o, d * k)], 0.5)
        assert abs(r["integral"][0] - base["integral"][0]) <= 1e-14 * base["integral"][0]
        assert abs(r["first_t"][0] * k - base["first_t"][0]) <= 1e-14 * base["first_t"][0]
        assert r["first_index"][0] == base["first_index"][0] and r["max_index"][0] == base["max_index"][0] and r["max"][0] == base["max"][0]


def test_camera_rays_follow_the_formula_of_the_header():
    cam, f, xs, ys = np.array([0.25, -0.5, -3.0]), 1.5, np.linspace(-1, 1, 5), np.linspace(0.8, -0.8, 3)
    o, d = _lib.camera_rays(cam, f, xs, ys)
    assert o.shape == d.shape == (3, 5, 3) and o.flags["C_CONTIGUOUS"] and d.flags["C_CONTIGUOUS"]
    for i in range(3):
        for j in range(5):
            assert np.array_equal(o[i, j], cam) and np.array_equal(d[i, j], [xs[j] - cam[0], ys[i] - cam[1], f - cam[2]])
    assert _lib.ray_wants("max") == ("max",) and _lib.ray_wants(["first", "integral"]) == ("integral", "first")
    for bad in ((), "depth", ("integral", "min")):
        with pytest.raises(ValueError):
            _lib.ray_wants(bad)


def test_view_through_a_scene_and_its_normalisation():
    g = whole_weights()
    scene = Scene(np.array([0.05, 0.1, -2.0, 1.0]), [], width=7, height=5, max_depth=1, f_distance=-1.0, number_of_samples=1)
    xs, ys = np.linspace(scene.left, scene.right, 7), np.linspace(scene.top, scene.bottom, 5)
    o, d = _lib.camera_rays(scene.camera[:3], scene.f_distance, xs, ys)
    vox = ray_voxels_numpy(SHAPE, ORIGIN, VOXEL, o.reshape(-1, 3), d.reshape(-1, 3))
    ref = ray_results_numpy(g, vox, 500.0)
    volume = VOXEL[0] * VOXEL[1] * VOXEL[2]
    tr = stub_tracer(g)
    got = tr.view(scene)
    assert got.shape == (5, 7) and np.array_equal(got, ref["integral"].reshape(5, 7) / volume) and got.max() > 0
    assert tr.ctx.calls[0] == ("tally_view", (0.05, 0.1, -2.0), -1.0, 7, 5) and tr.ctx.calls[1][4] == ("integral",)
    assert np.array_equal(tr.view(scene, "max"), ref["max"].reshape(5, 7))
    depth = tr.view(scene, "depth", threshold=500.0)
    assert np.array_equal(depth, (ref["first_t"] * np.linalg.norm(d.reshape(-1, 3), axis=1)).reshape(5, 7))
    assert np.isfinite(depth).any() and np.isinf(depth).any() and tr.ctx.calls[-1][3] == 500.0 and tr.ctx.calls[-1][4] == ("first",)
    fl = stub_tracer(g, quantity="fluence", photons=250)
    assert np.array_equal(fl.view(scene), ref["integral"].reshape(5, 7) / (volume * 250.0))
    assert np.array_equal(fl.view(scene, "max"), ref["max"].reshape(5, 7) / (volume * 250.0))
    assert np.array_equal(fl.view(scene, "depth", threshold=500.0 / (volume * 250.0)), depth)       # the threshold is a fluence
    assert fl.ctx.calls[-1][3] == 500.0 / (volume * 250.0) * (volume * 250.0)
    for what, thr in (("dose", None), ("depth", None), ("depth", -1.0), ("depth", np.inf)):
        with pytest.raises(ValueError):
            tr.view(scene, what, threshold=thr)
    with pytest.raises(ValueError):
        stub_tracer(g, quantity="fluence", photons=0).view(scene)


def test_line_integral():
    g = whole_weights()
    tr = stub_tracer(g)
    p0, p1 = np.array([-0.25, -0.45, 0.1]), np.array([0.1, 0.1, 0.7])
    ref = ray_results_numpy(g, ray_voxels_numpy(SHAPE, ORIGIN, VOXEL, [p0], [p1 - p0], [(0.0, 1.0)]), 0.0)["integral"][0]
    got = tr.line_integral(p0, p1)
    assert isinstance(got, float) and got == ref / (VOXEL[0] * VOXEL[1] * VOXEL[2]) and got > 0
    assert tr.ctx.calls[-1] == ("tally_rays", 1, (0.0, 1.0), None, ("integral",))
    whole = ray_results_numpy(g, ray_voxels_numpy(SHAPE, ORIGIN, VOXEL, [p0], [p1 - p0]), 0.0)["integral"][0]
    assert whole > ref                                                             # the segment ends inside the grid
    assert stub_tracer(g, "fluence", 40).line_integral(p0, p1) == ref / (VOXEL[0] * VOXEL[1] * VOXEL[2] * 40.0)
    for bad in ((p0, p0), (p0, [np.nan, 0, 0])):
        with pytest.raises(ValueError):
            tr.line_integral(*bad)


def test_parallel_projection_rays_and_result():
    g = whole_weights()
    tr = stub_tracer(g)
    nx, ny, nz = SHAPE
    centre = (ORIGIN[0] + 0.5 * nx * VOXEL[0], ORIGIN[1] + 0.5 * ny * VOXEL[1], 0.4)
    # along +z with rows following +y: a ray through every column centre
    o, d = tr.parallel_rays((0, 0, 2.0), centre, (0, -1, 0), nx, ny, (nx * VOXEL[0], ny * VOXEL[1]))
    assert o.shape == d.shape == (ny, nx, 3) and np.array_equal(d, np.broadcast_to([0.0, 0.0, 1.0], d.shape))
    assert np.allclose(o[..., 0], (ORIGIN[0] + (np.arange(nx) + 0.5) * VOXEL[0])[None, :], rtol=0, atol=1e-15)
    assert np.allclose(o[..., 1], (ORIGIN[1] + (np.arange(ny) + 0.5) * VOXEL[1])[:, None], rtol=0, atol=1e-15)
    assert np.all(o[..., 2] < ORIGIN[2])                                           # they start behind the grid
    got = tr.parallel_projection((0, 0, 2.0), centre, (0, -1, 0), nx, ny, (nx * VOXEL[0], ny * VOXEL[1]))
    ref = g.sum(axis=0) * VOXEL[2] / (VOXEL[0] * VOXEL[1] * VOXEL[2])
    assert got.shape == (ny, nx) and np.allclose(got, ref, rtol=1e-13, atol=0)
    assert np.array_equal(tr.parallel_projection((0, 0, 1), centre, (0, -1, 0), nx, ny, (nx * VOXEL[0], ny * VOXEL[1]), what="max"), g.max(axis=0))
    # an oblique view: u, v, w orthonormal, u = w x v, row 0 at +v, the plane through the centre
    o, d = tr.parallel_rays((1.0, 1.0, 1.0), centre, (0, 0, 1.0), 4, 2, 3.0)
    w = d[0, 0]
    assert np.allclose(w, np.ones(3) / np.sqrt(3.0)) and np.array_equal(d, np.broadcast_to(w, d.shape))
    u, v = o[0, 1] - o[0, 0], o[0, 0] - o[1, 0]
    assert np.allclose(np.linalg.norm(u), 3.0 / 4) and np.allclose(np.linalg.norm(v), 3.0 / 2) and v[2] > 0
    assert abs(u @ w) < 1e-14 and abs(v @ w) < 1e-14 and abs(u @ v) < 1e-14 and np.allclose(np.cross(w, v / np.linalg.norm(v)), u / np.linalg.norm(u))
    assert np.allclose(o.reshape(-1, 3).mean(axis=0) - ((o[0, 0] - centre) @ w) * w, centre)
    for bad in (dict(direction=(0, 0, 0)), dict(up=(2, 2, 2)), dict(width=0), dict(extent=0.0), dict(extent=(1.0, np.inf))):
        args = dict(direction=(1.0, 1.0, 1.0), centre=centre, up=(0, 0, 1.0), width=4, height=2, extent=3.0)
        args.update(bad)
        with pytest.raises(ValueError):
            tr.parallel_rays(**args)


@pytest.mark.parametrize("shape,n", FAMILIES)
def test_the_ray_families_hold_no_grazing_ray(shape, n):
    o, d, tr, vox = family_reference(shape, n)
    kinds = np.arange(n) % 6
    met = np.array([v["index"].size > 0 for v in vox])
    grazing = np.array([v["grazing"] for v in vox])
    print("%s: %d rays, %d meet the grid, %d grazing; voxels per ray up to %d" % (shape, n, met.sum(), grazing.sum(), max(v["index"].size for v in vox)))
    assert grazing.sum() <= 0.01 * n
    assert not met[kinds == 4].any() and met[kinds == 0].all() and met[kinds == 1].all() and met[kinds == 3].mean() > 0.9
    assert np.all(tr[kinds == 2, 0] > 0) and np.all(np.isfinite(tr[kinds == 3, 1])) and np.isinf(tr[kinds == 0, 1]).all()
