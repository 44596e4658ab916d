"""CPU suite of the results by region: the four label entry points exist at every layer; label_sums_numpy / histogram_numpy
restate lt_tally_label_sums / lt_tally_histogram in NumPy (the GPU suite imports them as its reference); label_volume of a
LayeredSlab against hand-built arrays; and the PhotonTracer methods on top -- set_regions, region_totals, dose_volume,
run_batches(labels=True), region_totals_error -- driven by a stub context whose methods are those restatements."""
import ctypes
import os
import re

import numpy as np
import pytest

import light_transport_amd as lt
from light_transport_amd import _lib
from light_transport_amd.src import photon_tracing as PT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("lt_set_labels", "lt_labels_info", "lt_tally_label_sums", "lt_tally_histogram")
NONE = 255


def as_weight(g):
    """A raw tally as lt_read_grid_f64 converts it: u64 -> (double)raw * 2^-40 (one rounding), floats widened."""
    return g.astype(np.float64) * 2.0 ** -40 if g.dtype == np.uint64 else g.astype(np.float64)


def _flat(g, labels):
    lab = np.zeros(g.size, dtype=np.uint8) if labels is None else np.asarray(labels, dtype=np.uint8).ravel()
    return g.ravel(), lab


def label_sums_numpy(g, labels, n_labels, dtype):
    """The definition of lt_tally_label_sums on a raw tally g [nz, ny, nx] and a label volume (None: label 0 everywhere):
    dict of [n_labels] arrays -- ``sum`` of the label's voxels in ``dtype`` (uint64: the integer sum; float64), ``voxels``,
    ``filled``, ``peak`` (the largest voxel, in g's own dtype) and ``peak_index`` (the lowest flat index holding it, -1 for a
    label without voxels)."""
    v, lab = _flat(g, labels)
    keep = lab < n_labels
    out = dict(sum=np.zeros(n_labels, dtype=dtype), voxels=np.zeros(n_labels, dtype=np.uint64), filled=np.zeros(n_labels, dtype=np.uint64),
               peak=np.zeros(n_labels, dtype=g.dtype), peak_index=np.full(n_labels, -1, dtype=np.int64))
    np.add.at(out["sum"], lab[keep], v[keep].astype(dtype))
    np.add.at(out["voxels"], lab[keep], np.uint64(1))
    np.add.at(out["filled"], lab[keep & (v != 0)], np.uint64(1))
    for l in range(n_labels):
        idx = np.flatnonzero(lab == l)
        if idx.size:
            out["peak"][l] = v[idx].max()
            out["peak_index"][l] = idx[np.argmax(v[idx])]          # argmax: the first of equal maxima
    return out


def histogram_numpy(g, labels, n_labels, edges, dtype):
    """The definition of lt_tally_histogram: (voxels uint64, sums in ``dtype``) [n_labels, len(edges) + 1]; the class of a
    voxel is the number of edges <= its value as weight."""
    v, lab = _flat(g, labels)
    keep = lab < n_labels
    cls = np.searchsorted(np.asarray(edges, dtype=np.float64), as_weight(v), side="right")
    vox = np.zeros((n_labels, len(edges) + 1), dtype=np.uint64)
    w = np.zeros((n_labels, len(edges) + 1), dtype=dtype)
    np.add.at(vox, (lab[keep], cls[keep]), np.uint64(1))
    np.add.at(w, (lab[keep], cls[keep]), v[keep].astype(dtype))
    return vox, w


class StubContext:
    """Stands where the Context would: a raw grid [nz, ny, nx], labels, and the label calls as the NumPy restatements; a launch
    adds the next of ``batches`` to the grid; every call is recorded."""

    def __init__(self, grid, batches=()):
        self.grid, self.batches, self.calls, self.on = grid.copy(), list(batches), [], False
        self.labels, self.n_labels = None, 0

    def _acc(self):
        return np.uint64 if self.grid.dtype == np.uint64 else np.float64

    def set_labels(self, labels, n_labels=None):
        self.calls.append(("set_labels", None if labels is None else labels.shape, n_labels))
        self.labels = labels
        self.n_labels = 0 if labels is None else (int(labels[labels != NONE].max()) + 1 if n_labels is None else n_labels)

    def labels_info(self):
        return self.n_labels

    def tally_label_sums(self, raw=False):
        self.calls.append(("tally_label_sums", raw))
        r = label_sums_numpy(self.grid, self.labels, max(self.n_labels, 1), self._acc())
        res = dict(weight=as_weight(r["sum"]), voxels=r["voxels"], filled=r["filled"], peak=as_weight(r["peak"]), peak_index=r["peak_index"])
        if raw:
            res["raw"] = r["sum"]
        return res

    def tally_histogram(self, edges, raw=False):
        self.calls.append(("tally_histogram", tuple(np.asarray(edges).tolist()), raw))
        vox, w = histogram_numpy(self.grid, self.labels, max(self.n_labels, 1), edges, self._acc())
        return vox, (w if raw else as_weight(w))

    def stats_enabled(self):
        return self.on

    def stats_enable(self, on=True):
        self.on = on

    def launch(self, n, seed=0, photon_offset=0, f32_walk=False):
        self.calls.append(("launch", n, seed, photon_offset, f32_walk))
        self.grid = self.grid + self.batches.pop(0)

    def stats_fold(self):
        self.calls.append(("stats_fold",))

    def sync(self):
        pass


SHAPE = (12, 8, 6)            # (nx, ny, nz)


def stub_tracer(grid, dtype="f64", quantity="absorbed", photons=1000, batches=(), geometry=None):
    tr = PT.PhotonTracer(ctx=StubContext(grid, batches))
    tr.grid = PT.VoxelGrid(SHAPE, (-1.5, 2.0, 0.25), (0.1, 0.2, 0.3), dtype=dtype)
    tr.quantity, tr.photons, tr.geometry = quantity, photons, geometry
    return tr


def whole_weights(seed=5):
    """float64 [nz, ny, nx] of whole numbers (sums are exact), a third of them zero."""
    rs = np.random.RandomState(seed)
    g = rs.randint(0, 1000, size=SHAPE[::-1]).astype(np.float64)
    g[rs.random_sample(g.shape) < 0.33] = 0.0
    return g


def three_labels(seed=6):
    rs = np.random.RandomState(seed)
    lab = rs.randint(0, 3, size=SHAPE[::-1]).astype(np.uint8)
    lab[rs.random_sample(lab.shape) < 0.2] = NONE
    return lab


def test_the_symbols_are_declared_exported_and_bound():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lt.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lt_[a-z0-9_]+)\s*\(", txt))
    assert os.path.exists(lt.LIB_PATH), "liblt_hip.so not built: run __graft_entry__.build()"
    for name in NEW_SYMBOLS:
        assert name in declared, "%s is not declared in lt.h" % name
        assert getattr(_lib.lib(), name) is not None                   # resolves in the built library
        assert name in _lib.SYMBOLS and name in _lib.PROTOTYPES
    assert re.search(r"#define\s+LT_LABEL_NONE\s+255\b", txt) and _lib.LABEL_NONE == 255
    assert re.search(r"#define\s+LT_ABI_VERSION\s+3\b", txt) and ctypes.CDLL(lt.LIB_PATH).lt_abi_version() == 3
    for name in ("set_labels", "labels_info", "tally_label_sums", "tally_histogram"):
        assert callable(getattr(_lib.Context, name))
    for name in ("set_regions", "region_totals", "dose_volume", "region_totals_error"):
        assert callable(getattr(PT.PhotonTracer, name))
    assert callable(PT.label_volume)


def test_the_restatements_on_a_grid_worked_by_hand():
    g = np.array([[[0, 5, 5, 2], [7, 0, 1, 7]]], dtype=np.uint64) << np.uint64(40)            # weights 0 5 5 2 / 7 0 1 7
    lab = np.array([[[0, 0, 0, 1], [1, NONE, 2, 1]]], dtype=np.uint8)
    r = label_sums_numpy(g, lab, 4, np.uint64)
    assert np.array_equal(as_weight(r["sum"]), [10, 16, 1, 0])
    assert np.array_equal(r["voxels"], [3, 3, 1, 0]) and np.array_equal(r["filled"], [2, 3, 1, 0])
    assert np.array_equal(as_weight(r["peak"]), [5, 7, 1, 0]) and np.array_equal(r["peak_index"], [1, 4, 6, -1])      # lowest index of 5 and of 7
    vox, w = histogram_numpy(g, lab, 4, [0.0, 2.0, 7.0], np.uint64)                           # an edge ON a value: <=
    assert np.array_equal(vox, [[0, 1, 2, 0], [0, 0, 1, 2], [0, 1, 0, 0], [0, 0, 0, 0]])
    assert np.array_equal(as_weight(w), [[0, 0, 10, 0], [0, 0, 2, 14], [0, 1, 0, 0], [0, 0, 0, 0]])
    vox1, _ = histogram_numpy(g, None, 1, [1.5], np.uint64)                                   # no labels: one label, nobody left out
    assert np.array_equal(vox1, [[3, 5]])
    rf = label_sums_numpy(np.zeros((1, 1, 3)), np.array([[[1, 1, NONE]]], dtype=np.uint8), 2, np.float64)
    assert np.array_equal(rf["peak_index"], [-1, 0]) and np.array_equal(rf["voxels"], [0, 2])  # all zero: the first voxel


def test_label_volume_of_a_slab():
    media = [PT.OpticalMedium(0.1, 10.0, 0.9)] * 3
    slab = PT.LayeredSlab(media, [0.5, 1.0, 0.75], z0=1.0)              # bounds 1, 1.5, 2.5, 3.25
    grid = PT.VoxelGrid((3, 2, 12), (0.0, 0.0, 0.25), (1.0, 1.0, 0.25))  # centres 0.375, 0.625, ..., 3.125 -- 1.125 .. ; none on a bound
    lab = PT.label_volume(None, slab, grid)
    assert lab.dtype == np.uint8 and lab.shape == (12, 2, 3) and lab.flags["C_CONTIGUOUS"]
    assert np.array_equal(lab[:, 0, 0], [NONE, NONE, NONE, 0, 0, 1, 1, 1, 1, 2, 2, 2])
    assert np.all(lab == lab[:, :1, :1])
    # centres exactly on bounds: z = 1.0 opens layer 0, 1.5 belongs to layer 1 (lo <= z < hi), 3.25 is outside
    grid2 = PT.VoxelGrid((1, 1, 6), (0.0, 0.0, 0.25), (1.0, 1.0, 0.5))   # centres 0.5, 1.0, 1.5, 2.0, 2.5, 3.0
    assert np.array_equal(PT.label_volume(None, slab, grid2).ravel(), [NONE, 0, 1, 1, 2, 2])
    grid3 = PT.VoxelGrid((1, 1, 2), (0.0, 0.0, 2.75), (1.0, 1.0, 0.5))   # centres 3.0, 3.5
    assert np.array_equal(PT.label_volume(None, slab, grid3).ravel(), [2, NONE])
    # an infinite last layer takes everything below; a grid that starts above the slab: those centres are left out
    inf = PT.LayeredSlab(media[:2], [0.3, np.inf], z0=0.0)
    grid4 = PT.VoxelGrid((2, 2, 5), (0.0, 0.0, -0.4), (1.0, 1.0, 0.2))   # centres -0.3, -0.1, 0.1, 0.3, 0.5
    assert np.array_equal(PT.label_volume(None, inf, grid4)[:, 1, 1], [NONE, NONE, 0, 1, 1])
    with pytest.raises(TypeError):
        PT.label_volume(None, object(), grid)
    with pytest.raises(ValueError):
        PT.label_volume(_NoMesh(), PT.MeshVolume(media), grid)


class _NoMesh:
    _mesh = None


def test_set_regions_passes_the_geometrys_labels_or_the_callers():
    media = [PT.OpticalMedium(0.1, 10.0, 0.9)] * 2
    slab = PT.LayeredSlab(media, [0.9, np.inf], z0=0.25)                 # voxel centres 0.4, 0.7, 1.0, 1.3, ...: two in layer 0
    tr = stub_tracer(whole_weights(), geometry=slab)
    lab = tr.set_regions()
    assert tr.ctx.calls == [("set_labels", (6, 8, 12), 2)]
    assert np.array_equal(lab[:, 0, 0], [0, 0, 0, 1, 1, 1]) and tr.ctx.labels is lab
    mine = three_labels()
    assert tr.set_regions(mine) is not None and tr.ctx.calls[-1] == ("set_labels", (6, 8, 12), None) and tr.ctx.n_labels == 3


@pytest.mark.parametrize("quantity", ["absorbed", "fluence"])
def test_region_totals_normalise_and_place_the_peak(quantity):
    g, lab = whole_weights(), three_labels()
    tr = stub_tracer(g, quantity=quantity, photons=4000)
    tr.set_regions(lab)
    tr.ctx.calls.clear()
    r = tr.region_totals()
    assert tr.ctx.calls == [("tally_label_sums", False)]
    ref = label_sums_numpy(g, lab, 3, np.float64)
    assert np.array_equal(r["weight"], ref["sum"]) and np.array_equal(r["voxels"], ref["voxels"]) and np.array_equal(r["filled"], ref["filled"])
    assert np.array_equal(r["share"], ref["sum"] / 4000.0)
    dv = 0.1 * 0.2 * 0.3
    if quantity == "absorbed":
        assert np.array_equal(r["total"], ref["sum"]) and np.array_equal(r["peak"], ref["peak"])
    else:
        assert np.array_equal(r["total"], ref["sum"] / (ref["voxels"].astype(np.float64) * (tr.grid.voxel_volume * 4000.0)))
        assert np.array_equal(r["peak"], ref["peak"] / (1.0 * (tr.grid.voxel_volume * 4000.0))) and abs(tr.grid.voxel_volume - dv) < 1e-15
    for l in range(3):
        z, y, x = np.unravel_index(ref["peak_index"][l], g.shape)
        assert g[z, y, x] == ref["peak"][l] and lab[z, y, x] == l
        assert np.array_equal(r["peak_position"][l], [-1.5 + 0.1 * (x + 0.5), 2.0 + 0.2 * (y + 0.5), 0.25 + 0.3 * (z + 0.5)])
    # a label without voxels: index -1, no position
    tr.ctx.set_labels(lab, 5)
    r5 = tr.region_totals()
    assert np.array_equal(r5["peak_index"][3:], [-1, -1]) and np.all(np.isnan(r5["peak_position"][3:])) and np.all(r5["voxels"][3:] == 0)


def test_dose_volume_is_the_reverse_cumulative_share():
    g, lab = whole_weights(seed=8), three_labels(seed=9)
    tr = stub_tracer(g)
    tr.set_regions(lab)
    edges = [0.0, 100.0, 500.0, float(g.max()), 2000.0]
    dv = tr.dose_volume(edges)
    assert tr.ctx.calls[-1] == ("tally_histogram", tuple(edges), False)
    assert dv["volume"].shape == dv["weight"].shape == (3, 5)
    for l in range(3):
        mine = g[lab == l]
        for k, e in enumerate(edges):
            assert dv["volume"][l, k] == np.count_nonzero(mine >= e) / mine.size
            assert dv["weight"][l, k] == mine[mine >= e].sum() / mine.sum()          # whole numbers: exact sums, one division
    assert np.all(dv["volume"][:, 0] == 1.0) and np.all(dv["volume"][:, 4] == 0.0) and np.any(dv["volume"][:, 3] > 0)
    # fluence: the edges are fluences, a voxel's weight is fluence x dV x photons
    tf = stub_tracer(g, quantity="fluence", photons=250)
    tf.set_regions(lab)
    scale = tf.grid.voxel_volume * 250.0
    dvf = tf.dose_volume(np.array([100.0, 500.0]) / scale)
    assert np.allclose(tf.ctx.calls[-1][1], (100.0, 500.0), rtol=1e-15)
    assert np.allclose(dvf["volume"], dv["volume"][:, 1:3], atol=0.02)
    # a label without voxels: NaN
    tr.ctx.set_labels(lab, 4)
    assert np.all(np.isnan(tr.dose_volume(edges)["volume"][3]))


@pytest.mark.parametrize("dtype", ["f64", "u64fx"])
def test_run_batches_keeps_the_moments_of_the_label_totals(dtype):
    rs = np.random.RandomState(11)
    lab = three_labels()
    if dtype == "u64fx":
        start = np.zeros(SHAPE[::-1], dtype=np.uint64)
        batches = [rs.randint(0, 2 ** 40, size=start.shape, dtype=np.uint64) for _ in range(4)]
    else:
        start = np.zeros(SHAPE[::-1])
        batches = [rs.randint(0, 1000, size=start.shape).astype(np.float64) for _ in range(4)]
    acc = np.uint64 if dtype == "u64fx" else np.float64
    tr = stub_tracer(start, dtype=dtype, photons=0, batches=batches)
    tr.set_regions(lab)
    with pytest.raises(ValueError):
        tr.region_totals_error()
    tr.ctx.calls.clear()
    tr.run_batches(4000, 4, seed=3, labels=True)
    per_batch = [as_weight(label_sums_numpy(d, lab, 3, acc)["sum"]) for d in batches]
    s1, s2 = sum(per_batch), sum(d * d for d in per_batch)
    err = tr.region_totals_error()
    assert err.shape == (3,) and np.array_equal(err, _lib.relative_error(4, s1, s2)) and np.all(err > 0)
    reads = [c for c in tr.ctx.calls if c[0] == "tally_label_sums"]
    assert reads == [("tally_label_sums", dtype == "u64fx")] * 5                      # before the first batch and after every fold
    assert [c[0] for c in tr.ctx.calls].count("launch") == 4 and tr.photons == 4000
    # without labels=True nothing of the kind is asked for
    tr2 = stub_tracer(start, dtype=dtype, photons=0, batches=[b.copy() for b in batches])
    tr2.run_batches(4000, 4)
    assert not [c for c in tr2.ctx.calls if c[0] == "tally_label_sums"]
