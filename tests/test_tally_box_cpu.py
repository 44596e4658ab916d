"""CPU suite of the box read-out of the tally: lt_tally_box exists at every layer, box_shape and the edges of region() are
right where the bin divides the box, where it does not and where it exceeds it, and PhotonTracer.region / slice / coarse /
run_batches(regions=) ask the context for the right boxes -- driven by a stub context whose tally_box is the NumPy restatement
(box_sums_numpy, which the GPU suite uses as its reference too)."""
import ctypes
import os
import re

import numpy as np
import pytest

import light_transport_amd as lt
from light_transport_amd import _lib
from light_transport_amd.src import photon_tracing as PT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def box_sums_numpy(g, lo, size, bin, dtype):
    """The definition of lt_tally_box on an array g [nz, ny, nx]: the box cut out, converted to ``dtype`` (uint64 or float64), and
    along every axis the blocks of ``bin`` voxels added up, the last one clipped.  lo, size, bin in x, y, z order."""
    sub = g[lo[2]:lo[2] + size[2], lo[1]:lo[1] + size[1], lo[0]:lo[0] + size[0]].astype(dtype)
    assert sub.shape == tuple(size[::-1]), "the box leaves the array"
    for axis, a in ((0, 2), (1, 1), (2, 0)):
        sub = np.add.reduceat(sub, np.arange(0, size[a], bin[a]), axis=axis, dtype=dtype)
    return sub


def block_voxels(size, bin):
    """[oz, oy, ox]: the grid voxels in every output voxel, by counting."""
    return box_sums_numpy(np.ones(tuple(size[::-1]), dtype=np.uint64), (0, 0, 0), size, bin, np.uint64).astype(np.float64)


class StubContext:
    """Stands where the Context would.  Holds a grid [nz, ny, nx]; a launch adds the next of ``batches`` to it; every call is
    recorded by name and arguments."""

    def __init__(self, grid, batches=()):
        self.grid, self.batches, self.calls, self.on = grid.copy(), list(batches), [], False

    def _note(self, name, *args):
        self.calls.append((name,) + args)

    def tally_box(self, lo, size, bin=(1, 1, 1), raw=False):
        self._note("tally_box", tuple(lo), tuple(size), tuple(bin), raw)
        if raw:
            return box_sums_numpy(self.grid, lo, size, bin, np.uint64)
        w = box_sums_numpy(self.grid, lo, size, bin, np.uint64 if self.grid.dtype == np.uint64 else np.float64)
        return w.astype(np.float64) * 2.0 ** -40 if self.grid.dtype == np.uint64 else w

    def tally_sum(self, keep, raw=False):
        self._note("tally_sum", keep, raw)
        axes = tuple(ax for ax, bit in ((0, 4), (1, 2), (2, 1)) if not keep & bit)
        return self.grid.sum(axis=axes)

    def stats_enabled(self):
        self._note("stats_enabled")
        return self.on

    def stats_enable(self, on=True):
        self._note("stats_enable", on)
        self.on = on

    def launch(self, n, seed=0, photon_offset=0, f32_walk=False):
        self._note("launch", n, seed, photon_offset, f32_walk)
        self.grid = self.grid + self.batches.pop(0)

    def stats_fold(self):
        self._note("stats_fold")

    def sync(self):
        self._note("sync")


def stub_tracer(grid, shape, dtype="f64", quantity="absorbed", photons=1000, batches=()):
    tr = PT.PhotonTracer(ctx=StubContext(grid, batches))
    tr.grid = PT.VoxelGrid(shape, (-1.5, 2.0, 0.25), (0.1, 0.2, 0.3), dtype=dtype)
    tr.quantity, tr.photons = quantity, photons
    return tr


def random_weights(shape, seed=5):
    nx, ny, nz = shape
    return np.random.RandomState(seed).randint(0, 1000, size=(nz, ny, nx)).astype(np.float64)     # whole numbers: sums are exact


def test_the_symbol_is_declared_exported_and_bound():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lt.h")).read(), flags=re.S)
    assert "lt_tally_box" in set(re.findall(r"\b(lt_[a-z0-9_]+)\s*\(", txt)), "lt_tally_box is not declared in lt.h"
    assert os.path.exists(lt.LIB_PATH), "liblt_hip.so not built: run __graft_entry__.build()"
    assert _lib.lib().lt_tally_box is not None                        # resolves in the built library
    assert "lt_tally_box" in _lib.SYMBOLS and "lt_tally_box" in _lib.PROTOTYPES
    assert re.search(r"#define\s+LT_ABI_VERSION\s+3\b", txt) and ctypes.CDLL(lt.LIB_PATH).lt_abi_version() == 3
    assert callable(_lib.box_shape) and callable(_lib.Context.tally_box)
    for name in ("region", "slice", "coarse", "region_error"):
        assert callable(getattr(PT.PhotonTracer, name))


@pytest.mark.parametrize("size,bin,shape", [
    ((12, 8, 6), (1, 1, 1), (6, 8, 12)), ((12, 8, 6), (4, 2, 3), (2, 4, 3)),          # dividing
    ((13, 9, 7), (4, 2, 3), (3, 5, 4)), ((7, 7, 7), (3, 5, 7), (1, 2, 3)),           # not dividing: a clipped last block
    ((5, 3, 2), (9, 3, 100), (1, 1, 1)), ((1, 1, 1), (2, 2, 2), (1, 1, 1))])         # bins beyond the box
def test_box_shape(size, bin, shape):
    assert _lib.box_shape(size, bin) == shape
    assert box_sums_numpy(np.zeros(size[::-1]), (0, 0, 0), size, bin, np.float64).shape == shape


def test_box_shape_and_triples_reject_nonsense():
    assert _lib.box_shape((4, 5, 6)) == (6, 5, 4)
    for size, bin in (((4, 5), (1, 1, 1)), ((4, 5, 6), 2), ((4, 5, 0), (1, 1, 1)), ((4, 5, 6), (1, 0, 1)), ((4.0, 5, 6), (1, 1, 1))):
        with pytest.raises(ValueError):
            _lib.box_shape(size, bin)


@pytest.mark.parametrize("lo,size,bin", [((0, 0, 0), (12, 8, 6), (4, 2, 3)), ((3, 1, 2), (7, 6, 3), (3, 4, 2)), ((2, 0, 1), (5, 3, 2), (9, 3, 100))])
def test_region_passes_the_box_on_and_gives_edges_in_scene_units(lo, size, bin):
    shape = (12, 8, 6)
    w = random_weights(shape)
    tr = stub_tracer(w, shape)
    got, (ze, ye, xe) = tr.region(lo, size, bin)
    assert tr.ctx.calls == [("tally_box", lo, size, bin, False)]
    assert np.array_equal(got, box_sums_numpy(w, lo, size, bin, np.float64))
    org, vox = tr.grid.origin, tr.grid.voxel
    for a, e in ((0, xe), (1, ye), (2, ze)):
        idx = [lo[a] + min(k * bin[a], size[a]) for k in range(-(-size[a] // bin[a]) + 1)]      # the last edge: the box's end
        assert e.shape == (got.shape[2 - a] + 1,)
        assert np.array_equal(e, np.array([org[a] + vox[a] * i for i in idx]))
        assert e[0] == org[a] + vox[a] * lo[a] and e[-1] == org[a] + vox[a] * (lo[a] + size[a])


def test_slice_and_coarse_ask_for_the_right_boxes():
    shape = (12, 8, 6)
    w = random_weights(shape)
    tr = stub_tracer(w, shape)
    for axis, number, index, box, ref in (("y", 1, 5, ((0, 5, 0), (12, 1, 6), (1, 1, 1)), w[:, 5, :]),
                                          ("x", 2, 11, ((11, 0, 0), (1, 8, 6), (1, 1, 1)), w[:, :, 11]),
                                          ("z", 0, 0, ((0, 0, 0), (12, 8, 1), (1, 1, 1)), w[0])):
        tr.ctx.calls.clear()
        got = tr.slice(axis, index)
        assert tr.ctx.calls == [("tally_box",) + box + (False,)] and np.array_equal(got, ref)
        assert np.array_equal(tr.slice(number, index), ref)
    tr.ctx.calls.clear()
    got = tr.slice("y", 3, bin=4)
    assert tr.ctx.calls == [("tally_box", (0, 3, 0), (12, 1, 6), (4, 1, 4), False)]
    assert np.array_equal(got, box_sums_numpy(w, (0, 3, 0), (12, 1, 6), (4, 1, 4), np.float64)[:, 0, :]) and got.shape == (2, 3)
    assert tr.slice("x", 2, bin=(3, 5)).shape == (2, 3)            # (by, bz) = (3, 5): [ceil(6 / 5), ceil(8 / 3)]
    assert tr.ctx.calls[-1] == ("tally_box", (2, 0, 0), (1, 8, 6), (1, 3, 5), False)
    tr.ctx.calls.clear()
    assert np.array_equal(tr.coarse(4), box_sums_numpy(w, (0, 0, 0), shape, (4, 4, 4), np.float64))
    assert np.array_equal(tr.coarse((5, 3, 2)), box_sums_numpy(w, (0, 0, 0), shape, (5, 3, 2), np.float64))
    assert tr.ctx.calls == [("tally_box", (0, 0, 0), shape, (4, 4, 4), False), ("tally_box", (0, 0, 0), shape, (5, 3, 2), False)]
    for bad in (lambda: tr.slice("w", 0), lambda: tr.slice("y", 0, bin=(1, 2, 3)), lambda: tr.coarse((1, 2))):
        with pytest.raises(ValueError):
            bad()


def test_fluence_region_is_the_mean_over_the_clipped_blocks():
    """The reference divides every voxel by dV x photons first and takes the mean of each block on the host; region() divides
    the block's sum (exact here: whole-number weights) once by (voxels x dV x photons).  The reference rounds every voxel's
    quotient (2^-53 relative each) and the n - 1 additions of a block of n non-negative terms, and both round their product and
    final division: (n + 4) 2^-52 ref, the bound the tally-sums suite derives for its fluence means."""
    shape, lo, size, bin = (13, 9, 7), (1, 2, 0), (11, 7, 7), (4, 3, 5)
    w = random_weights(shape, seed=6)
    tr = stub_tracer(w, shape, quantity="fluence", photons=4096)
    got, _ = tr.region(lo, size, bin)
    fl = w / (tr.grid.voxel_volume * 4096.0)                                     # what fluence() would return
    n = block_voxels(size, bin)
    assert n.min() == 3 * 1 * 2 and n.max() == 4 * 3 * 5                         # clipped: x 4 + 4 + 3, y 3 + 3 + 1, z 5 + 2
    ref = box_sums_numpy(fl, lo, size, bin, np.float64) / n
    assert got.shape == ref.shape == (2, 3, 3) and np.all(np.abs(got - ref) <= (n + 4) * 2.0 ** -52 * ref) and ref.min() > 0
    whole = tr.coarse((20, 20, 20))                                              # one block: the mean over the grid
    assert whole.shape == (1, 1, 1) and abs(whole[0, 0, 0] - fl.mean()) <= (w.size + 4) * 2.0 ** -52 * fl.mean()


@pytest.mark.parametrize("dtype", ["f64", "u64fx"])
def test_run_batches_keeps_the_moments_of_a_region(dtype):
    shape, box = (12, 8, 6), ((1, 0, 2), (10, 8, 3), (4, 3, 2))
    rs = np.random.RandomState(11)
    if dtype == "u64fx":
        start = np.zeros((6, 8, 12), dtype=np.uint64)
        batches = [rs.randint(0, 2 ** 40, size=start.shape, dtype=np.uint64) for _ in range(4)]
        weight = lambda d: box_sums_numpy(d, *box, np.uint64).astype(np.float64) * 2.0 ** -40      # noqa: E731
    else:
        start = np.zeros((6, 8, 12))
        batches = [rs.randint(0, 1000, size=start.shape).astype(np.float64) for _ in range(4)]
        weight = lambda d: box_sums_numpy(d, *box, np.float64)                                      # noqa: E731
    tr = stub_tracer(start, shape, dtype=dtype, photons=0, batches=batches)
    with pytest.raises(ValueError):
        tr.region_error(*box)
    tr.run_batches(4000, 4, seed=3, regions=(box,))
    per_batch = [weight(d) for d in batches]
    s1, s2 = sum(per_batch), sum(d * d for d in per_batch)
    err = tr.region_error(*box)
    assert err.shape == _lib.box_shape(box[1], box[2]) == (2, 3, 3)
    assert np.array_equal(err, _lib.relative_error(4, s1, s2)) and np.all(err > 0)
    reads = [c for c in tr.ctx.calls if c[0] == "tally_box"]
    assert reads == [("tally_box",) + box + (dtype == "u64fx",)] * 5                # before the first batch and after every fold
    with pytest.raises(ValueError):
        tr.region_error(box[0], box[1], (1, 1, 1))                                  # another bin was not asked for


def test_run_batches_without_regions_calls_the_context_as_before():
    shape = (12, 8, 6)
    batches = [np.ones((6, 8, 12)) for _ in range(2)]
    tr = stub_tracer(np.zeros((6, 8, 12)), shape, photons=0, batches=batches)
    tr.run_batches(200, 2, seed=7, photon_offset=50, profiles=("z",))
    assert tr.ctx.calls == [("stats_enabled",), ("stats_enable", True), ("tally_sum", 4, False),
                            ("launch", 100, 7, 50, False), ("stats_fold",), ("tally_sum", 4, False),
                            ("launch", 100, 7, 150, False), ("stats_fold",), ("tally_sum", 4, False), ("sync",)]
    assert tr.photons == 200 and np.array_equal(tr.profile_error("z"), np.zeros(6))      # equal batches: no spread
    tr2 = stub_tracer(np.zeros((6, 8, 12)), shape, photons=0, batches=[np.ones((6, 8, 12)) for _ in range(2)])
    tr2.run_batches(200, 2)
    assert [c[0] for c in tr2.ctx.calls] == ["stats_enabled", "stats_enable", "launch", "stats_fold", "launch", "stats_fold", "sync"]
