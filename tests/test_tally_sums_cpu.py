"""CPU suite of the tally sums (lt_tally_sum_axes / lt_tally_sum_columns and what is built on them): the parts that need no
device -- the radial bin table (host C++) against its NumPy restatement integer for integer, the argument handling of
Context.tally_sum, and reduce_sums_host over two gloo ranks (raw fixed-point profiles reduce to the single-process bits)."""
import os
import sys

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from light_transport_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def radial_bins_numpy(shape_xy, origin, voxel, centre, dr, nr):
    """The five operations of lt.h, one IEEE double operation each."""
    nx, ny = shape_xy
    xc = origin[0] + (np.arange(nx, dtype=np.float64) + 0.5) * voxel[0]
    yc = origin[1] + (np.arange(ny, dtype=np.float64) + 0.5) * voxel[1]
    dx, dy = xc - centre[0], yc - centre[1]
    r = np.sqrt((dx * dx)[None, :] + (dy * dy)[:, None])
    b = np.floor(r / dr)
    return np.where(b >= nr, nr, b).astype(np.int32)


def test_radial_bins_match_numpy_integer_for_integer():
    for shape, origin, voxel, centre, dr, nr in (
            ((37, 19), (-3.7, -1.9), (0.2, 0.2), (0.1, -0.3), 0.37, 6),
            ((37, 19), (-3.7, -1.9), (0.2, 0.3), (0.1, -0.3), 0.37, 300),       # no column reaches the overflow bin
            ((1, 1), (0.0, 0.0), (1.0, 1.0), (0.5, 0.5), 1.0, 1),
            ((512, 512), (-25.6, -25.6), (0.1, 0.1), (0.0, 0.0), 0.1, 362)):
        got = _lib.radial_bins(shape, origin, voxel, centre, dr, nr)
        assert got.dtype == np.int32 and got.shape == (shape[1], shape[0])
        assert np.array_equal(got, radial_bins_numpy(shape, origin, voxel, centre, dr, nr))
        assert got.min() >= 0 and got.max() <= nr


@pytest.mark.parametrize("centre", [(0.0, 0.0), (0.25, 0.25)])
def test_radial_bins_on_bin_edges(centre):
    """Voxel centres at odd multiples of 0.25, rings of width 0.25.  About (0, 0) no centre has a radius that is a multiple of
    0.25 (the sum of two odd squares is no square); about (0.25, 0.25) the offsets are multiples of 0.5 and every Pythagorean
    pair sits exactly on an edge.  Such a column belongs to the UPPER ring, and everything from nr dr on is in bin nr."""
    n, nr, dr = 16, 8, 0.25
    got = _lib.radial_bins((n, n), (-4.0, -4.0), (0.5, 0.5), centre, dr, nr)
    assert np.array_equal(got, radial_bins_numpy((n, n), (-4.0, -4.0), (0.5, 0.5), centre, dr, nr))
    # offsets in units of 0.25, exact integers: r / dr = sqrt(i^2 + j^2)
    c = np.rint((-4.0 + (np.arange(n) + 0.5) * 0.5) / 0.25).astype(np.int64)
    i, j = c - int(round(centre[0] / 0.25)), c - int(round(centre[1] / 0.25))
    q2 = (i * i)[None, :] + (j * j)[:, None]
    root = np.rint(np.sqrt(q2)).astype(np.int64)
    on_edge = root * root == q2
    assert np.array_equal(got[on_edge], np.minimum(root[on_edge], nr))          # the upper bin, never root - 1
    if centre == (0.25, 0.25):
        assert on_edge.sum() > 20 and (got[on_edge] < nr).sum() > 8
    beyond = q2 >= nr * nr
    assert beyond.any() and np.all(got[beyond] == nr) and np.all(got[~beyond] < nr)
    assert np.all(got[~beyond] == np.floor(np.sqrt(q2[~beyond].astype(np.float64))))


def test_radial_bins_errors():
    ok = dict(shape_xy=(4, 3), origin_xy=(0, 0), voxel_xy=(1, 1), centre_xy=(0, 0), dr=0.5, nr=2)
    assert _lib.radial_bins(**ok).shape == (3, 4)
    for bad in (dict(dr=0.0), dict(dr=-1.0), dict(dr=float("nan")), dict(nr=0), dict(nr=-3), dict(shape_xy=(0, 3)), dict(shape_xy=(4, -1))):
        with pytest.raises(_lib.LtError):
            _lib.radial_bins(**dict(ok, **bad))
    import ctypes as C
    assert _lib.lib().lt_radial_bins(C.c_int(2), C.c_int(2), None, None, None, C.c_double(1.0), C.c_int(1), None) == -1


def test_keep_strings_map_to_masks():
    want = {"": 0, "x": 1, "y": 2, "xy": 3, "yx": 3, "z": 4, "xz": 5, "zx": 5, "yz": 6, "zy": 6, "Z": 4, "Yx": 3}
    for k, m in want.items():
        assert _lib.keep_mask(k) == m
    for m in range(7):
        assert _lib.keep_mask(m) == m and _lib.keep_mask(np.int32(m)) == m
    for bad in ("xyz", "zyx", "xx", "w", "x,y", " z", 7, 8, -1, None, 1.0, True, ("x",)):
        with pytest.raises(ValueError):
            _lib.keep_mask(bad)
    shape = (5, 4, 3)        # nz, ny, nx
    assert [_lib.kept_shape(m, shape) for m in range(7)] == [(), (3,), (4,), (4, 3), (5,), (5, 3), (5, 4)]


def test_new_entry_points_are_listed():
    for s in ("lt_tally_sum_axes", "lt_tally_sum_columns", "lt_radial_bins", "lt_write_grid"):
        assert s in _lib.SYMBOLS and hasattr(_lib.lib(), s)


def _worker(rank, world, port, n_photons, out_dir):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from light_transport_amd.distributed import reduce_sums_host, shard_range
    from tests import scenes as S
    off, cnt = shard_range(n_photons, rank, world)
    _, fx, _ = S.two_layer(n=24).oracle().run(cnt, seed=21, photon_offset=off, want_fx=True, want_f64=False)
    mine = [fx.sum(axis=(1, 2), dtype=np.uint64), fx.sum(axis=0, dtype=np.uint64), fx.sum(dtype=np.uint64),
            fx.sum(axis=(1, 2), dtype=np.uint64).astype(np.float64) * 2.0 ** -40]
    keep = [a.copy() for a in mine]
    red = reduce_sums_host(mine, dst=0)
    assert all(np.array_equal(a, b) for a, b in zip(mine, keep))            # the inputs are left alone
    assert [a.dtype for a in red] == [a.dtype for a in mine] and [a.shape for a in red] == [a.shape for a in mine]
    allred = reduce_sums_host(mine[:1])
    if rank == 0:
        np.savez(os.path.join(out_dir, "sums.npz"), z=red[0], xy=red[1], total=red[2], zf=red[3], z_all=allred[0])
    else:
        np.save(os.path.join(out_dir, "z_all_rank1.npy"), allred[0])
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_gloo_reduce_of_raw_profiles(tmp_path):
    sys.path.insert(0, ROOT)
    from tests import scenes as S
    n = 3001
    port = 31500 + (os.getpid() % 2000)
    mp.spawn(_worker, args=(2, port, n, str(tmp_path)), nprocs=2, join=True)
    got = np.load(os.path.join(str(tmp_path), "sums.npz"))
    _, fx, _ = S.two_layer(n=24).oracle().run(n, seed=21, want_fx=True, want_f64=False)
    z = fx.sum(axis=(1, 2), dtype=np.uint64)
    assert got["z"].dtype == np.uint64 and np.array_equal(got["z"], z)          # bit for bit
    assert np.array_equal(got["xy"], fx.sum(axis=0, dtype=np.uint64))
    assert got["total"].shape == () and got["total"] == fx.sum(dtype=np.uint64)
    np.testing.assert_allclose(got["zf"], z.astype(np.float64) * 2.0 ** -40, rtol=4e-16)
    assert np.array_equal(got["z_all"], z)
    assert np.array_equal(np.load(os.path.join(str(tmp_path), "z_all_rank1.npy")), z)       # all-reduce: every rank
    assert z.sum() > 0
