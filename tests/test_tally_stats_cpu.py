"""CPU suite of the batch statistics of the tally: the six lt_stats_* entry points exist at every layer, the NumPy restatement
of the estimator (_lib.relative_error) gives the values the definition demands, and PhotonTracer.run_batches rejects unequal
batches before it touches a device."""
import ctypes
import os
import re

import numpy as np
import pytest

import light_transport_amd as lt
from light_transport_amd import _lib
from light_transport_amd.src import photon_tracing as PT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["lt_stats_enable", "lt_stats_fold", "lt_stats_batches", "lt_stats_read_m2", "lt_stats_read_relerr", "lt_stats_summary"]


def test_the_six_symbols_are_declared_exported_and_bound():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lt.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lt_[a-z0-9_]+)\s*\(", txt))
    assert os.path.exists(lt.LIB_PATH), "liblt_hip.so not built: run __graft_entry__.build()"
    L = ctypes.CDLL(lt.LIB_PATH)
    for n in NAMES:
        assert n in declared, n + " is not declared in lt.h"
        assert hasattr(L, n), n + " is not exported"
        assert n in _lib.SYMBOLS and n in _lib.PROTOTYPES, n + " is not bound in _lib"
    assert re.search(r"#define\s+LT_ABI_VERSION\s+3\b", txt) and L.lt_abi_version() == 3
    for name in ("stats_enable", "stats_fold", "stats_batches", "stats_m2", "stats_relerr", "stats_summary"):
        assert callable(getattr(_lib.Context, name))
    for name in ("run_batches", "relative_error", "error_summary", "profile_error"):
        assert callable(getattr(PT.PhotonTracer, name))


def test_relative_error_of_equal_batches_is_zero():
    for n in (2, 5, 8):
        x = np.array([0.25, 3.0, 1e-7, 12345.0])         # every batch adds x: s1 = n x, m2 = n x^2, both exact for these n x
        r = _lib.relative_error(n, n * x, n * (x * x))
        assert r.dtype == np.float64 and np.array_equal(r, np.zeros(4))


@pytest.mark.parametrize("n", [2, 8])
def test_relative_error_is_exactly_one_where_one_batch_contributed(n):
    x = np.array([1.0, 0.3, 7.25e-9, 2.0 ** 24])
    r = _lib.relative_error(n, x, x * x)                 # q = n x^2 / x^2 = n, v = n - 1, R = sqrt(1): no rounding anywhere
    assert np.array_equal(r, np.ones(4))


def test_relative_error_is_nan_without_weight_and_keeps_the_shape():
    s1 = np.array([[0.0, 2.0], [0.0, 0.0]])
    m2 = np.array([[0.0, 2.5], [1.0, 0.0]])
    r = _lib.relative_error(4, s1, m2)
    assert r.shape == (2, 2) and np.array_equal(np.isnan(r), s1 == 0.0)
    assert r[0, 1] == np.sqrt(((4 * 2.5) / 4.0 - 1.0) / 3.0)
    assert np.isnan(_lib.relative_error(2, 0.0, 0.0))    # scalars too


def test_relative_error_is_zero_where_rounding_leaves_q_below_one():
    """Three equal batches of x = 1.3, summed as a fold sums them: the roundings of s1 and m2 do not follow one another and
    q = 3 m2 / s1^2 comes out as 1 - 2^-53 -- a variance that would be negative.  R is 0, not NaN."""
    x = 1.3
    s1, m2 = (x + x) + x, (x * x + x * x) + x * x
    q = (3.0 * m2) / (s1 * s1)
    assert q < 1.0
    assert _lib.relative_error(3, s1, m2) == 0.0
    assert _lib.relative_error(3, np.array([s1, 1.0]), np.array([m2, 1.0 / 3.0 - 1e-9]))[1] == 0.0


class _NoDevice:
    """Stands where the Context would: any use of it is a device call the test forbids."""

    def __getattr__(self, name):
        raise AssertionError("run_batches touched the context (%s) before checking its arguments" % name)


@pytest.mark.parametrize("n_photons,n_batches", [(4096, 0), (4096, 1), (4096, 3), (10, 4), (4096, -2)])
def test_run_batches_rejects_unequal_batches_before_any_device_call(n_photons, n_batches):
    tr = PT.PhotonTracer(ctx=_NoDevice())
    with pytest.raises(ValueError):
        tr.run_batches(n_photons, n_batches, seed=1, profiles=("z",))
