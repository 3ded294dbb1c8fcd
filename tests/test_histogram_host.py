"""omr_histogram_bin_of (the histogram's binning rule on the host) against its numpy restatement.

The reference snapshot has no histogram code: the rule in include/omr/omr.h is the project's own,
and the restatement below is the checker for it, here and in tests/test_histogram_gpu.py.  All
arithmetic is IEEE double with one rounding per operation; comparisons are exact.
"""
import numpy as np
import pytest

import omr
from omr import _lib

BIN_COUNTS = (1, 7, 256, 1000, 4096)
INT32_RANGE = (-2147483648.0, 2147483647.0)


def ref_bins(v, lo, hi, n):
    """Bin index of every value: -3 NaN, -1 below lo, -2 above hi, else
    min((int64)((v - lo) / ((hi - lo + 1.0) / n)), n - 1)."""
    v = np.asarray(v, dtype=np.float64)
    lo, hi = np.float64(lo), np.float64(hi)
    out = np.empty(v.shape, dtype=np.int64)
    nan = np.isnan(v)
    with np.errstate(invalid="ignore"):
        below = v < lo
        above = v > hi
    inside = ~(nan | below | above)
    rng = hi - lo + np.float64(1.0)
    bin_range = rng / np.float64(n)
    q = (v[inside] - lo) / bin_range
    out[nan] = -3
    out[below] = -1
    out[above] = -2
    out[inside] = np.minimum(q.astype(np.int64), n - 1)     # truncation; q >= 0 here
    return out


def ref_histogram(v, lo, hi, n):
    """(counts[n] uint32, below, above, nan_count) of the values v."""
    b = ref_bins(np.asarray(v, dtype=np.float64).reshape(-1), lo, hi, n)
    counts = np.bincount(b[b >= 0], minlength=n).astype(np.uint32)
    return counts, int((b == -1).sum()), int((b == -2).sum()), int((b == -3).sum())


def edge_values(lo, hi, n, max_edges=None):
    """Every bin edge lo + k * bin_range (k = 0..n, or max_edges of them spread over 0..n with
    both ends) and both of its nextafter neighbours, as doubles."""
    lo, hi = np.float64(lo), np.float64(hi)
    bin_range = (hi - lo + np.float64(1.0)) / np.float64(n)
    ks = np.arange(n + 1, dtype=np.float64)
    if max_edges is not None and ks.size > max_edges:
        ks = np.unique(np.round(np.linspace(0, n, max_edges)))
    e = lo + ks * bin_range
    return np.concatenate([e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf)])


def lib_bins(v, lo, hi, n):
    return np.array([omr.histogram_bin_of(x, lo, hi, n) for x in np.asarray(v, dtype=np.float64).reshape(-1)],
                    dtype=np.int64)


@pytest.mark.parametrize("n", BIN_COUNTS)
def test_every_uint16_value(n):
    v = np.arange(65536, dtype=np.float64)
    want = ref_bins(v, 0.0, 65535.0, n)
    np.testing.assert_array_equal(lib_bins(v, 0.0, 65535.0, n), want)
    # the restatement itself, on this range: nothing outside, and the bins as even as n allows
    assert want.min() == 0 and want.max() == n - 1
    counts = np.bincount(want, minlength=n)
    expect = {1: (65536, 65536), 7: (9362, 9363), 256: (256, 256), 1000: (65, 66), 4096: (16, 16)}[n]
    assert (counts.min(), counts.max()) == expect
    assert counts.sum() == 65536


@pytest.mark.parametrize("n", BIN_COUNTS)
@pytest.mark.parametrize("lo,hi", [INT32_RANGE, (0.0, 1.0)])
def test_bin_edges_and_neighbours(lo, hi, n):
    v = edge_values(lo, hi, n)
    np.testing.assert_array_equal(lib_bins(v, lo, hi, n), ref_bins(v, lo, hi, n))


@pytest.mark.parametrize("n", BIN_COUNTS)
def test_clamp_when_the_plus_one_is_absorbed(n):
    lo, hi = -1e300, 1e300
    # hi - lo >= 2^53: range == hi - lo, so v = hi gives q = n and only the clamp keeps it in
    assert omr.histogram_bin_of(hi, lo, hi, n) == n - 1
    assert omr.histogram_bin_of(lo, lo, hi, n) == 0
    v = np.concatenate([edge_values(lo, hi, n, 64), [hi, lo, 0.0, -0.0, 1.0, np.nextafter(hi, 0.0)]])
    np.testing.assert_array_equal(lib_bins(v, lo, hi, n), ref_bins(v, lo, hi, n))


@pytest.mark.parametrize("n", BIN_COUNTS)
@pytest.mark.parametrize("lo,hi", [(0.0, 65535.0), INT32_RANGE, (0.0, 1.0), (-3.5, 1234.25), (7.0, 7.0)])
def test_special_values(lo, hi, n):
    assert omr.histogram_bin_of(float("nan"), lo, hi, n) == -3
    assert omr.histogram_bin_of(float("inf"), lo, hi, n) == -2
    assert omr.histogram_bin_of(float("-inf"), lo, hi, n) == -1
    assert omr.histogram_bin_of(lo, lo, hi, n) == 0
    assert omr.histogram_bin_of(np.nextafter(lo, -np.inf), lo, hi, n) == -1
    assert omr.histogram_bin_of(np.nextafter(hi, np.inf), lo, hi, n) == -2
    v = np.array([np.nan, np.inf, -np.inf, lo, hi, 0.0, -0.0, (lo + hi) / 2])
    np.testing.assert_array_equal(lib_bins(v, lo, hi, n), ref_bins(v, lo, hi, n))
    assert 0 <= omr.histogram_bin_of(hi, lo, hi, n) <= n - 1


def test_constants_and_struct_layout():
    import ctypes
    assert (_lib.HIST_RANGE_TYPE, _lib.HIST_RANGE_PLANE, _lib.HIST_RANGE_EXPLICIT) == (0, 1, 2)
    assert _lib.HIST_MAX_BINS == 4096
    assert ctypes.sizeof(_lib.PlaneStats) == 32 and _lib.PlaneStats.nan_count.offset == 24
    assert ctypes.sizeof(_lib.HistogramInfo) == 40 and _lib.HistogramInfo.nan_count.offset == 32
