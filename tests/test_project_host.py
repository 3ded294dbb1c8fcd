"""The projection's plane count and its stepping rule, on the host (no GPU).

omr_projection_plane_count is the one place the count of projected planes is computed
(enqueue_projection, the fused glue and the restatement take it from the same expression).
It is compared here with the two loops of the reference, restated with Java's int arithmetic:
  max       for (int z = start; z <= end; z += stepping)      ProjectionService.java:184
  mean/sum  for (int z = start; z <  end; z += stepping)      ProjectionService.java:271
where `z += stepping` wraps at 2^31 and a negative z makes getPixelValue throw.
"""
import ctypes
import itertools

import numpy as np
import pytest

import oracle_lib as O
from omr import _lib

INT_MAX = 2**31 - 1
ALGS = [_lib.PROJECTION_MAX, _lib.PROJECTION_MEAN, _lib.PROJECTION_SUM]
STEPPINGS = [1, 2, 3, 7, 12, 13, 2**31 - 2, 2**31 - 1]


def java_loop(alg, start, end, stepping):
    """The reference's loop with Java int wrap-around: the number of planes read, or None where z
    wraps negative and the plane read throws."""
    z, count = start, 0
    while (z <= end) if alg == _lib.PROJECTION_MAX else (z < end):
        if z < 0:
            return None
        count += 1
        z += stepping
        if z > INT_MAX:
            z -= 2**32
    return count


def plane_count(alg, start, end, stepping):
    n = ctypes.c_int64(-7)
    st = _lib.lib.omr_projection_plane_count(alg, start, end, stepping, ctypes.byref(n))
    return st, n.value


def oracle_count(alg, start, end, stepping):
    n = ctypes.c_int64(-7)
    st = O.lib.oracle_projection_plane_count(alg, start, end, stepping, ctypes.byref(n))
    return st, n.value


@pytest.mark.parametrize("alg", ALGS)
def test_plane_count_matches_the_reference_loops(alg):
    for start, end, stepping in itertools.product(range(13), range(13), STEPPINGS):
        exp = java_loop(alg, start, end, stepping)
        st, n = plane_count(alg, start, end, stepping)
        if exp is None:
            assert st == _lib.INVALID_ARGUMENT, (start, end, stepping)
        else:
            assert (st, n) == (_lib.OK, exp), (start, end, stepping)
        assert oracle_count(alg, start, end, stepping) == (st, n), (start, end, stepping)


def test_plane_count_rejection_boundary():
    MAX, MEAN, SUM = ALGS
    # start + stepping == INT_MAX exactly: valid, one plane
    for alg in ALGS:
        assert plane_count(alg, 0, 2, INT_MAX) == (_lib.OK, 1)
        assert plane_count(alg, 1, 2, INT_MAX - 1) == (_lib.OK, 1)
    # one more wraps, when the loop runs at all: start <= end (max), start < end (mean, sum)
    for alg in ALGS:
        assert plane_count(alg, 1, 2, INT_MAX)[0] == _lib.INVALID_ARGUMENT
        assert plane_count(alg, 2, 3, INT_MAX - 1)[0] == _lib.INVALID_ARGUMENT
    assert plane_count(MAX, 1, 1, INT_MAX)[0] == _lib.INVALID_ARGUMENT
    assert plane_count(MEAN, 1, 1, INT_MAX) == (_lib.OK, 0)
    assert plane_count(SUM, 1, 1, INT_MAX) == (_lib.OK, 0)
    for alg in ALGS:                                   # the loop never runs: nothing wraps
        assert plane_count(alg, 2, 1, INT_MAX) == (_lib.OK, 0)
    # the issue's own example: (end - start + stepping - 1) wrapped in int32
    assert plane_count(MEAN, 0, 2, INT_MAX) == (_lib.OK, 1)
    # a later step wraps (only a stack of 2^30 planes and more reaches this): same rule, last z + stepping
    for alg, start, end, stepping in [(MAX, 0, INT_MAX - 1, 2**30), (SUM, 0, INT_MAX - 1, 2**30),
                                      (MAX, 5, 2**30 + 5, 2**30), (MEAN, 5, 2**30 + 5, 2**30),
                                      (MAX, 0, 2**30 - 1, 2**30), (MAX, 0, INT_MAX - 1, 1)]:
        exp = java_loop(alg, start, end, stepping) if stepping > 1 else INT_MAX
        st, n = plane_count(alg, start, end, stepping)
        assert (st, n if st == 0 else None) == ((_lib.OK, exp) if exp is not None else (_lib.INVALID_ARGUMENT, None))
        assert oracle_count(alg, start, end, stepping)[0] == st
    # what every projection call rejects anyway
    assert plane_count(MAX, 0, 2, 0)[0] == _lib.INVALID_ARGUMENT
    assert plane_count(MAX, 0, 2, -1)[0] == _lib.INVALID_ARGUMENT
    assert plane_count(MAX, -1, 2, 1)[0] == _lib.INVALID_ARGUMENT
    assert plane_count(MAX, 0, -2, 1)[0] == _lib.INVALID_ARGUMENT
    assert plane_count(3, 0, 2, 1)[0] == _lib.INVALID_ARGUMENT
    assert _lib.lib.omr_projection_plane_count(MAX, 0, 2, 1, None) == _lib.INVALID_ARGUMENT


@pytest.mark.parametrize("alg", ALGS)
def test_oracle_project_stack_status_parity(alg):
    """oracle_project_stack answers the same arguments with the same status, and where it
    projects, a pixel that holds 1 in every plane counts the planes (sum) or shows that one was read
    (max: 1, or 0 for an empty range)."""
    z = 13
    stack = np.ones((z, 1, 1), np.uint16)
    for start, end, stepping in itertools.product(range(13), range(13), STEPPINGS):
        st, n = plane_count(alg, start, end, stepping)
        ost, out = O.project(stack, _lib.PIXELS_UINT16, 1, 1, z, alg, start, end, stepping)
        assert ost == st, (start, end, stepping)
        if st == _lib.OK:
            v = int(out.view(np.uint16)[0])
            exp = {_lib.PROJECTION_MAX: min(n, 1), _lib.PROJECTION_MEAN: min(n, 1), _lib.PROJECTION_SUM: n}[alg]
            assert v == exp, (start, end, stepping)
