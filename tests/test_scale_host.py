"""The scaling rule of the scaled render (K10) restated in numpy, its self-checks, and the
host-only thumbnail size helper.

scale_ref is the reference the GPU tests (test_scale_gpu.py) compare with, bit for bit: an exact
area-weighted mean in integers, rounded half up (include/omr/omr.h)."""
import ctypes

import numpy as np
import pytest

from omr import _lib


def weights(n_src, n_dst):
    """Integer overlap matrix [n_dst][n_src]: in units of 1/n_dst source cell x covers
    [x*n_dst, (x+1)*n_dst) and output cell i covers [i*n_src, (i+1)*n_src)."""
    assert 1 <= n_dst <= n_src
    x = np.arange(n_src, dtype=np.int64)[None, :]
    i = np.arange(n_dst, dtype=np.int64)[:, None]
    lo = np.maximum(i * n_src, x * n_dst)
    hi = np.minimum((i + 1) * n_src, (x + 1) * n_dst)
    return np.maximum(hi - lo, 0)


def scale_ref(argb, tw, th):
    """argb uint32 [H][W] -> uint32 [th][tw] by the rule, every byte (alpha included)."""
    argb = np.ascontiguousarray(argb, dtype=np.uint32)
    H, W = argb.shape
    wx, wy = weights(W, tw), weights(H, th)
    assert 255 * W * H + W * H // 2 < 2 ** 53        # float64 matmul of integers stays exact
    fx, fy = wx.astype(np.float64), wy.astype(np.float64)
    out = np.zeros((th, tw), np.uint32)
    for shift in (0, 8, 16, 24):
        plane = ((argb >> np.uint32(shift)) & np.uint32(0xFF)).astype(np.float64)
        s = (fy @ plane @ fx.T).astype(np.int64)
        out |= (((s + (W * H) // 2) // (W * H)).astype(np.uint32)) << np.uint32(shift)
    return out


def thumbnail_size_ref(size_x, size_y, longest_side):
    big, small = max(size_x, size_y), min(size_x, size_y)
    if big <= longest_side:
        return size_x, size_y
    short = max(1, small * longest_side // big)
    return (longest_side, short) if size_x >= size_y else (short, longest_side)


def _random_argb(rng, h, w):
    return rng.integers(0, 2 ** 32, (h, w), dtype=np.uint64).astype(np.uint32)


# ---- scale_ref's self-checks -------------------------------------------------------------------
@pytest.mark.parametrize("n_src,n_dst", [(1, 1), (7, 7), (7, 1), (16, 4), (13, 6), (33, 32), (200, 61), (4200, 96)])
def test_weight_rows_sum_to_the_source_length(n_src, n_dst):
    w = weights(n_src, n_dst)
    assert (w.sum(1) == n_src).all() and (w.sum(0) == n_dst).all()
    assert w.min() >= 0 and w.max() <= n_dst


def test_float_matmul_is_the_integer_matmul():
    rng = np.random.default_rng(1)
    a = _random_argb(rng, 131, 200)
    wx, wy = weights(200, 97), weights(131, 61)
    exp = np.zeros((61, 97), np.uint32)
    for shift in (0, 8, 16, 24):
        s = wy @ ((a >> np.uint32(shift)) & np.uint32(0xFF)).astype(np.int64) @ wx.T
        exp |= ((s + (200 * 131) // 2) // (200 * 131)).astype(np.uint32) << np.uint32(shift)
    np.testing.assert_array_equal(scale_ref(a, 97, 61), exp)


def test_identity_returns_the_input():
    a = _random_argb(np.random.default_rng(2), 5, 7)
    np.testing.assert_array_equal(scale_ref(a, 7, 5), a)


def test_integer_ratio_is_the_block_mean_rounded_half_up():
    rng = np.random.default_rng(3)
    a = _random_argb(rng, 12, 20)
    got = scale_ref(a, 5, 4)                         # 4 x 3 blocks
    for shift in (0, 8, 16, 24):
        p = ((a >> np.uint32(shift)) & np.uint32(0xFF)).astype(np.int64)
        mean = (p.reshape(4, 3, 5, 4).sum((1, 3)) + 6) // 12
        np.testing.assert_array_equal((got >> np.uint32(shift)) & np.uint32(0xFF), mean)


def test_half_rounds_up():
    assert scale_ref(np.array([[0, 1]], np.uint32), 1, 1)[0, 0] == 1
    assert scale_ref(np.array([[0, 0, 1]], np.uint32), 1, 1)[0, 0] == 0


def test_constant_image_stays_constant():
    a = np.full((131, 200), 0xFF9C0137, np.uint32)
    assert (scale_ref(a, 97, 61) == 0xFF9C0137).all()


@pytest.mark.parametrize("fh,fv", [(True, False), (False, True), (True, True)])
def test_scale_then_flip_is_flip_then_scale(fh, fv):
    a = _random_argb(np.random.default_rng(4), 33, 47)

    def flip(x):
        x = x[:, ::-1] if fh else x
        return x[::-1] if fv else x
    np.testing.assert_array_equal(flip(scale_ref(a, 13, 10)), scale_ref(flip(a), 13, 10))


# ---- omr_thumbnail_size --------------------------------------------------------------------------
def _size(x, y, s):
    w, h = ctypes.c_int32(-1), ctypes.c_int32(-1)
    st = _lib.lib.omr_thumbnail_size(x, y, s, ctypes.byref(w), ctypes.byref(h))
    return st, w.value, h.value


def test_thumbnail_size_against_the_restatement():
    grid = [1, 2, 3, 7, 63, 64, 65, 95, 96, 97, 100, 255, 256, 257, 1000, 1024, 2047, 2999, 3000]
    for s in (1, 64, 96, 256):
        for x in grid:
            for y in grid:
                assert _size(x, y, s) == (0,) + thumbnail_size_ref(x, y, s), (x, y, s)


def test_thumbnail_size_cases():
    import omr
    assert omr.thumbnail_size(300, 200, 96) == (96, 64)
    assert omr.thumbnail_size(200, 300) == (64, 96)
    assert omr.thumbnail_size(80, 96, 96) == (80, 96)          # no upscaling
    assert omr.thumbnail_size(3000, 7, 96) == (96, 1)          # max(1, 7*96 // 3000 = 0)
    assert omr.thumbnail_size(7, 3000, 96) == (1, 96)
    assert omr.thumbnail_size(2 ** 31 - 1, 2 ** 31 - 2, 2 ** 30) == (2 ** 30, 2 ** 30 - 1)   # int64 product


@pytest.mark.parametrize("x,y,s", [(0, 10, 96), (10, 0, 96), (-1, 10, 96), (10, 10, 0), (10, 10, -5)])
def test_thumbnail_size_invalid(x, y, s):
    assert _size(x, y, s)[0] == _lib.INVALID_ARGUMENT
    import omr
    with pytest.raises(_lib.OmrError):
        omr.thumbnail_size(x, y, s)


def test_thumbnail_size_null_outputs():
    assert _lib.lib.omr_thumbnail_size(10, 10, 96, None, None) == _lib.INVALID_ARGUMENT
