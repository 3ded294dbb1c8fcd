"""K9 on the device: plane statistics and histograms against the numpy restatement of
tests/test_histogram_host.py.  Counts and statistics are compared exactly, no tolerance."""
import ctypes
import os

import numpy as np
import pytest

import omr
from omr import _lib
from omr.synthetic import microscopy_u16
from test_histogram_host import BIN_COUNTS, INT32_RANGE, edge_values, ref_histogram

pytestmark = pytest.mark.gpu

DTYPES = {_lib.PIXELS_INT8: np.int8, _lib.PIXELS_UINT8: np.uint8, _lib.PIXELS_INT16: np.int16,
          _lib.PIXELS_UINT16: np.uint16, _lib.PIXELS_INT32: np.int32, _lib.PIXELS_UINT32: np.uint32,
          _lib.PIXELS_FLOAT: np.float32, _lib.PIXELS_DOUBLE: np.float64}
TYPE_RANGE = {_lib.PIXELS_INT8: (-128.0, 127.0), _lib.PIXELS_UINT8: (0.0, 255.0),
              _lib.PIXELS_INT16: (-32768.0, 32767.0), _lib.PIXELS_UINT16: (0.0, 65535.0),
              _lib.PIXELS_INT32: INT32_RANGE, _lib.PIXELS_UINT32: (0.0, 4294967295.0),
              _lib.PIXELS_FLOAT: (0.0, 1.0), _lib.PIXELS_DOUBLE: (0.0, 1.0)}
TYPE_IDS = {v: k for k, v in _lib.PIXEL_TYPE_NAMES.items()}
ALL_TYPES = sorted(DTYPES)


def is_float(pt):
    return pt in (_lib.PIXELS_FLOAT, _lib.PIXELS_DOUBLE)


def order(a, big_endian):
    """The array's bytes as the device reads them: big-endian (file order) or native."""
    return a.astype(a.dtype.newbyteorder(">")) if big_endian else np.ascontiguousarray(a)


def random_plane(pt, h, w, rng, nans=0):
    dt = DTYPES[pt]
    if is_float(pt):
        a = (rng.normal(0.3, 40.0, size=(h, w))).astype(dt)
        a.reshape(-1)[rng.choice(h * w, 12, replace=False)] = rng.uniform(0, 1, 12).astype(dt)   # some inside (0, 1)
        if nans:
            a.reshape(-1)[rng.choice(h * w, nans, replace=False)] = np.nan
        return a
    info = np.iinfo(dt)
    return rng.integers(info.min, int(info.max) + 1, size=(h, w), dtype=np.int64).astype(dt)


def check_hist(ctx, planes, pt, w, h, ranges, n, big_endian=False, row_stride=0, region=None, values=None):
    """One device call against the restatement; values[i]: the pixels plane i's region holds."""
    dev = [order(p, big_endian) for p in planes]
    counts, info = ctx.histogram(dev, pt, w, h, ranges, bins=n, big_endian=big_endian, row_stride=row_stride,
                                 region=region)
    assert counts.shape == (len(planes), n) and counts.dtype == np.uint32
    for i, p in enumerate(planes):
        v = (p if values is None else values[i]).astype(np.float64).reshape(-1)
        lo, hi = ranges[i] if len(ranges) > 1 else ranges[0]
        want, below, above, nan = ref_histogram(v, lo, hi, n)
        tag = f"{TYPE_IDS[pt]} be={big_endian} n={n} range=({lo}, {hi}) plane {i}"
        np.testing.assert_array_equal(counts[i], want, err_msg=tag)
        assert (info[i]["below"], info[i]["above"], info[i]["nan_count"]) == (below, above, nan), tag
        assert (info[i]["lo"], info[i]["hi"]) == (lo, hi), tag
        assert int(counts[i].sum(dtype=np.uint64)) + below + above + nan == v.size, tag
    return counts, info


# 1 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("big_endian", [False, True])
@pytest.mark.parametrize("pt", ALL_TYPES, ids=[TYPE_IDS[t] for t in ALL_TYPES])
def test_ragged_plane_every_type(ctx, pt, big_endian):
    w, h = 9, 13                                   # 117 pixels: no row is a whole number of vectors
    rng = np.random.default_rng(100 + pt)
    p = random_plane(pt, h, w, rng, nans=2 if is_float(pt) else 0)
    v = np.sort(p.astype(np.float64).reshape(-1))
    v = v[~np.isnan(v)]
    narrow = (float(v[v.size // 4]), float(v[3 * v.size // 4]))
    ranges = {"type": TYPE_RANGE[pt], "plane": (float(v[0]), float(v[-1])), "narrow": narrow}
    for n in BIN_COUNTS:
        for name, r in ranges.items():
            _, info = check_hist(ctx, [p], pt, w, h, [r], n, big_endian=big_endian)
            if name == "narrow":
                assert info[0]["below"] > 0 and info[0]["above"] > 0
            if name == "plane":
                assert info[0]["below"] == 0 and info[0]["above"] == 0


# 2 ---------------------------------------------------------------------------------------
REGION = (3, 5, 41, 17)
REGION_W, REGION_H, REGION_STRIDE = 64, 50, 80


def poisoned_plane(pt, rng):
    """[50][80] buffer of a 64-wide plane: mid-range pixels inside REGION, extreme values (and
    NaN for float) everywhere else, the stride padding included."""
    dt = DTYPES[pt]
    x, y, w, h = REGION
    if is_float(pt):
        buf = np.empty((REGION_H, REGION_STRIDE), dtype=dt)
        buf.reshape(-1)[0::3] = np.finfo(dt).max
        buf.reshape(-1)[1::3] = -np.finfo(dt).max
        buf.reshape(-1)[2::3] = np.nan
        inside = rng.uniform(0.25, 0.75, size=(h, w)).astype(dt)
    else:
        info = np.iinfo(dt)
        buf = np.where(rng.integers(0, 2, size=(REGION_H, REGION_STRIDE)) == 1, info.max, info.min).astype(dt)
        span = int(info.max) - int(info.min)
        inside = rng.integers(int(info.min) + span // 4, int(info.max) - span // 4, size=(h, w)).astype(dt)
    buf[y:y + h, x:x + w] = inside
    return buf, inside


@pytest.mark.parametrize("big_endian", [False, True])
@pytest.mark.parametrize("pt", [_lib.PIXELS_UINT8, _lib.PIXELS_UINT16, _lib.PIXELS_FLOAT],
                         ids=["uint8", "uint16", "float"])
def test_misaligned_region(ctx, pt, big_endian):
    buf, inside = poisoned_plane(pt, np.random.default_rng(7 + pt))
    for n in (7, 256, 4096):
        counts, info = check_hist(ctx, [buf], pt, REGION_W, REGION_H, [TYPE_RANGE[pt]], n, big_endian=big_endian,
                                  row_stride=REGION_STRIDE, region=REGION, values=[inside])
        assert info[0]["nan_count"] == 0 and info[0]["below"] == 0 and info[0]["above"] == 0
    st = ctx.plane_stats([order(buf, big_endian)], pt, REGION_W, REGION_H, big_endian=big_endian,
                         row_stride=REGION_STRIDE, region=REGION)[0]
    assert (st["min"], st["max"]) == (float(inside.min()), float(inside.max()))
    assert (st["count"], st["nan_count"]) == (inside.size, 0)


# 3 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("big_endian", [False, True])
@pytest.mark.parametrize("pt", [_lib.PIXELS_UINT16, _lib.PIXELS_INT16], ids=["uint16", "int16"])
def test_every_16bit_code(ctx, pt, big_endian):
    rng = np.random.default_rng(16)
    p = rng.permutation(65536).astype(np.uint16).view(DTYPES[pt]).reshape(256, 256)
    for n in (256, 1000, 4096):
        check_hist(ctx, [p], pt, 256, 256, [TYPE_RANGE[pt]], n, big_endian=big_endian)
    # a range with fractional ends inside the type's: the table's below / above thresholds
    check_hist(ctx, [p], pt, 256, 256, [(-1000.5, 20000.25)], 1000, big_endian=big_endian)


# 4 ---------------------------------------------------------------------------------------
def edge_plane(pt, lo, hi, n):
    """33 x 31 plane of bin edges and their neighbours in the pixel type (padded with lo)."""
    dt = DTYPES[pt]
    e = edge_values(lo, hi, n, max_edges=100 if pt == _lib.PIXELS_FLOAT else 300)
    if is_float(pt):
        v = e.astype(dt)
        if pt == _lib.PIXELS_FLOAT:      # the float32 neighbours too: a double's are lost in the rounding
            v = np.concatenate([v, np.nextafter(v, dt(-np.inf)), np.nextafter(v, dt(np.inf))])
        v = np.concatenate([v, np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, lo, hi], dtype=dt)])
    else:
        info = np.iinfo(dt)
        f = np.floor(e)
        v = np.clip(np.concatenate([f - 1, f, f + 1, [lo, hi]]), info.min, info.max).astype(np.int64).astype(dt)
    v = np.unique(v) if not is_float(pt) else v
    rng = np.random.default_rng(n)
    if v.size > 33 * 31:
        v = rng.choice(v, 33 * 31, replace=False)
    out = np.full(33 * 31, lo, dtype=dt)
    out[:v.size] = v
    return rng.permutation(out).reshape(31, 33)


@pytest.mark.parametrize("big_endian", [False, True])
@pytest.mark.parametrize("pt", [_lib.PIXELS_INT32, _lib.PIXELS_UINT32, _lib.PIXELS_FLOAT, _lib.PIXELS_DOUBLE],
                         ids=["int32", "uint32", "float", "double"])
def test_bin_edges_evaluated_types(ctx, pt, big_endian):
    ranges = [INT32_RANGE, (0.0, 1.0)] if pt != _lib.PIXELS_UINT32 else [(0.0, 4294967295.0), (0.0, 1.0)]
    for lo, hi in ranges:
        for n in BIN_COUNTS:
            p = edge_plane(pt, lo, hi, n)
            check_hist(ctx, [p], pt, 33, 31, [(lo, hi)], n, big_endian=big_endian)
    if pt == _lib.PIXELS_DOUBLE:         # the clamp: hi - lo + 1.0 == hi - lo, v = hi gives q = n
        p = edge_plane(pt, -1e300, 1e300, 256)
        counts, _ = check_hist(ctx, [p], pt, 33, 31, [(-1e300, 1e300)], 256, big_endian=big_endian)
        assert counts[0][255] >= 1


# 5 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [256, 4096])
def test_contention_and_counter_width(ctx, n):
    const = np.full((512, 512), 1234, dtype=np.uint16)
    counts, _ = check_hist(ctx, [const], _lib.PIXELS_UINT16, 512, 512, [TYPE_RANGE[_lib.PIXELS_UINT16]], n)
    assert counts.max() == 262144 and np.count_nonzero(counts) == 1
    yy, xx = np.mgrid[0:512, 0:512]
    checker = np.where((yy + xx) % 2 == 0, 300, 40000).astype(np.uint16)
    counts, _ = check_hist(ctx, [checker], _lib.PIXELS_UINT16, 512, 512, [TYPE_RANGE[_lib.PIXELS_UINT16]], n,
                           big_endian=True)
    assert sorted(counts[counts > 0].tolist()) == [131072, 131072]
    # the same through the evaluated route (a type without a table)
    counts, _ = check_hist(ctx, [const.astype(np.int32)], _lib.PIXELS_INT32, 512, 512, [(0.0, 65535.0)], n)
    assert counts.max() == 262144


# 6 ---------------------------------------------------------------------------------------
def test_many_workgroups_batched(ctx):
    rng = np.random.default_rng(6)
    planes = [microscopy_u16(1024, 1024, rng, blobs=8) for _ in range(3)]
    ranges = [(0.0, 65535.0), (100.0, 4095.0), (float(planes[2].min()), float(planes[2].max()))]
    counts, info = check_hist(ctx, planes, _lib.PIXELS_UINT16, 1024, 1024, ranges, 256, big_endian=True)
    for i in range(3):
        assert int(counts[i].sum(dtype=np.uint64)) + info[i]["below"] + info[i]["above"] + info[i]["nan_count"] == 1048576
    again, info2 = ctx.histogram([order(p, True) for p in planes], _lib.PIXELS_UINT16, 1024, 1024, ranges, bins=256,
                                 big_endian=True)
    np.testing.assert_array_equal(again, counts)
    assert info2 == info


# 7 ---------------------------------------------------------------------------------------
def ref_stats(p):
    v = p.astype(np.float64).reshape(-1)
    nan = int(np.isnan(v).sum())
    ok = v[~np.isnan(v)]
    return {"min": float(ok.min()) if ok.size else float("inf"), "max": float(ok.max()) if ok.size else float("-inf"),
            "count": int(ok.size), "nan_count": nan}


@pytest.mark.parametrize("big_endian", [False, True])
@pytest.mark.parametrize("pt", ALL_TYPES, ids=[TYPE_IDS[t] for t in ALL_TYPES])
def test_statistics_every_type(ctx, pt, big_endian):
    rng = np.random.default_rng(70 + pt)
    for h, w in ((13, 9), (64, 257)):
        p = random_plane(pt, h, w, rng, nans=3 if is_float(pt) else 0)
        if is_float(pt):
            p[0, 0], p[h - 1, w - 1] = np.inf, -np.inf          # the infinities take part
        got = ctx.plane_stats([order(p, big_endian)], pt, w, h, big_endian=big_endian)
        assert got == [ref_stats(p)], f"{TYPE_IDS[pt]} be={big_endian} {w}x{h}"


def test_statistics_all_nan_and_batch(ctx):
    p = np.full((31, 33), np.nan, dtype=np.float32)
    got = ctx.plane_stats([p], _lib.PIXELS_FLOAT, 33, 31)[0]
    assert got == {"min": float("inf"), "max": float("-inf"), "count": 0, "nan_count": 31 * 33}
    rng = np.random.default_rng(71)
    planes = []
    for i in range(4):
        a = rng.integers(1000 * (i + 1), 2000 * (i + 1), size=(100, 130)).astype(np.int16)
        a[rng.integers(0, 100), rng.integers(0, 130)] = -5 * (i + 1)
        planes.append(a)
    got = ctx.plane_stats([order(a, True) for a in planes], _lib.PIXELS_INT16, 130, 100, big_endian=True)
    assert got == [ref_stats(a) for a in planes]
    assert len({g["min"] for g in got}) == 4 and len({g["max"] for g in got}) == 4


# 8 ---------------------------------------------------------------------------------------
def test_pixel_buffer_histogram(ctx, tmp_path):
    rng = np.random.default_rng(8)
    px = rng.integers(200, 5000, size=(2, 2, 3, 37, 53)).astype(np.uint16)
    path = os.path.join(tmp_path, "pixels.raw")
    omr.write_romio(path, px, _lib.PIXELS_UINT16)
    with omr.PixelBuffer(path, 53, 37, 3, 2, 2, _lib.PIXELS_UINT16) as pb:
        z, c, t = 2, 1, 1
        plane = px[t, c, z]
        cases = [(_lib.HIST_RANGE_TYPE, None, None, (0.0, 65535.0)),
                 (_lib.HIST_RANGE_PLANE, None, None, (float(plane.min()), float(plane.max()))),
                 (_lib.HIST_RANGE_EXPLICIT, 1000.0, 3000.5, (1000.0, 3000.5))]
        for mode, lo, hi, (rlo, rhi) in cases:
            counts, info, stats = pb.histogram(ctx, z, c, t, bins=256, range_mode=mode, lo=lo, hi=hi)
            want, below, above, nan = ref_histogram(plane, rlo, rhi, 256)
            np.testing.assert_array_equal(counts, want)
            assert info == {"lo": rlo, "hi": rhi, "below": below, "above": above, "nan_count": nan}
            assert stats == ref_stats(plane)
        x, y, w, h = 5, 7, 31, 11
        sub = plane[y:y + h, x:x + w]
        counts, info, stats = pb.histogram(ctx, z, c, t, bins=1000, range_mode=_lib.HIST_RANGE_PLANE, region=(x, y, w, h))
        want, below, above, nan = ref_histogram(sub, float(sub.min()), float(sub.max()), 1000)
        np.testing.assert_array_equal(counts, want)
        assert (info["lo"], info["hi"], info["below"], info["above"]) == (float(sub.min()), float(sub.max()), 0, 0)
        assert stats == ref_stats(sub)
        js = omr.histogram_json(ctx, pb, z, c, t, bins=256)
        assert set(js) == {"min", "max", "binCount", "data", "leftOutsideCount", "rightOutsideCount"}
        want, below, above, _ = ref_histogram(plane, 0.0, 65535.0, 256)
        assert js["data"] == want.tolist() and all(type(v) is int for v in js["data"])
        assert (js["min"], js["max"], js["binCount"]) == (0.0, 65535.0, 256)
        assert (js["leftOutsideCount"], js["rightOutsideCount"]) == (below, above)
        js = omr.histogram_json(ctx, pb, z, c, t, bins=64, use_pixels_type_range=False)
        assert (js["min"], js["max"]) == (float(plane.min()), float(plane.max())) and sum(js["data"]) == plane.size
        with pytest.raises(omr.OmrError) as e:
            pb.histogram(ctx, 3, c, t)
        assert e.value.status == _lib.INVALID_ARGUMENT
        # the host-plane call sees the same plane
        counts, info, stats = ctx.histogram_host(plane.astype(">u2"), _lib.PIXELS_UINT16, 53, 37, bins=256,
                                                 range_mode=_lib.HIST_RANGE_PLANE, big_endian=True)
        want, _, _, _ = ref_histogram(plane, float(plane.min()), float(plane.max()), 256)
        np.testing.assert_array_equal(counts, want)
        assert stats == ref_stats(plane)


# 9 ---------------------------------------------------------------------------------------
def test_argument_errors_leave_the_context_usable(ctx):
    import torch
    w, h, n = 40, 30, 64
    rng = np.random.default_rng(9)
    p = rng.integers(0, 65536, size=(h, w)).astype(np.uint16)
    d = torch.from_numpy(p.view(np.uint8).reshape(-1)).to("cuda:0")
    big = torch.empty(1 << 32, dtype=torch.uint8, device="cuda:0")     # a real 65536 x 65536 uint8 plane
    torch.cuda.synchronize()
    lib = _lib.lib
    PT = _lib.PIXELS_UINT16
    counts = np.zeros((32, 4096), np.uint32)
    info = (_lib.HistogramInfo * 33)()
    stats = (_lib.PlaneStats * 33)()

    def hist(planes=(d.data_ptr(),), n_planes=None, pt=PT, width=w, height=h, stride=0, region=None, lo=(0.0,),
             hi=(65535.0,), bins=n, counts_p=counts.ctypes.data, info_p=info, planes_null=False, lo_null=False):
        k = len(planes) if n_planes is None else n_planes
        ptrs = (ctypes.c_void_p * max(len(planes), 1))(*planes)
        los = (ctypes.c_double * 33)(*(list(lo) * 33)[:33])
        his = (ctypes.c_double * 33)(*(list(hi) * 33)[:33])
        reg = None if region is None else ctypes.pointer(_lib.Region(*region))
        return lib.omr_histogram_device(ctx.h, None if planes_null else ptrs, k, pt, 0, width, height, stride, reg,
                                        None if lo_null else los, his, bins, counts_p, info_p)

    def stat(planes=(d.data_ptr(),), n_planes=None, pt=PT, width=w, height=h, stride=0, region=None, out=stats):
        k = len(planes) if n_planes is None else n_planes
        ptrs = (ctypes.c_void_p * max(len(planes), 1))(*planes)
        reg = None if region is None else ctypes.pointer(_lib.Region(*region))
        return lib.omr_plane_stats_device(ctx.h, ptrs, k, pt, 0, width, height, stride, reg, out)

    inf, nan = float("inf"), float("nan")
    bad = {
        "null plane list": hist(planes_null=True), "null plane": hist(planes=(None,)),
        "null counts": hist(counts_p=None), "null info": hist(info_p=None), "null lo": hist(lo_null=True),
        "null stats": stat(out=None), "null plane (stats)": stat(planes=(None,)),
        "pixel type": hist(pt=8), "pixel type -1": hist(pt=-1), "pixel type (stats)": stat(pt=99),
        "0 planes": hist(n_planes=0), "33 planes": hist(planes=(d.data_ptr(),) * 33),
        "0 planes (stats)": stat(n_planes=0), "33 planes (stats)": stat(planes=(d.data_ptr(),) * 33),
        "0 bins": hist(bins=0), "4097 bins": hist(bins=4097), "-1 bins": hist(bins=-1),
        "lo nan": hist(lo=(nan,)), "hi inf": hist(hi=(inf,)), "lo -inf": hist(lo=(-inf,)),
        "hi - lo inf": hist(lo=(-1.7e308,), hi=(1.7e308,)), "lo > hi": hist(lo=(10.0,), hi=(9.0,)),
        "width 0": hist(width=0), "height -1": hist(height=-1), "width 0 (stats)": stat(width=0),
        "region w 0": hist(region=(0, 0, 0, 5)), "region h -1": hist(region=(0, 0, 5, -1)),
        "region right": hist(region=(10, 0, 31, 5)), "region bottom": hist(region=(0, 26, 5, 5)),
        "region x -1": hist(region=(-1, 0, 5, 5)), "region (stats)": stat(region=(0, 0, 41, 5)),
        "stride 1": hist(stride=1), "stride w-1": hist(stride=w - 1), "stride (stats)": stat(stride=w - 1),
        "2^32 pixels": hist(planes=(big.data_ptr(),), pt=_lib.PIXELS_UINT8, width=65536, height=65536, lo=(0.0,),
                            hi=(255.0,)),
        "2^32 pixels (stats)": stat(planes=(big.data_ptr(),), pt=_lib.PIXELS_UINT8, width=65536, height=65536),
    }
    wrong = {k: v for k, v in bad.items() if v != _lib.INVALID_ARGUMENT}
    assert not wrong, wrong
    with pytest.raises(omr.OmrError) as e:
        ctx.histogram_host(p, PT, w, h, bins=n, range_mode=3)
    assert e.value.status == _lib.INVALID_ARGUMENT
    with pytest.raises(omr.OmrError) as e:
        ctx.histogram_host(p, PT, w, h, bins=n, range_mode=_lib.HIST_RANGE_EXPLICIT, lo=5.0, hi=nan)
    assert e.value.status == _lib.INVALID_ARGUMENT
    del big
    # the same context, a valid call: still exact
    assert hist() == _lib.OK
    want, below, above, _ = ref_histogram(p, 0.0, 65535.0, n)
    np.testing.assert_array_equal(counts.reshape(-1)[:n], want)
    check_hist(ctx, [p], PT, w, h, [(1000.0, 60000.0)], n)
    assert ctx.plane_stats([d], PT, w, h) == [ref_stats(p)]
