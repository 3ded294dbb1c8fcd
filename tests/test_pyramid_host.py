"""Resolution pyramids on the host (no GPU): the level-count and level-size helpers against the
formula, the numpy restatement of the two downsampling rules (pyramid_ref, which the GPU tests
import as their checker), the sidecar file written with numpy and read back through level views,
rejected sidecars, and omr_get_region_def fed with an attached buffer's descriptions."""
import ctypes
import math

import numpy as np
import pytest

import omr
from omr import PixelBuffer, _lib, write_pyramid, write_romio
from omr._lib import lib

SUB, MEAN = _lib.PYRAMID_SUBSAMPLE, _lib.PYRAMID_MEAN
NP_TYPES = {_lib.PIXELS_INT8: np.int8, _lib.PIXELS_UINT8: np.uint8, _lib.PIXELS_INT16: np.int16,
            _lib.PIXELS_UINT16: np.uint16, _lib.PIXELS_INT32: np.int32, _lib.PIXELS_UINT32: np.uint32,
            _lib.PIXELS_FLOAT: np.float32, _lib.PIXELS_DOUBLE: np.float64}


def max_levels(w, h):
    """1 + floor(log2(min(w, h))), capped at 16."""
    return min(_lib.PYRAMID_MAX_LEVELS, min(w, h).bit_length())


def level_count_ref(w, h, min_side):
    n = 1
    while max(w >> (n - 1), h >> (n - 1)) > min_side and n < max_levels(w, h):
        n += 1
    return n


def pyramid_ref(plane, rule, n_levels):
    """The rule of include/omr/omr.h in numpy: [L0, L1, ..., L(n_levels-1)] of a native-endian
    array [..., H, W] (leading axes are independent planes).  Level k is made from level k-1."""
    cur = np.ascontiguousarray(plane)
    cur = cur.astype(cur.dtype.newbyteorder("="))
    out = [cur]
    for _ in range(1, n_levels):
        h, w = cur.shape[-2] // 2, cur.shape[-1] // 2
        assert h >= 1 and w >= 1
        a = cur[..., 0:2 * h:2, 0:2 * w:2]
        b = cur[..., 0:2 * h:2, 1:2 * w:2]
        c = cur[..., 1:2 * h:2, 0:2 * w:2]
        d = cur[..., 1:2 * h:2, 1:2 * w:2]
        if rule == SUB:
            nxt = a.copy()
        elif cur.dtype == np.float64:
            with np.errstate(all="ignore"):
                nxt = ((a + b) + (c + d)) * 0.25
        elif cur.dtype == np.float32:
            with np.errstate(all="ignore"):
                f = np.float64
                nxt = (((a.astype(f) + b.astype(f)) + (c.astype(f) + d.astype(f))) * 0.25).astype(np.float32)
        else:
            i = np.int64
            s = a.astype(i) + b.astype(i) + c.astype(i) + d.astype(i) + 2
            nxt = (s >> 2).astype(cur.dtype)          # >> on int64 floors (arithmetic shift)
        cur = np.ascontiguousarray(nxt)
        out.append(cur)
    return out


# ---- level count and sizes ---------------------------------------------------------------------
@pytest.mark.parametrize("w,h,expect", [(4096, 4096, 5), (4096, 300, 5), (257, 256, 2), (256, 256, 1), (1, 1, 1),
                                        (3, 1000, 2), (1000, 3, 2), (100000, 80000, 10), (512, 1, 1), (513, 513, 2)])
def test_level_count_table(w, h, expect):
    assert omr.pyramid_level_count(w, h) == expect == level_count_ref(w, h, 256)


def test_level_count_against_formula():
    rng = np.random.default_rng(11)
    for _ in range(300):
        w, h = int(rng.integers(1, 200000)), int(rng.integers(1, 200000))
        m = int(rng.choice([1, 2, 7, 64, 256, 1000, 2**31 - 1]))
        assert omr.pyramid_level_count(w, h, m) == level_count_ref(w, h, m), (w, h, m)
    assert omr.pyramid_level_count(2**31 - 1, 2**31 - 1, 1) == 16          # the cap


@pytest.mark.parametrize("bad", [(0, 4, 256), (4, 0, 256), (-1, 4, 256), (4, 4, 0), (4, 4, -3)])
def test_level_count_invalid(bad):
    assert lib.omr_pyramid_level_count(*bad) == -_lib.INVALID_ARGUMENT
    with pytest.raises(_lib.OmrError) as e:
        omr.pyramid_level_count(*bad)
    assert e.value.status == _lib.INVALID_ARGUMENT


@pytest.mark.parametrize("w,h", [(4096, 4096), (4096, 300), (257, 256), (37, 21), (1, 1), (3, 1000), (65535, 2)])
def test_level_sizes(w, h):
    top = max_levels(w, h)
    for n in range(1, top + 1):
        sizes = omr.pyramid_level_sizes(w, h, n)
        assert sizes == [[w // 2**k, h // 2**k] for k in range(n)]
        assert min(sizes[-1]) >= 1
    for n in (0, -1, top + 1, 17):
        with pytest.raises(_lib.OmrError) as e:
            omr.pyramid_level_sizes(w, h, n)
        assert e.value.status == _lib.INVALID_ARGUMENT
    assert math.floor(math.log2(min(w, h))) + 1 >= top


def test_level_sizes_null_and_bad_size():
    out = (ctypes.c_int32 * 4)()
    assert lib.omr_pyramid_level_sizes(8, 8, 2, None) == _lib.INVALID_ARGUMENT
    assert lib.omr_pyramid_level_sizes(0, 8, 1, out) == _lib.INVALID_ARGUMENT
    assert lib.omr_pyramid_level_sizes(8, -8, 1, out) == _lib.INVALID_ARGUMENT


# ---- the restatement checks itself ---------------------------------------------------------------
@pytest.mark.parametrize("pt", sorted(NP_TYPES))
def test_ref_mean_of_constant_is_constant(pt):
    dt = NP_TYPES[pt]
    values = [1.5, -3.25, 0.0] if np.issubdtype(dt, np.floating) else \
        [np.iinfo(dt).min, np.iinfo(dt).max, 0, 1, np.iinfo(dt).max - 1]
    for v in values:
        plane = np.full((13, 22), v, dtype=dt)
        for lv in pyramid_ref(plane, MEAN, 4):
            assert lv.dtype == dt and np.all(lv == dt(v))


def test_ref_int8_rounds_half_up_with_floor():
    assert pyramid_ref(np.array([[-1, -1], [-1, -2]], np.int8), MEAN, 2)[1].tolist() == [[-1]]   # floor(-1.25 + .5)
    assert pyramid_ref(np.array([[-1, -2], [-2, -2]], np.int8), MEAN, 2)[1].tolist() == [[-2]]   # floor(-1.75 + .5)
    assert pyramid_ref(np.array([[1, 2], [2, 2]], np.uint8), MEAN, 2)[1].tolist() == [[2]]       # 1.75 + .5
    assert pyramid_ref(np.array([[1, 1], [2, 2]], np.uint8), MEAN, 2)[1].tolist() == [[2]]       # the half, up
    assert pyramid_ref(np.array([[-1, -1], [-2, -2]], np.int16), MEAN, 2)[1].tolist() == [[-1]]  # -1.5 -> -1


def test_ref_uint32_does_not_wrap():
    m = 2**32 - 1
    assert pyramid_ref(np.array([[m, m], [m, m - 1]], np.uint32), MEAN, 2)[1].tolist() == [[m]]
    assert pyramid_ref(np.array([[m, m - 3], [m - 1, m - 2]], np.uint32), MEAN, 2)[1].tolist() == [[m - 1]]
    lo = -2**31
    assert pyramid_ref(np.array([[lo, lo], [lo, lo + 1]], np.int32), MEAN, 2)[1].tolist() == [[lo]]


def test_ref_subsample_is_strided_level0():
    rng = np.random.default_rng(3)
    plane = rng.integers(0, 65536, (2, 45, 83), dtype=np.uint16)
    levels = pyramid_ref(plane, SUB, 6)
    for k, lv in enumerate(levels):
        assert lv.shape == (2, 45 >> k, 83 >> k)
        assert np.array_equal(lv, plane[:, ::2**k, ::2**k][:, :45 >> k, :83 >> k])


def test_ref_float_through_double_and_nan():
    # 1 + 2^-24 + 2^-24 + 0 in float would lose both small terms; through double the sum is exact
    a = np.array([[1.0, 2.0**-24], [2.0**-24, 0.0]], np.float32)
    want = np.float32((1.0 + 2.0**-23) * 0.25)
    assert pyramid_ref(a, MEAN, 2)[1][0, 0] == want != np.float32(0.25)
    b = np.array([[np.nan, 1.0], [2.0, 3.0]], np.float32)
    assert np.isnan(pyramid_ref(b, MEAN, 2)[1][0, 0])
    assert pyramid_ref(np.array([[np.inf, 1], [2, 3]], np.float64), MEAN, 2)[1][0, 0] == np.inf


# ---- sidecar, attach, level views ----------------------------------------------------------------------
SX, SY, SZ, SC, ST = 37, 21, 2, 3, 2


@pytest.fixture(scope="module")
def image(tmp_path_factory):
    d = tmp_path_factory.mktemp("pyr")
    rng = np.random.default_rng(9)
    px = rng.integers(0, 65536, (ST, SC, SZ, SY, SX), dtype=np.uint16)
    levels = pyramid_ref(px, MEAN, 3)
    write_romio(d / "pixels", px, _lib.PIXELS_UINT16)
    write_pyramid(d / "pixels_pyramid", levels[1:], _lib.PIXELS_UINT16, rule=MEAN, size=(SX, SY))
    return d, levels


def open_image(d):
    return PixelBuffer(d / "pixels", SX, SY, SZ, SC, ST, _lib.PIXELS_UINT16)


def test_sidecar_layout(image):
    d, levels = image
    raw = (d / "pixels_pyramid").read_bytes()
    assert raw[:8] == b"OMRPYR1\0"
    assert np.frombuffer(raw[8:24], "<u4").tolist() == [1, MEAN, _lib.PIXELS_UINT16, 3]
    assert np.frombuffer(raw[24:44], "<i4").tolist() == [SX, SY, SZ, SC, ST]
    assert raw[44:4096] == bytes(4096 - 44)
    n1 = levels[1].nbytes
    assert raw[4096:4096 + n1] == levels[1].astype(">u2").tobytes()
    off2 = -(-(4096 + n1) // 4096) * 4096
    assert raw[4096 + n1:off2] == bytes(off2 - 4096 - n1)
    assert raw[off2:] == levels[2].astype(">u2").tobytes()


def test_attach_levels_and_descriptions(image):
    d, _ = image
    with open_image(d) as pb:
        assert pb.getResolutionLevels() == 1 and pb.getResolutionDescriptions() == [[SX, SY]]
        pb.attach_pyramid(d / "pixels_pyramid")
        assert pb.getResolutionLevels() == 3
        assert pb.getResolutionDescriptions() == [[37, 21], [18, 10], [9, 5]]
        out = (ctypes.c_int32 * 2)()
        assert lib.omr_pixel_buffer_resolution_descriptions(pb.h, out, 1) == 3 and list(out) == [37, 21]
        assert lib.omr_pixel_buffer_resolution_descriptions(None, out, 1) == -_lib.INVALID_ARGUMENT
        assert lib.omr_pixel_buffer_resolution_levels(None) == 0


def test_level_views_return_the_levels(image):
    d, levels = image
    with open_image(d) as pb:
        pb.attach_pyramid(d / "pixels_pyramid")
        for k in range(3):
            with pb.level(k) as v:
                w, h = SX >> k, SY >> k
                assert (v.size_x, v.size_y, v.size_z, v.size_c, v.size_t) == (w, h, SZ, SC, ST)
                assert v.getResolutionLevels() == 1 and v.getResolutionDescriptions() == [[w, h]]
                plane_bytes = w * h * 2
                for t in range(ST):
                    for c in range(SC):
                        for z in range(SZ):
                            assert v.plane_offset(z, c, t) == ((t * SC + c) * SZ + z) * plane_bytes
                            assert np.array_equal(v.get_tile(z, c, t, 0, 0, w, h).astype(np.uint16), levels[k][t, c, z])
                            x, y, tw, th = w // 3, h // 2, w - w // 3 - 1, h - h // 2
                            assert np.array_equal(v.get_tile(z, c, t, x, y, tw, th).astype(np.uint16),
                                                  levels[k][t, c, z, y:y + th, x:x + tw])
                assert v.get_tile(1, 2, 1, w - 1, h - 1, 1, 1)[0, 0] == levels[k][1, 2, 1, h - 1, w - 1]


@pytest.mark.parametrize("bad", [(0, 0, 0, 17, 0, 2, 1), (0, 0, 0, 0, 10, 1, 1), (0, 0, 0, 0, 0, 19, 1),
                                 (2, 0, 0, 0, 0, 1, 1), (0, 3, 0, 0, 0, 1, 1), (0, 0, 2, 0, 0, 1, 1),
                                 (0, 0, 0, -1, 0, 1, 1)])
def test_level_view_out_of_bounds(image, bad):
    d, _ = image
    with open_image(d) as pb:
        pb.attach_pyramid(d / "pixels_pyramid")
        with pb.level(1) as v:                       # 18 x 10
            with pytest.raises(_lib.OmrError) as e:
                v.get_tile(*bad)
            assert e.value.status == _lib.INVALID_ARGUMENT
            assert v.plane_offset(2, 0, 0) == -1


def test_view_outlives_parent_and_serials_differ(image):
    d, levels = image
    pb = open_image(d)
    pb.attach_pyramid(d / "pixels_pyramid")
    v2, v0, v2b = pb.level(2), pb.level(0), pb.level(2)
    pb.close()
    assert np.array_equal(v2.get_tile(1, 1, 1, 0, 0, 9, 5).astype(np.uint16), levels[2][1, 1, 1])
    assert np.array_equal(v0.get_tile(0, 2, 0, 3, 4, 30, 10).astype(np.uint16), levels[0][0, 2, 0, 4:14, 3:33])
    v2.close()
    assert np.array_equal(v2b.get_tile(0, 0, 0, 0, 0, 9, 5).astype(np.uint16), levels[2][0, 0, 0])
    v2b.close()
    v0.close()


def test_no_sidecar_one_level(image):
    d, _ = image
    with open_image(d) as pb:
        assert pb.getResolutionLevels() == 1
        with pb.level(0) as v:
            assert v.size_x == SX
        for r in (1, -1, 3):
            with pytest.raises(_lib.OmrError) as e:
                pb.level(r)
            assert e.value.status == _lib.INVALID_ARGUMENT
        pb.attach_pyramid(d / "pixels_pyramid")
        with pytest.raises(_lib.OmrError) as e:
            pb.level(3)
        assert e.value.status == _lib.INVALID_ARGUMENT
        view = ctypes.c_void_p()
        assert lib.omr_pixel_buffer_level(None, 0, ctypes.byref(view)) == _lib.INVALID_ARGUMENT
        assert lib.omr_pixel_buffer_level(pb.h, 0, None) == _lib.INVALID_ARGUMENT


def _patched(raw, off, fmt, value):
    b = bytearray(raw)
    b[off:off + 4] = np.array([value], fmt).tobytes()
    return bytes(b)


@pytest.mark.parametrize("name", ["truncated", "longer", "magic", "version", "rule", "type", "size_x", "size_y", "size_z",
                                  "size_c", "size_t", "n_levels_past_bound", "n_levels_zero", "header_only", "empty"])
def test_rejected_sidecars(image, tmp_path, name):
    d, _ = image
    raw = (d / "pixels_pyramid").read_bytes()
    bad = {
        "truncated": raw[:-1], "longer": raw + b"\0", "magic": b"OMRPYR2\0" + raw[8:],
        "version": _patched(raw, 8, "<u4", 2), "rule": _patched(raw, 12, "<u4", 2),
        "type": _patched(raw, 16, "<u4", _lib.PIXELS_INT16), "size_x": _patched(raw, 24, "<i4", SX + 1),
        "size_y": _patched(raw, 28, "<i4", SY - 1), "size_z": _patched(raw, 32, "<i4", SZ + 1),
        "size_c": _patched(raw, 36, "<i4", 1), "size_t": _patched(raw, 40, "<i4", 0),
        "n_levels_past_bound": _patched(raw, 20, "<u4", 6),      # 1 + floor(log2(21)) = 5
        "n_levels_zero": _patched(raw, 20, "<u4", 0), "header_only": raw[:64], "empty": b"",
    }[name]
    p = tmp_path / "bad"
    p.write_bytes(bad)
    with open_image(d) as pb:
        with pytest.raises(_lib.OmrError) as e:
            pb.attach_pyramid(p)
        assert e.value.status == _lib.INVALID_ARGUMENT
        assert pb.getResolutionLevels() == 1


def test_missing_sidecar_and_one_level_sidecar(image, tmp_path):
    d, _ = image
    with open_image(d) as pb:
        with pytest.raises(_lib.OmrError) as e:
            pb.attach_pyramid(tmp_path / "none")
        assert e.value.status == _lib.NOT_FOUND
        assert lib.omr_pixel_buffer_attach_pyramid(pb.h, None) == _lib.INVALID_ARGUMENT
        write_pyramid(tmp_path / "one", [], _lib.PIXELS_UINT16, size=(SX, SY))   # no levels: only level 0
        raw = bytearray((tmp_path / "one").read_bytes())
        raw[32:44] = np.array([SZ, SC, ST], "<i4").tobytes()
        (tmp_path / "one").write_bytes(bytes(raw))
        pb.attach_pyramid(tmp_path / "one")
        assert pb.getResolutionLevels() == 1


def test_region_def_from_attached_descriptions(image):
    d, _ = image
    with open_image(d) as pb:
        pb.attach_pyramid(d / "pixels_pyramid")
        levels = pb.getResolutionDescriptions()
        flat = (ctypes.c_int32 * 6)(*[v for lv in levels for v in lv])
        req, out = _lib.Region(1, 0, 4, 4), _lib.Region()
        # tile=2,1,0,4,4: level 2 is 9 x 5; tile (1, 0) of 4 x 4 starts at x = 4, y = 0 and is cut
        # to the level: width min(4, 9 - 4) = 4, height min(4, 5 - 0) = 4
        assert lib.omr_get_region_def(0, ctypes.byref(req), 2, flat, 3, 256, 256, 2048, 0, 0, ctypes.byref(out)) == 0
        assert (out.x, out.y, out.width, out.height) == (4, 0, 4, 4)
        req = _lib.Region(2, 1, 4, 4)       # the corner tile: x = 8, y = 4 -> 1 x 1 left
        assert lib.omr_get_region_def(0, ctypes.byref(req), 2, flat, 3, 256, 256, 2048, 0, 0, ctypes.byref(out)) == 0
        assert (out.x, out.y, out.width, out.height) == (8, 4, 1, 1)
        assert lib.omr_resolution_level(3, 2) == 0       # the omeis level of the smallest description
