"""Raw pixel tiles on the host (K12, no GPU): the raw TIFF writer for all eight pixel types read
back with a small baseline-TIFF reader (and PIL where PIL knows the type), its size bound, raw TIFF
tiles of ROMIO files and pyramid level views, the grey PNG batch's size bound against the formats'
own constants, and the argument errors of every call that needs no device."""
import ctypes
import io
import struct

import numpy as np
import pytest
from PIL import Image

import omr
from omr import PixelBuffer, _lib, write_pyramid, write_romio
from omr._lib import lib

NP_TYPES = {_lib.PIXELS_INT8: "i1", _lib.PIXELS_UINT8: "u1", _lib.PIXELS_INT16: "i2", _lib.PIXELS_UINT16: "u2",
            _lib.PIXELS_INT32: "i4", _lib.PIXELS_UINT32: "u4", _lib.PIXELS_FLOAT: "f4", _lib.PIXELS_DOUBLE: "f8"}
SAMPLE_FORMAT = {"u": 1, "i": 2, "f": 3}
# 300 x 200 uint8: 28 rows of 300 bytes per strip, 200 = 7 * 28 + 4 (an uneven last strip);
# 1000 x 37 uint16: 5 rows of 2000 bytes per strip, 37 = 7 * 5 + 2
SIZES = [(1, 1), (7, 3), (300, 200), (1000, 37)]
PIL_MODES = {_lib.PIXELS_UINT8: "L", _lib.PIXELS_UINT16: "I;16B", _lib.PIXELS_INT32: "I", _lib.PIXELS_FLOAT: "F"}


def pixels_of(pt, w, h, seed=0):
    rng = np.random.default_rng(seed + 17 * pt + w)
    kind = NP_TYPES[pt]
    if kind[0] == "f":
        return (rng.standard_normal((h, w)) * 1000).astype("=" + kind)
    info = np.iinfo(np.dtype(kind))
    a = rng.integers(info.min, int(info.max) + 1, (h, w), dtype=np.int64 if kind != "u4" else np.uint64)
    a.flat[0], a.flat[-1] = info.min, info.max
    return a.astype("=" + kind)


def read_baseline_tiff(data):
    """{tag: values} of the first IFD of a big-endian TIFF, and the concatenated strip bytes."""
    assert data[:4] == b"MM\x00\x2a"
    (ifd,) = struct.unpack(">I", data[4:8])
    (n,) = struct.unpack(">H", data[ifd:ifd + 2])
    tags, last = {}, 0
    for k in range(n):
        tag, typ, cnt = struct.unpack(">HHI", data[ifd + 2 + 12 * k:ifd + 10 + 12 * k])
        assert tag > last, "IFD entries ascend"
        last = tag
        size = {3: 2, 4: 4}[typ]
        field = data[ifd + 10 + 12 * k:ifd + 14 + 12 * k]
        raw = field[:size * cnt] if size * cnt <= 4 else data[struct.unpack(">I", field)[0]:][:size * cnt]
        tags[tag] = list(struct.unpack(">" + {3: "H", 4: "I"}[typ] * cnt, raw))
    assert struct.unpack(">I", data[ifd + 2 + 12 * n:ifd + 6 + 12 * n]) == (0,), "one IFD"
    strips = b"".join(data[o:o + c] for o, c in zip(tags[273], tags[279]))
    assert all(o + c <= len(data) for o, c in zip(tags[273], tags[279]))
    return tags, strips


def check_raw_tiff(data, a, pt):
    """The file `data` holds the native-order [h][w] array `a` of pixel type pt."""
    h, w = a.shape
    kind = NP_TYPES[pt]
    bps = int(kind[1])
    tags, strips = read_baseline_tiff(data)
    assert tags[256] == [w] and tags[257] == [h]
    assert tags[258] == [8 * bps]                        # BitsPerSample
    assert tags[259] == [1]                              # no compression
    assert tags[262] == [1]                              # BlackIsZero
    assert tags[277] == [1]                              # one sample per pixel
    assert tags[339] == [SAMPLE_FORMAT[kind[0]]]
    rps = tags[278][0]
    row = w * bps
    ns = (h + rps - 1) // rps
    assert len(tags[273]) == len(tags[279]) == ns
    assert rps == h or rps * row >= 8192                 # strips of at least 8 KiB
    assert rps == h or (rps - 1) * row < 8192            # ... and no more rows than that takes
    assert tags[279] == [min(rps, h - s * rps) * row for s in range(ns)]
    assert all(tags[273][s + 1] == tags[273][s] + tags[279][s] for s in range(ns - 1))
    assert strips == a.astype(">" + kind).tobytes()
    assert len(data) == tags[273][-1] + tags[279][-1]
    if pt in PIL_MODES:
        im = Image.open(io.BytesIO(data))
        assert im.mode == PIL_MODES[pt] and im.size == (w, h)
        assert np.array_equal(np.asarray(im).astype(a.dtype), a)


@pytest.mark.parametrize("pt", sorted(NP_TYPES))
@pytest.mark.parametrize("w,h", SIZES)
def test_encode_tiff_raw_all_types(pt, w, h):
    a = pixels_of(pt, w, h)
    files = []
    for order in (">", "<"):
        src = a.astype(order + NP_TYPES[pt])
        data = omr.encode_tiff_raw(src)
        check_raw_tiff(data, a, pt)
        assert len(data) == lib.omr_tiff_raw_max_bytes(w, h, pt)
        files.append(data)
        # the C call itself, with the byte order as its flag
        cap = lib.omr_tiff_raw_max_bytes(w, h, pt)
        out = np.zeros(cap + 8, np.uint8)
        out[cap:] = 0xA5
        n = ctypes.c_size_t(0)
        assert lib.omr_encode_tiff_raw(src.ctypes.data, pt, int(order == ">"), w, h, out.ctypes.data, cap,
                                       ctypes.byref(n)) == _lib.OK
        assert n.value == cap and out[:cap].tobytes() == data and (out[cap:] == 0xA5).all()
        n = ctypes.c_size_t(0)
        assert lib.omr_encode_tiff_raw(src.ctypes.data, pt, int(order == ">"), w, h, out.ctypes.data, cap - 1,
                                       ctypes.byref(n)) == _lib.BUFFER_TOO_SMALL
        assert n.value == cap
    assert files[0] == files[1]                          # both byte orders give the same file


def test_uneven_strips_are_in_the_cases():
    for (w, h), bps in (((300, 200), 1), ((1000, 37), 2)):
        rps = -(-8192 // (w * bps))
        assert 1 < rps < h and h % rps != 0


def test_encode_tiff_raw_argument_errors():
    a = np.zeros((4, 4), np.uint16)
    out = np.zeros(4096, np.uint8)
    n = ctypes.c_size_t(0)
    p, o = a.ctypes.data, out.ctypes.data
    U16 = _lib.PIXELS_UINT16
    assert lib.omr_encode_tiff_raw(None, U16, 1, 4, 4, o, 4096, ctypes.byref(n)) == _lib.INVALID_ARGUMENT
    for w, h in ((0, 4), (4, 0), (-1, 4), (65536, 1), (1, 65536)):
        assert lib.omr_encode_tiff_raw(p, U16, 1, w, h, o, 4096, ctypes.byref(n)) == _lib.INVALID_ARGUMENT
        assert lib.omr_tiff_raw_max_bytes(w, h, U16) == 0
    for pt in (-1, 8, 100):
        assert lib.omr_encode_tiff_raw(p, pt, 1, 4, 4, o, 4096, ctypes.byref(n)) == _lib.INVALID_ARGUMENT
        assert lib.omr_tiff_raw_max_bytes(4, 4, pt) == 0
    assert lib.omr_tiff_raw_max_bytes(65535, 65535, _lib.PIXELS_DOUBLE) == 0     # past 32-bit offsets
    assert lib.omr_encode_tiff_raw(p, U16, 1, 4, 4, None, 0, ctypes.byref(n)) == _lib.BUFFER_TOO_SMALL
    assert n.value == lib.omr_tiff_raw_max_bytes(4, 4, U16)
    assert lib.omr_encode_tiff_raw(p, U16, 1, 4, 4, o, 4096, None) == _lib.OK    # out_len is optional
    with pytest.raises(omr.OmrError):
        omr.encode_tiff_raw(np.zeros((2, 2, 2), np.uint8))
    with pytest.raises(omr.OmrError):
        omr.encode_tiff_raw(np.zeros((2, 2), np.complex64))


@pytest.fixture(scope="module")
def romio(tmp_path_factory):
    """A 2-t 3-c 2-z 41 x 29 int16 image as a ROMIO file, and its pixels."""
    d = tmp_path_factory.mktemp("raw_tile")
    rng = np.random.default_rng(5)
    px = rng.integers(-32768, 32768, (2, 3, 2, 29, 41)).astype(np.int16)
    path = d / "pixels.romio"
    write_romio(path, px, _lib.PIXELS_INT16)
    return d, path, px


def test_pixel_buffer_tile_tiff(romio):
    _, path, px = romio
    I16 = _lib.PIXELS_INT16
    with PixelBuffer(path, 41, 29, 2, 3, 2, I16) as pb:
        for (z, c, t, x, y, w, h) in ((0, 0, 0, 0, 0, 41, 29), (1, 2, 1, 5, 3, 16, 8), (1, 1, 0, 30, 20, 11, 9),
                                      (0, 2, 1, 40, 28, 1, 1)):          # whole plane, inner, edge, corner
            check_raw_tiff(pb.tile_tiff(z, c, t, x, y, w, h), px[t, c, z, y:y + h, x:x + w], I16)
        for bad in ((0, 0, 0, 31, 20, 11, 9), (0, 0, 0, 0, 21, 4, 9), (2, 0, 0, 0, 0, 4, 4), (0, 3, 0, 0, 0, 4, 4),
                    (0, 0, 2, 0, 0, 4, 4), (0, 0, 0, -1, 0, 4, 4), (0, 0, 0, 0, 0, 0, 4), (0, 0, 0, 0, 0, 4, 0)):
            with pytest.raises(omr.OmrError) as e:
                pb.tile_tiff(*bad)
            assert e.value.status == _lib.INVALID_ARGUMENT, bad
        n = ctypes.c_size_t(0)
        out = np.zeros(4096, np.uint8)
        cap = lib.omr_tiff_raw_max_bytes(16, 8, I16)
        assert lib.omr_pixel_buffer_tile_tiff(pb.h, 0, 0, 0, 0, 0, 16, 8, out.ctypes.data, cap - 1,
                                              ctypes.byref(n)) == _lib.BUFFER_TOO_SMALL
        assert n.value == cap
    assert lib.omr_pixel_buffer_tile_tiff(None, 0, 0, 0, 0, 0, 4, 4, out.ctypes.data, 4096,
                                          ctypes.byref(n)) == _lib.INVALID_ARGUMENT


def test_pixel_buffer_tile_tiff_level_view(romio):
    d, path, px = romio
    I16 = _lib.PIXELS_INT16
    lv1 = px[..., 0:28:2, 0:40:2].copy()                  # any [t][c][z][14][20] pixels serve
    lv2 = (lv1[..., 0:14:2, 0:20:2] // 3).astype(np.int16)
    side = d / "pixels.pyr"
    write_pyramid(side, [lv1, lv2], I16, size=(41, 29))
    with PixelBuffer(path, 41, 29, 2, 3, 2, I16) as pb:
        pb.attach_pyramid(side)
        for k, lv in ((1, lv1), (2, lv2)):
            with pb.level(k) as view:
                hh, ww = lv.shape[-2:]
                check_raw_tiff(view.tile_tiff(1, 2, 1, 0, 0, ww, hh), lv[1, 2, 1], I16)
                check_raw_tiff(view.tile_tiff(0, 1, 0, 3, 2, ww - 3, hh - 2), lv[0, 1, 0, 2:, 3:], I16)
                with pytest.raises(omr.OmrError):
                    view.tile_tiff(0, 0, 0, 1, 0, ww, hh)


# ---- the grey PNG batch's size bound ------------------------------------------------------------
def png_stored_file_bytes(w, h, bps):
    """A grey PNG whose IDAT is one zlib stream of stored deflate blocks (RFC 1950 / 1951, PNG 1.2)."""
    raw = (w * bps + 1) * h                               # a filter byte per row
    blocks = max(1, -(-raw // 65535))                     # stored blocks carry a 16-bit length
    zlib_bytes = 2 + 5 * blocks + raw + 4                 # CMF/FLG, 5 header bytes per block, Adler-32
    chunk = 4 + 4 + 4                                     # length, type, CRC
    return 8 + (chunk + 13) + (chunk + zlib_bytes) + chunk


@pytest.mark.parametrize("w,h", [(1, 1), (3, 5), (257, 3), (1024, 16), (1024, 1024), (4096, 3), (4096, 4096)])
@pytest.mark.parametrize("bps", [1, 2])
def test_png_gray_batch_max_bytes(w, h, bps):
    one = lib.omr_png_gray_batch_max_bytes(w, h, bps, 1)
    need = png_stored_file_bytes(w, h, bps)
    assert one >= need and one % 16 == 0
    assert one <= need + 512                              # and no wild over-estimate
    for n in (2, 37):
        assert lib.omr_png_gray_batch_max_bytes(w, h, bps, n) >= n * (need + 15) // 16 * 16
        assert lib.omr_png_gray_batch_max_bytes(w, h, bps, n) == n * one


def test_png_gray_argument_errors_without_a_device():
    mb = lib.omr_png_gray_batch_max_bytes
    assert mb(16, 16, 1, 0) == 0 and mb(16, 16, 1, -1) == 0
    assert mb(0, 16, 1, 1) == 0 and mb(16, 0, 2, 1) == 0
    assert mb(16, 16, 4, 1) == 0 and mb(16, 16, 8, 1) == 0 and mb(16, 16, 0, 1) == 0 and mb(16, 16, 3, 1) == 0
    # a null context never reaches the device
    tab = (_lib.RawTile * 1)()
    assert lib.omr_encode_png_gray_batch_device(None, ctypes.addressof(tab), 1, _lib.PIXELS_UINT8, 1, 4, 4, None, 0,
                                                None, None, None) == _lib.INVALID_ARGUMENT
    req = (_lib.RawTileRequest * 1)()
    assert lib.omr_pixel_buffer_tiles_png(None, None, ctypes.addressof(req), 1, 4, 4, None, 0, None, None,
                                          None) == _lib.INVALID_ARGUMENT
    assert ctypes.sizeof(_lib.RawTile) == 24 and _lib.RawTile.x.offset == 16
    assert ctypes.sizeof(_lib.RawTileRequest) == 20
    assert ctypes.sizeof(_lib.TileJob) == 88             # no batcher job for raw tiles
