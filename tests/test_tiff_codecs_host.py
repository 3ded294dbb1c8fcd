"""The forms omr_tiff_image_open_ex adds to the TIFF reader, host side: Deflate and zstd segments,
the floating-point predictor and chunky pixels of several samples.  Files libtiff wrote (the golden
fixture) and files of the project's writer (tiff_codec_cases.CASES) open with the right `accept`,
report what they hold and read back through get_tile exactly; every form is refused without its
bit; damaged segments answer OMR_INTERNAL on that segment alone; and Pillow reads the writer's
Deflate and Predictor 3 files.  No GPU; no tolerance anywhere."""
import ctypes
import struct
import zlib

import numpy as np
import pytest

import omr
import tiff_codec_cases as tc
from omr import _lib

TYPES = {"int8": _lib.PIXELS_INT8, "uint8": _lib.PIXELS_UINT8, "int16": _lib.PIXELS_INT16,
         "uint16": _lib.PIXELS_UINT16, "int32": _lib.PIXELS_INT32, "uint32": _lib.PIXELS_UINT32,
         "float32": _lib.PIXELS_FLOAT, "float64": _lib.PIXELS_DOUBLE}


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return tc.Files(tmp_path_factory.mktemp("tiff_codecs"))


@pytest.fixture(scope="module")
def golden(tmp_path_factory):
    return tc.load_golden(tmp_path_factory.mktemp("tiff_golden"))


def status_of(fn):
    with pytest.raises(omr.OmrError) as e:
        fn()
    return e.value.status


def same(tile, want):
    return tile.tobytes() == np.ascontiguousarray(want.astype(tile.dtype)).tobytes()


# ---- files of libtiff --------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(tc.GOLDEN_FILES))
def test_golden_files(golden, name):
    path, px = golden[name]
    dtype, spp, comp, pred, _ = tc.GOLDEN_FILES[name]
    need = tc.golden_need(name)
    with omr.TiffImage(path, 1, spp, 1, accept=need) as img:
        assert img.info["compression"] == (50000 if comp == "zstd" else 8) and img.info["predictor"] == pred
        assert img.samples_per_pixel == spp and img.size_c == spp and img.pixel_type == TYPES[dtype]
        assert not img.info["tiled"] and img.info["segment_height"] == 32      # the last strip has 6 rows
        for c in range(spp):
            assert same(img.get_tile(0, 0, c, 0, 0, 0, tc.W, tc.H), px[c])
            assert same(img.get_tile(0, 0, c, 0, 7, 20, 101, 47), px[c, 20:67, 7:108])
            assert same(img.get_tile(0, 0, c, 0, 149, 69, 1, 1), px[c, 69:, 149:])
    assert status_of(lambda: omr.TiffImage(path, 1, spp, 1)) == _lib.INVALID_ARGUMENT
    for drop in need:                                        # every bit the file needs is needed
        rest = tuple(n for n in tc.ACCEPT_ALL if n != drop)
        assert status_of(lambda: omr.TiffImage(path, 1, spp, 1, accept=rest)) == _lib.INVALID_ARGUMENT, drop
    with omr.TiffImage(path, 1, spp, 1, accept=tc.ACCEPT_ALL):
        pass


# ---- files of the project's writer ---------------------------------------------------------------------

def test_cases_cover_the_forms():
    seen = {(c.dtype, c.compression) for c in tc.CASES if c.spp == 1}
    for dtype in tc.NAMES:
        assert (dtype, 8) in seen and (dtype, 50000) in seen
    for dtype in ("float32", "float64"):
        for bo in "<>":
            assert any(c.dtype == dtype and c.predictor == 3 and c.bo == bo for c in tc.CASES)
    for spp in (3, 4):
        for dtype in ("uint8", "uint16"):
            for pred in (1, 2):
                for bo in "<>":
                    assert any((c.spp, c.dtype, c.predictor, c.bo) == (spp, dtype, pred, bo) for c in tc.CASES)
    assert any(c.zero_rows for c in tc.CASES) and any(c.compression == 32946 for c in tc.CASES)
    assert {c.strips for c in tc.CASES} == {False, True} and {c.bigtiff for c in tc.CASES} == {False, True}


@pytest.mark.parametrize("case", tc.CASES, ids=repr)
def test_written_files(files, case):
    path, lv0, lv1, _ = files.get(case)
    with case.open(path) as img:
        i = img.info
        assert i["compression"] == (8 if case.compression == 32946 else case.compression)
        assert i["predictor"] == case.predictor and img.samples_per_pixel == case.spp
        assert img.size_c == case.size_c and img.pixel_type == TYPES[case.dtype]
        assert img.big_endian == (case.bo == ">") and bool(i["big_tiff"]) == case.bigtiff
        assert bool(i["tiled"]) == (not case.strips)
        assert (i["segment_width"], i["segment_height"]) == ((tc.W, 16) if case.strips else (80, 16))
        assert img.level_sizes == [[tc.W, tc.H], [tc.LW, tc.LH]]
        for level, a in ((0, lv0), (1, lv1)):
            h, w = a.shape[-2:]
            for c in range(case.size_c):
                assert same(img.get_tile(level, 0, c, 0, 0, 0, w, h), a[0, c, 0]), (level, c)
                # crops that begin inside a segment and end before its last column
                for (x, y, cw, ch) in ((5, 3, 60, 9), (70, 14, 5, 20), (w - 9, h - 11, 7, 10), (1, 17, w - 2, 2)):
                    assert same(img.get_tile(level, 0, c, 0, x, y, cw, ch), a[0, c, 0, y:y + ch, x:x + cw]), (level, c, x, y)
    # refused by the plain open and without any one of its bits
    assert status_of(lambda: omr.TiffImage(path, 1, case.size_c, 1)) == _lib.INVALID_ARGUMENT
    for drop in case.need:
        rest = tuple(n for n in tc.ACCEPT_ALL if n != drop)
        assert status_of(lambda: case.open(path, accept=rest)) == _lib.INVALID_ARGUMENT, drop


def test_zero_count_segments_are_in_the_file(files):
    for case in tc.CASES:
        if not case.zero_rows or case.bigtiff or case.bo != "<":
            continue
        path, _, _, res = files.get(case)
        raw = open(path, "rb").read()
        offs, cnts, n = tc.segment_table(raw, res["ifds"][0])
        counts = struct.unpack_from("<%dI" % n, raw, cnts)
        per_row = 1 if case.strips else 2
        assert all(c == 0 for c in counts[2 * per_row:3 * per_row]) and all(c > 0 for c in counts[:2 * per_row])


# ---- refusals ------------------------------------------------------------------------------------------

def _open_ex(path, size_c, struct_size, accept):
    h = ctypes.c_void_p()
    opt = _lib.TiffOpenOptions(struct_size, accept)
    st = _lib.lib.omr_tiff_image_open_ex(str(path).encode(), 1, size_c, 1, b"XYZCT", ctypes.byref(opt), ctypes.byref(h))
    if st == _lib.OK:
        _lib.lib.omr_tiff_image_close(h)
    else:
        assert not h.value
    return st


def test_options(files, tmp_path):
    path = files.get(tc.CASE_BY_NAME["uint16-32946-p2-le-tiles"])[0]
    size = ctypes.sizeof(_lib.TiffOpenOptions)
    assert size == 8
    assert _open_ex(path, 2, size, 1) == _lib.OK
    assert _open_ex(path, 2, size + 8, 15) == _lib.OK             # a later, larger struct
    assert _open_ex(path, 2, size, 16) == _lib.INVALID_ARGUMENT    # unknown bits
    assert _open_ex(path, 2, size, 1 | 1 << 31) == _lib.INVALID_ARGUMENT
    assert _open_ex(path, 2, size - 1, 1) == _lib.INVALID_ARGUMENT
    assert _open_ex(path, 2, 0, 1) == _lib.INVALID_ARGUMENT
    assert _open_ex(path, 2, size, 2) == _lib.INVALID_ARGUMENT     # zstd alone does not admit Deflate
    assert status_of(lambda: omr.TiffImage(path, 1, 2, 1, accept=("lzma",))) == _lib.INVALID_ARGUMENT
    # a file that uses none of the forms opens with any accept, and as before with none
    a = tc.pixels("uint16", 2, tc.W, tc.H, 1)
    omr.write_tiled_tiff(tmp_path / "plain.tif", a, tile=(80, 16), compression=5, predictor=2)
    with omr.TiffImage(tmp_path / "plain.tif", 1, 2, 1, accept=tc.ACCEPT_ALL) as img, \
            omr.TiffImage(tmp_path / "plain.tif", 1, 2, 1) as plain:
        assert img.samples_per_pixel == plain.samples_per_pixel == 1
        assert img.get_tile(0, 0, 1, 0, 0, 0, tc.W, tc.H).tobytes() == plain.get_tile(0, 0, 1, 0, 0, 0, tc.W, tc.H).tobytes()
    assert _lib.lib.omr_tiff_image_samples_per_pixel(None) < 0


def test_refused_files(tmp_path):
    every = tc.ACCEPT_ALL
    path = tmp_path / "r.tif"
    rgb = tc.pixels("uint8", 6, tc.W, tc.H, 2)

    def refused(size_c=6, **kw):
        return status_of(lambda: omr.TiffImage(path, 1, size_c, 1, accept=every)) == _lib.INVALID_ARGUMENT

    omr.write_tiled_tiff(path, rgb, tile=(80, 16), compression=8, samples_per_pixel=3)
    with omr.TiffImage(path, 1, 6, 1, accept=every) as img:
        assert img.samples_per_pixel == 3
    for size_c in (4, 5, 7, 2, 1):                           # size_c not a multiple of spp
        assert refused(size_c), size_c
    assert refused(9)                                        # fewer IFDs than Z * (C / spp) * T
    with omr.TiffImage(path, 1, 3, 1, accept=every) as img:  # fewer planes than the file has: fine, as ever
        assert img.size_c == 3
    omr.write_tiled_tiff(path, rgb, tile=(80, 16), compression=8, samples_per_pixel=3, tag_overrides={284: 2})
    assert refused()                                         # PlanarConfiguration 2
    omr.write_tiled_tiff(path, rgb, tile=(80, 16), compression=8, samples_per_pixel=3, tag_overrides={262: 6})
    assert refused()                                         # YCbCr
    omr.write_tiled_tiff(path, tc.pixels("uint8", 5, 40, 20, 3), tile=(16, 16), samples_per_pixel=5)
    assert refused(5)                                        # more than 4 samples
    omr.write_tiled_tiff(path, tc.pixels("uint16", 2, 40, 20, 3), tile=(16, 16), tag_overrides={317: 3})
    assert refused(2)                                        # Predictor 3 on integers
    omr.write_tiled_tiff(path, tc.pixels("float32", 3, 40, 20, 3), tile=(16, 16), samples_per_pixel=3,
                         tag_overrides={317: 3})
    assert refused(3)                                        # Predictor 3 with several samples
    omr.write_tiled_tiff(path, tc.pixels("float64", 2, 40, 20, 3), tile=(16, 16), compression=8, tag_overrides={317: 2})
    assert refused(2)                                        # Predictor 2 on 64-bit samples stays refused
    omr.write_tiled_tiff(path, tc.pixels("uint8", 2, 40, 20, 3), tile=(16, 16), tag_overrides={259: 7})
    assert refused(2)                                        # JPEG: no bit admits it
    # samples of different widths (BitsPerSample 8, 8, 16)
    omr.write_tiled_tiff(path, rgb, tile=(80, 16), samples_per_pixel=3)
    raw = bytearray(path.read_bytes())
    at = raw.index(struct.pack("<HHI", 258, 3, 3))
    where = struct.unpack_from("<I", raw, at + 8)[0]
    assert struct.unpack_from("<3H", raw, where) == (8, 8, 8)
    struct.pack_into("<H", raw, where + 4, 16)
    path.write_bytes(raw)
    assert refused()


# ---- damaged segments -------------------------------------------------------------------------------------

@pytest.mark.parametrize("comp", [8, 50000])
@pytest.mark.parametrize("how", ["truncated", "bit"])
def test_damaged_segment(tmp_path, comp, how):
    a = tc.pixels("uint16", 2, tc.W, tc.H, 5)
    path = tmp_path / "d.tif"
    res = omr.write_tiled_tiff(path, a, tile=(80, 16), compression=comp, predictor=2)
    raw = bytearray(path.read_bytes())
    offs, cnts, n = tc.segment_table(raw, res["ifds"][0])
    k = 3                                                    # tile (1, 1) of plane 0
    off, cnt = struct.unpack_from("<I", raw, offs + 4 * k)[0], struct.unpack_from("<I", raw, cnts + 4 * k)[0]
    if how == "truncated":
        struct.pack_into("<I", raw, cnts + 4 * k, cnt // 2)
    else:
        raw[off + cnt // 2] ^= 0x10
    path.write_bytes(raw)
    with omr.TiffImage(path, 1, 2, 1, accept=("deflate", "zstd")) as img:
        assert status_of(lambda: img.get_tile(0, 0, 0, 0, 80, 16, 70, 16)) == _lib.INTERNAL
        assert status_of(lambda: img.get_tile(0, 0, 0, 0, 0, 0, tc.W, tc.H)) == _lib.INTERNAL
        # that segment only: its neighbours and the other plane read
        assert same(img.get_tile(0, 0, 0, 0, 0, 16, 80, 16), a[0, 0, 0, 16:32, :80])
        assert same(img.get_tile(0, 0, 0, 0, 80, 32, 70, 38), a[0, 0, 0, 32:, 80:])
        assert same(img.get_tile(0, 0, 1, 0, 0, 0, tc.W, tc.H), a[0, 1, 0])


def test_trailing_bytes_are_refused(tmp_path):
    """The strict rule: a stream must end where the segment's bytes end (LZW cuts; these do not)."""
    a = tc.pixels("uint8", 1, tc.W, tc.H, 6)
    path = tmp_path / "t.tif"
    seg = a[0, 0, 0, :16, :80].tobytes()
    for comp, encode in ((8, zlib.compress), (50000, omr.zstd_encode)):
        for data, ok in ((seg, True), (seg + b"\0", False), (seg[:-1], False)):
            res = omr.write_tiled_tiff(path, a, tile=(80, 16), compression=comp)
            raw = bytearray(path.read_bytes())
            offs, cnts, n = tc.segment_table(raw, res["ifds"][0])
            stream = encode(data)
            struct.pack_into("<I", raw, offs, len(raw))      # tile (0, 0): a stream of its own behind the file
            struct.pack_into("<I", raw, cnts, len(stream))
            path.write_bytes(bytes(raw) + stream)
            with omr.TiffImage(path, 1, 1, 1, accept=("deflate", "zstd")) as img:
                if ok:
                    assert same(img.get_tile(0, 0, 0, 0, 0, 0, 80, 16), a[0, 0, 0, :16, :80])
                else:
                    assert status_of(lambda: img.get_tile(0, 0, 0, 0, 0, 0, 80, 16)) == _lib.INTERNAL, (comp, len(data))
                assert same(img.get_tile(0, 0, 0, 0, 80, 0, 70, 16), a[0, 0, 0, :16, 80:])


# ---- the writer against libtiff ----------------------------------------------------------------------------

def _pil():
    Image = pytest.importorskip("PIL.Image")
    features = pytest.importorskip("PIL.features")
    if not features.check("libtiff"):
        pytest.skip("Pillow without libtiff")
    return Image


@pytest.mark.parametrize("what", ["uint8-8-p1", "uint16-8-p2", "uint16-32946-p1", "float32-8-p3", "float32-50000-p3",
                                  "uint8x3-8-p2", "uint8-50000-p2"])
def test_writer_read_by_libtiff(tmp_path, what):
    """(Compressed files only: Pillow reads stored segments with a decoder of its own, without libtiff.)"""
    Image = _pil()
    name, comp, pred = what.split("-")
    spp = 3 if name.endswith("x3") else 1
    dtype = name.split("x")[0]
    a = tc.pixels(dtype, 2 * spp, 100, 70, zlib.crc32(what.encode()))
    omr.write_tiled_tiff(tmp_path / "w.tif", a, tile=(32, 16), compression=int(comp), predictor=int(pred[1:]),
                         samples_per_pixel=spp)
    with Image.open(tmp_path / "w.tif") as im:
        assert im.n_frames == 2
        for k in range(2):
            im.seek(k)
            got = np.array(im)
            want = a[0, k, 0] if spp == 1 else np.moveaxis(a[0, 3 * k:3 * k + 3, 0], 0, -1)
            assert got.tobytes() == np.ascontiguousarray(want).tobytes(), k


def test_writer_defaults_unchanged(tmp_path):
    """samples_per_pixel = 1 and the old codecs: the bytes of the file do not depend on the new arguments."""
    a = tc.pixels("uint16", 2, 100, 70, 9)
    omr.write_tiled_tiff(tmp_path / "a.tif", a, tile=(32, 16), compression=5, predictor=2)
    omr.write_tiled_tiff(tmp_path / "b.tif", a, tile=(32, 16), compression=5, predictor=2, samples_per_pixel=1)
    raw = (tmp_path / "a.tif").read_bytes()
    assert raw == (tmp_path / "b.tif").read_bytes()
    n = struct.unpack_from("<H", raw, struct.unpack_from("<I", raw, 4)[0])[0]
    assert n == 13                                           # the entries it always wrote: no ExtraSamples, one value each
