"""JPEG-compressed TIFF segments on the host (K17): omr_tiff_image_open_ex with OMR_TIFF_ACCEPT_JPEG,
get_tile and omr_jpeg_decode_host against the pixels libtiff and libjpeg-turbo agree on
(tests/golden/tiff_jpeg.npz), byte for byte; the forms the fixture reaches
(omr_jpeg_stream_forms); what is refused (OMR_INVALID_ARGUMENT) and what counts as damage
(OMR_INTERNAL); and, with Pillow at hand, the files write_tiled_tiff(compression=7) makes."""
import struct

import numpy as np
import pytest

import omr
import tiff_jpeg_cases as jc
from omr import _lib


def regions(W, H):
    """Whole image, and regions across segment borders (segments are 16 rows tall, tiles 80 wide)."""
    return [(0, 0, W, H), (W // 2 - 20, 9, 41, 29), (0, 15, W, 2), (W - 1, H - 1, 1, 1), (79, 15, 2, 2), (3, H - 12, W - 5, 12)]


@pytest.mark.parametrize("name", jc.NAMES)
def test_get_tile_equals_stored_pixels(tmp_path, name):
    px = jc.pixels(name)
    n, H, W = px.shape
    with omr.TiffImage(jc.write(tmp_path, name), 1, n, 1, accept=jc.ACCEPT) as img:
        assert (img.size_x, img.size_y, img.size_c, img.samples_per_pixel) == (W, H, n, n)
        assert img.info["compression"] == 7 and img.pixel_type == _lib.PIXELS_UINT8
        for c in range(n):
            for (x, y, w, h) in regions(W, H):
                got = img.get_tile(0, 0, c, 0, x, y, w, h)
                assert got.tobytes() == np.ascontiguousarray(px[c, y:y + h, x:x + w]).tobytes(), (c, x, y, w, h)


@pytest.mark.parametrize("name", jc.NAMES)
def test_decode_host_equals_stored_pixels_per_segment(name):
    tables, segs, n, ycc = jc.streams_of(name)
    for (x, y, w, h, stream) in segs:
        got = omr.jpeg_decode_host(stream, w, h, n, ycc, tables)
        want = jc.expected_segment(name, x, y, w, h)
        assert np.array_equal(got[:want.shape[0], :want.shape[1]], want), (x, y)


def test_fixture_reaches_every_form():
    met = set()
    for name in jc.NAMES:
        tables, segs, _, _ = jc.streams_of(name)
        for seg in segs:
            met |= omr.jpeg_stream_forms(seg[4], tables)
    assert not [f for f in jc.FORMS if f not in met], met
    assert {"MULTI_TABLE", "COM", "FILL_BYTES", "TABLES_STREAM"} <= met
    bits = _lib.ctypes.c_uint32()
    assert _lib.lib.omr_jpeg_stream_forms(None, 0, None, 4, bits) == _lib.INVALID_ARGUMENT
    assert _lib.lib.omr_jpeg_stream_forms(None, 0, b"abcd", 4, bits) == _lib.INTERNAL


def status_of(fn):
    with pytest.raises(omr.OmrError) as e:
        fn()
    return e.value.status, str(e.value)


def test_open_refusals(tmp_path):
    grey, rgb = jc.write(tmp_path, "grey_strips"), jc.write(tmp_path, "ycc420_tiles")
    assert status_of(lambda: omr.TiffImage(grey))[0] == _lib.INVALID_ARGUMENT                       # the plain open
    assert status_of(lambda: omr.TiffImage(grey, accept=("deflate", "zstd")))[0] == _lib.INVALID_ARGUMENT
    assert status_of(lambda: omr.TiffImage(rgb, 1, 3, 1, accept=("jpeg",)))[0] == _lib.INVALID_ARGUMENT   # no samples bit
    assert status_of(lambda: omr.TiffImage(rgb, 1, 3, 1, accept=("samples",)))[0] == _lib.INVALID_ARGUMENT
    omr.TiffImage(grey, accept=("jpeg",)).close()
    # Compression 6, old-style JPEG, stays refused; so does YCbCr with any other compression
    data = bytearray(jc.raw("grey_strips"))
    struct.pack_into("<H", data, jc.ifd_of(data)[259][0], 6)
    assert status_of(lambda: omr.TiffImage(jc.write(tmp_path, "old", data), accept=jc.ACCEPT))[0] == _lib.INVALID_ARGUMENT
    data = bytearray(jc.raw("ycc444_tiles"))
    struct.pack_into("<H", data, jc.ifd_of(data)[259][0], 8)
    path = jc.write(tmp_path, "ycc_deflate", data)
    assert status_of(lambda: omr.TiffImage(path, 1, 3, 1, accept=jc.ACCEPT + ("deflate",)))[0] == _lib.INVALID_ARGUMENT
    # sixteen bits per sample with Compression 7
    data = bytearray(jc.raw("grey_strips"))
    struct.pack_into("<H", data, jc.ifd_of(data)[258][0], 16)
    assert status_of(lambda: omr.TiffImage(jc.write(tmp_path, "deep", data), accept=jc.ACCEPT))[0] == _lib.INVALID_ARGUMENT


@pytest.mark.parametrize("variant,word", [(jc.as_progressive, "progressive"), (jc.as_12bit, "12-bit"),
                                          (jc.as_two_scans, "more than one scan")])
def test_unsupported_forms_are_invalid_argument(tmp_path, variant, word):
    tables, segs, n, ycc = jc.streams_of("ycc420_tiles")
    x, y, w, h, stream = segs[1]
    omr.jpeg_decode_host(stream, w, h, n, ycc, tables)
    st, msg = status_of(lambda: omr.jpeg_decode_host(variant(stream), w, h, n, ycc, tables))
    assert st == _lib.INVALID_ARGUMENT and word in msg, msg
    if len(variant(stream)) == len(stream):                  # and through the file
        with omr.TiffImage(jc.write(tmp_path, "v", jc.patched_file("ycc420_tiles", 1, variant)), 1, 3, 1, accept=jc.ACCEPT) as img:
            assert status_of(lambda: img.get_tile(0, 0, 0, 0, 80, 0, 16, 16))[0] == _lib.INVALID_ARGUMENT
            img.get_tile(0, 0, 0, 0, 0, 0, 16, 16)           # the other segments read


def test_four_components_and_other_samplings_are_invalid_argument():
    tables, segs, n, ycc = jc.streams_of("ycc420_tiles")
    x, y, w, h, stream = segs[0]
    s = bytearray(stream)
    s[jc.marker_at(s, 0xC0) + 11] = 0x12                     # luma 1 x 2: 4:4:0
    st, msg = status_of(lambda: omr.jpeg_decode_host(bytes(s), w, h, n, ycc, tables))
    assert st == _lib.INVALID_ARGUMENT and "sampling" in msg
    s = bytearray(stream)
    s[jc.marker_at(s, 0xDB) + 4] |= 0x10                     # Pq = 1: 16-bit entries
    st, msg = status_of(lambda: omr.jpeg_decode_host(bytes(s), w, h, n, ycc, tables))
    assert st == _lib.INVALID_ARGUMENT and "16-bit" in msg


DAMAGE = [("ycc420_tiles", lambda s: s[:len(s) // 2]), ("ycc420_tiles", lambda s: s[:-2]),
          ("ycc420_tiles", jc.with_undefined_code), ("grey_strips", jc.with_undefined_code),
          ("ycc420_rst_q30", jc.with_swapped_rst), ("ycc420_tiles", jc.with_wrong_frame_size)]


@pytest.mark.parametrize("name,variant", DAMAGE, ids=["half", "no-eoi", "code", "code-grey", "rst", "frame"])
def test_damage_is_internal(tmp_path, name, variant):
    tables, segs, n, ycc = jc.streams_of(name)
    x, y, w, h, stream = segs[1]
    assert status_of(lambda: omr.jpeg_decode_host(variant(stream), w, h, n, ycc, tables))[0] == _lib.INTERNAL
    if len(variant(stream)) == len(stream):
        with omr.TiffImage(jc.write(tmp_path, "d", jc.patched_file(name, 1, variant)), 1, n, 1, accept=jc.ACCEPT) as img:
            assert status_of(lambda: img.get_tile(0, 0, 0, 0, x, y, 8, 8))[0] == _lib.INTERNAL
            good = segs[0]
            assert img.get_tile(0, 0, 0, 0, good[0], good[1], 8, 8).tobytes() == \
                np.ascontiguousarray(jc.pixels(name)[0, good[1]:good[1] + 8, good[0]:good[0] + 8]).tobytes()


def test_missing_table_and_every_truncation():
    tables, segs, n, ycc = jc.streams_of("ycc420_tiles_shared")
    x, y, w, h, stream = segs[0]
    assert tables and status_of(lambda: omr.jpeg_decode_host(stream, w, h, n, ycc, None))[0] == _lib.INTERNAL
    for cut in range(1, len(stream)):                        # a cut stream is never good, and never read past its end
        assert status_of(lambda: omr.jpeg_decode_host(stream[:cut], w, h, n, ycc, tables))[0] == _lib.INTERNAL
    assert status_of(lambda: omr.jpeg_decode_host(stream, w, h, n, ycc, tables[:len(tables) // 2]))[0] == _lib.INTERNAL


def test_written_files_read_back_as_pillow_decodes_them(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(7)
    a = np.clip(np.add.outer(np.arange(70), np.arange(150))[None, :, :] + rng.integers(-20, 21, (3, 70, 150)), 0, 255)
    a = a.astype(np.uint8)[None, :, None]                    # [t][c][z][y][x]
    cases = [dict(tile=(80, 16), jpeg=dict(subsampling="4:2:0", tables="shared", restart_blocks=2)),
             dict(tile=(64, 32), jpeg=dict(subsampling="4:2:2", tables="inline", optimize=True)),
             dict(rows_per_strip=16, jpeg=dict(subsampling="4:4:4", tables="shared", quality=95)),
             dict(rows_per_strip=32, jpeg=dict(photometric="rgb", tables="inline"))]
    for k, kw in enumerate(cases):
        path = tmp_path / ("w%d.tif" % k)
        omr.write_tiled_tiff(path, a, compression=7, samples_per_pixel=3, **kw)
        want = np.asarray(Image.open(path))
        with omr.TiffImage(path, 1, 3, 1, accept=jc.ACCEPT) as img:
            for c in range(3):
                assert np.array_equal(img.get_tile(0, 0, c, 0, 0, 0, 150, 70), want[:, :, c]), (k, c)
        assert np.abs(want.astype(int) - np.moveaxis(a[0, :, 0], 0, -1)).mean() < 12       # a picture of the input
    path = tmp_path / "grey.tif"
    omr.write_tiled_tiff(path, a[:, :1], compression=7, tile=(80, 16), jpeg=dict(tables="shared"))
    with omr.TiffImage(path, accept=("jpeg",)) as img:
        assert np.array_equal(img.get_tile(0, 0, 0, 0, 0, 0, 150, 70), np.asarray(Image.open(path)))
