"""Tiled TIFF pixel data, host side (K13): the writer (omr.write_tiled_tiff) against libtiff, the
parser's view of the file (TiffImage.info, level_sizes), the host read route (TiffImage.get_tile,
a plain serial LZW decoder) against numpy slices and against files Pillow wrote, and the files
the reader must refuse: unsupported features (INVALID_ARGUMENT) and corrupt input (INTERNAL).
No GPU; every file is made in tmp_path."""
import struct

import numpy as np
import pytest

import omr
from omr import _lib
from omr.tiffimage import DIMENSION_ORDERS, lzw_encode

TYPES = {"int8": _lib.PIXELS_INT8, "uint8": _lib.PIXELS_UINT8, "int16": _lib.PIXELS_INT16,
         "uint16": _lib.PIXELS_UINT16, "int32": _lib.PIXELS_INT32, "uint32": _lib.PIXELS_UINT32,
         "float32": _lib.PIXELS_FLOAT, "float64": _lib.PIXELS_DOUBLE}


def pixels(name, shape, seed=0):
    rng = np.random.default_rng(seed)
    if name.startswith("float"):
        return np.round(rng.standard_normal(shape) * 300).astype(name)
    info = np.iinfo(name)
    return rng.integers(max(info.min, -30000), min(info.max, 60000), shape).astype(name)


def open_status(path, *dims):
    with pytest.raises(omr.OmrError) as e:
        omr.TiffImage(path, *dims)
    return e.value.status


# ---- the writer against libtiff -------------------------------------------------------------------

def _pil():
    Image = pytest.importorskip("PIL.Image")
    features = pytest.importorskip("PIL.features")
    if not features.check("libtiff"):
        pytest.skip("Pillow without libtiff")
    return Image


@pytest.mark.parametrize("name", ["uint8", "uint16"])
@pytest.mark.parametrize("bo", ["<", ">"])
@pytest.mark.parametrize("pred", [1, 2])
def test_writer_read_by_libtiff(tmp_path, name, bo, pred):
    Image = _pil()
    a = pixels(name, (1, 2, 1, 70, 100), seed=pred)
    a[..., 50:] //= 64                                       # some runs for the coder
    omr.write_tiled_tiff(tmp_path / "w.tif", a, tile=(32, 16), byteorder=bo, compression=5, predictor=pred)
    with Image.open(tmp_path / "w.tif") as im:
        assert im.n_frames == 2
        for k in range(2):
            im.seek(k)
            assert np.array_equal(np.array(im), a[0, k, 0]), k


def test_writer_noise_tile_read_by_libtiff(tmp_path):
    Image = _pil()
    a = np.random.default_rng(2).integers(0, 256, (1, 1, 1, 256, 256), dtype=np.uint8)
    omr.write_tiled_tiff(tmp_path / "n.tif", a, tile=(256, 256), compression=5)
    stream = lzw_encode(a.tobytes())
    # noise finds almost no repeats: ~one code per byte, so several table-full Clears (one per 3836
    # codes), and a mean width above 10 bits means 11- and 12-bit codes were written
    assert len(stream) > 65536 * 10 // 8
    with Image.open(tmp_path / "n.tif") as im:
        assert np.array_equal(np.array(im), a[0, 0, 0])
    with omr.TiffImage(tmp_path / "n.tif") as img:
        assert np.array_equal(img.get_tile(0, 0, 0, 0, 0, 0, 256, 256), a[0, 0, 0])


# ---- info and level sizes ---------------------------------------------------------------------------

@pytest.mark.parametrize("bigtiff", [False, True])
@pytest.mark.parametrize("bo", ["<", ">"])
@pytest.mark.parametrize("layout", ["tiles", "strips"])
def test_info_and_level_sizes(tmp_path, bigtiff, bo, layout):
    a = pixels("uint16", (2, 3, 2, 70, 100))
    l1, l2 = pixels("uint16", (2, 3, 2, 33, 49), 1), pixels("uint16", (2, 3, 2, 17, 20), 2)   # not size >> k
    kw = {"tile": (32, 16)} if layout == "tiles" else {"rows_per_strip": 9}
    omr.write_tiled_tiff(tmp_path / "i.tif", a, levels=[l1, l2], byteorder=bo, bigtiff=bigtiff, compression=5,
                         predictor=2, **kw)
    with omr.TiffImage(tmp_path / "i.tif", 2, 3, 2) as img:
        assert img.info == {"size_x": 100, "size_y": 70, "size_z": 2, "size_c": 3, "size_t": 2,
                            "pixel_type": _lib.PIXELS_UINT16, "big_endian": int(bo == ">"), "n_levels": 3,
                            "compression": 5, "predictor": 2, "tiled": int(layout == "tiles"),
                            "segment_width": 32 if layout == "tiles" else 100,
                            "segment_height": 16 if layout == "tiles" else 9, "big_tiff": int(bigtiff)}
        assert img.level_sizes == [[100, 70], [49, 33], [20, 17]]
        assert img.getResolutionLevels() == 3
        assert np.array_equal(img.get_tile(0, 1, 2, 1, 0, 0, 100, 70), a[1, 2, 1])
        assert np.array_equal(img.get_tile(1, 0, 1, 1, 0, 0, 49, 33), l1[1, 1, 0])
        assert np.array_equal(img.get_tile(2, 1, 0, 0, 0, 0, 20, 17), l2[0, 0, 1])


# predictor 2 is for 8-, 16- and 32-bit samples (64-bit: rejected, test_rejections)
@pytest.mark.parametrize("name,comp,pred", [(n, c, p) for n in TYPES for (c, p) in [(1, 1), (5, 1), (5, 2)]
                                            if not (n == "float64" and p == 2)])
def test_all_pixel_types(tmp_path, name, comp, pred):
    a = pixels(name, (1, 1, 2, 37, 50), seed=comp + pred)
    for bo in "<>":
        omr.write_tiled_tiff(tmp_path / "t.tif", a, tile=(16, 16), byteorder=bo, compression=comp, predictor=pred)
        with omr.TiffImage(tmp_path / "t.tif", 2, 1, 1) as img:
            assert img.pixel_type == TYPES[name] and img.info["compression"] == comp and img.info["predictor"] == pred
            for z in range(2):
                got = img.get_tile(0, z, 0, 0, 0, 0, 50, 37)
                assert got.dtype == img.dtype and got.tobytes() == a[0, 0, z].astype(img.dtype).tobytes()


# ---- host reads -------------------------------------------------------------------------------------

REGIONS = [(3, 2, 10, 9), (25, 10, 30, 20), (90, 60, 10, 10), (64, 48, 36, 22), (99, 69, 1, 1), (0, 0, 1, 1),
           (0, 0, 100, 70), (17, 0, 5, 70), (0, 33, 100, 3), (5, 5, 0, 0)]


@pytest.mark.parametrize("order", DIMENSION_ORDERS)
def test_get_tile_every_level_and_order(tmp_path, order):
    a = pixels("uint16", (2, 2, 3, 70, 100), 3)
    lv = [pixels("uint16", (2, 2, 3, 35, 50), 4), pixels("uint16", (2, 2, 3, 18, 23), 5)]
    omr.write_tiled_tiff(tmp_path / "o.tif", a, levels=lv, tile=(32, 16), byteorder=">", compression=5, predictor=2,
                         dimension_order=order)
    with omr.TiffImage(tmp_path / "o.tif", 3, 2, 2, order) as img:
        for (z, c, t) in [(0, 0, 0), (2, 1, 1), (1, 0, 1), (0, 1, 0)]:
            for level, arr in enumerate([a] + lv):
                H, W = arr.shape[3:]
                for (x, y, w, h) in REGIONS:
                    x, y = x * W // 100, y * H // 70
                    w, h = min(w, W - x), min(h, H - y)
                    got = img.get_tile(level, z, c, t, x, y, w, h)
                    assert np.array_equal(got, arr[t, c, z, y:y + h, x:x + w]), (level, z, c, t, x, y, w, h)
        for bad in [(0, 0, 0, 0, 95, 0, 10, 10), (0, 3, 0, 0, 0, 0, 1, 1), (3, 0, 0, 0, 0, 0, 1, 1),
                    (0, 0, 0, 0, -1, 0, 1, 1), (1, 0, 0, 0, 0, 0, 51, 1)]:
            with pytest.raises(omr.OmrError) as e:
                img.get_tile(*bad)
            assert e.value.status == _lib.INVALID_ARGUMENT, bad


def test_strips_and_streams_without_eoi_or_with_early_clears(tmp_path):
    a = pixels("int16", (1, 1, 1, 70, 100), 6)
    for kw in ({"eoi": False}, {"early_clear": 100}, {}):
        omr.write_tiled_tiff(tmp_path / "s.tif", a, rows_per_strip=16, compression=5, predictor=2, **kw)
        with omr.TiffImage(tmp_path / "s.tif") as img:
            for (x, y, w, h) in REGIONS:
                assert np.array_equal(img.get_tile(0, 0, 0, 0, x, y, w, h), a[0, 0, 0, y:y + h, x:x + w])


def test_zero_byte_count_segment_reads_as_zeros(tmp_path):
    a = pixels("uint16", (1, 1, 1, 70, 100), 7)
    a[0, 0, 0, 16:32, 32:64] = 0
    for comp in (1, 5):
        res = omr.write_tiled_tiff(tmp_path / "z.tif", a, tile=(32, 16), compression=comp, skip_zero_segments=True)
        raw = (tmp_path / "z.tif").read_bytes()
        counts = _tag(raw, res["ifds"][0], 325)
        assert counts.count(0) == 1
        with omr.TiffImage(tmp_path / "z.tif") as img:
            assert np.array_equal(img.get_tile(0, 0, 0, 0, 0, 0, 100, 70), a[0, 0, 0])
            assert not img.get_tile(0, 0, 0, 0, 32, 16, 32, 16).any()


# ---- an independent encoder -----------------------------------------------------------------------

@pytest.mark.parametrize("name", ["uint8", "uint16"])
@pytest.mark.parametrize("pred", [1, 2])
def test_files_written_by_libtiff(tmp_path, name, pred):
    Image = _pil()
    from PIL import TiffImagePlugin
    a = pixels(name, (300, 211), 8)
    a[:, 100:] //= 128
    ifd = TiffImagePlugin.ImageFileDirectory_v2()
    if pred == 2:
        ifd[317] = 2
    Image.fromarray(a).save(tmp_path / "p.tif", compression="tiff_lzw", tiffinfo=ifd)
    with omr.TiffImage(tmp_path / "p.tif") as img:
        assert img.info["compression"] == 5 and img.info["predictor"] == pred and not img.info["tiled"]
        assert np.array_equal(img.get_tile(0, 0, 0, 0, 0, 0, 211, 300), a)
        assert np.array_equal(img.get_tile(0, 0, 0, 0, 7, 150, 100, 149), a[150:299, 7:107])


# ---- rejections and corrupt input -------------------------------------------------------------------

def _tag(raw, ifd, tag, bo="<"):
    """Values of a classic-TIFF IFD entry."""
    n = struct.unpack_from(bo + "H", raw, ifd)[0]
    for k in range(n):
        t, typ, cnt, val = struct.unpack_from(bo + "HHII", raw, ifd + 2 + 12 * k)
        if t == tag:
            fmt = {3: "H", 4: "I"}[typ]
            size = struct.calcsize(fmt) * cnt
            at = ifd + 2 + 12 * k + 8 if size <= 4 else val
            return list(struct.unpack_from(bo + fmt * cnt, raw, at))
    raise KeyError(tag)


def _entry_at(raw, ifd, tag, bo="<"):
    n = struct.unpack_from(bo + "H", raw, ifd)[0]
    for k in range(n):
        if struct.unpack_from(bo + "H", raw, ifd + 2 + 12 * k)[0] == tag:
            return ifd + 2 + 12 * k
    raise KeyError(tag)


def test_missing_file(tmp_path):
    assert open_status(tmp_path / "none.tif") == _lib.NOT_FOUND


def test_rejections(tmp_path):
    a = pixels("uint16", (1, 2, 1, 40, 50))
    p = tmp_path / "r.tif"
    for override in ({259: 8}, {259: 7}, {259: 50000}, {317: 3}, {277: 3}, {266: 2}, {258: 12}, {339: 4}):
        omr.write_tiled_tiff(p, a, tile=(16, 16), compression=5, tag_overrides=override)
        assert open_status(p, 1, 2, 1) == _lib.INVALID_ARGUMENT, override
    omr.write_tiled_tiff(p, pixels("float64", (1, 1, 1, 40, 50)), tile=(16, 16), compression=5, tag_overrides={317: 2})
    assert open_status(p) == _lib.INVALID_ARGUMENT                      # predictor 2 with 64-bit samples
    omr.write_tiled_tiff(p, a, tile=(16, 16), compression=5)
    assert open_status(p, 1, 3, 1) == _lib.INVALID_ARGUMENT             # fewer IFDs than Z*C*T
    assert open_status(p, 1, 2, 1, "XYCZ") == _lib.INVALID_ARGUMENT
    assert open_status(p, 1, 2, 1, "XYZZT") == _lib.INVALID_ARGUMENT
    omr.TiffImage(p, 1, 2, 1).close()
    # planes that disagree: on size, on type, on level count
    res = omr.write_tiled_tiff(p, a, tile=(16, 16), compression=5)
    raw = bytearray(p.read_bytes())
    struct.pack_into("<I", raw, _entry_at(raw, res["ifds"][1], 256) + 8, 49)
    p.write_bytes(raw)
    assert open_status(p, 1, 2, 1) == _lib.INVALID_ARGUMENT
    raw = bytearray(p.read_bytes())
    struct.pack_into("<I", raw, _entry_at(raw, res["ifds"][1], 256) + 8, 50)
    struct.pack_into("<H", raw, _entry_at(raw, res["ifds"][1], 339) + 8, 2)
    p.write_bytes(raw)
    assert open_status(p, 1, 2, 1) == _lib.INVALID_ARGUMENT
    res = omr.write_tiled_tiff(p, a, levels=[a[..., ::2, ::2]], tile=(16, 16), compression=5)
    raw = bytearray(p.read_bytes())
    struct.pack_into("<H", raw, _entry_at(raw, res["ifds"][1], 330), 65000)   # plane 1 loses its SubIFDs tag
    p.write_bytes(raw)
    assert open_status(p, 1, 2, 1) == _lib.INVALID_ARGUMENT
    p.write_bytes(b"not a tiff file at all")
    assert open_status(p) == _lib.INVALID_ARGUMENT


def corrupt_files(tmp_path):
    """(name, path, dims) of files that are corrupt at open."""
    a = pixels("uint16", (1, 2, 1, 40, 50))
    base = tmp_path / "base.tif"
    res = omr.write_tiled_tiff(base, a, tile=(16, 16), compression=5)
    raw = base.read_bytes()
    ifd0, ifd1 = res["ifds"]
    out = []

    def add(name, data):
        p = tmp_path / (name + ".tif")
        p.write_bytes(bytes(data))
        out.append((name, p))

    add("truncated_half", raw[:len(raw) // 2])
    add("truncated_in_ifd", raw[:ifd1 + 20])
    add("truncated_header", raw[:6])
    b = bytearray(raw)
    offs_at = struct.unpack_from("<I", b, _entry_at(b, ifd0, 324) + 8)[0]
    struct.pack_into("<I", b, offs_at + 8, len(raw) - 3)                   # a segment runs past the end
    add("offset_past_end", b)
    b = bytearray(raw)
    struct.pack_into("<I", b, _entry_at(b, ifd0, 324) + 8, len(raw) + 1000)   # the offsets array itself
    add("array_past_end", b)
    b = bytearray(raw)
    n1 = struct.unpack_from("<H", b, ifd1)[0]
    struct.pack_into("<I", b, ifd1 + 2 + 12 * n1, ifd0)                    # IFD 1 -> IFD 0
    add("looping_chain", b)
    b = bytearray(raw)
    struct.pack_into("<I", b, _entry_at(b, ifd0, 324) + 4, 0xFFFFFFFF)     # count * 4 overflows 32 bits
    add("overflowing_count", b)
    b = bytearray(raw)
    struct.pack_into("<I", b, _entry_at(b, ifd0, 256) + 8, 0x7FFFFFFF)     # across * down no longer matches
    struct.pack_into("<I", b, _entry_at(b, ifd0, 257) + 8, 0x7FFFFFFF)
    add("huge_image", b)
    b = bytearray(raw)
    struct.pack_into("<H", b, _entry_at(b, ifd0, 322) + 8, 0)              # tile width 0
    add("zero_tile", b)
    return out


def test_corrupt_files_at_open(tmp_path):
    for name, p in corrupt_files(tmp_path):
        assert open_status(p, 1, 2, 1) == _lib.INTERNAL, name


def corrupt_streams():
    data = np.random.default_rng(9).integers(0, 9, 5000, dtype=np.uint8).tobytes()
    good = lzw_encode(data)
    bits = "100000000" + "000000101" + "100101100" + "100000001"          # Clear, 5, 300 (next free: 258), EOI
    return data, good, {
        "bad_code": int(bits.ljust(40, "0"), 2).to_bytes(5, "big"),
        "code_after_clear": int(("100000000" + "100000010").ljust(24, "0"), 2).to_bytes(3, "big"),
        "ends_early": good[:len(good) // 2],
        "eoi_early": lzw_encode(data[:100]),
        "lsb_first": b"\x00\x01" + good[2:],
        "empty": b"",
    }


def test_corrupt_streams_host_decoder():
    data, good, bad = corrupt_streams()
    assert omr.lzw_decode_host(good, len(data)) == data
    assert omr.lzw_decode_host(good, 4000) == data[:4000]                 # ends once the size is produced
    assert omr.lzw_decode_host(lzw_encode(data, eoi=False), len(data)) == data
    for name, s in bad.items():
        with pytest.raises(omr.OmrError) as e:
            omr.lzw_decode_host(s, len(data))
        assert e.value.status == _lib.INTERNAL, name


def test_corrupt_stream_in_a_file(tmp_path):
    a = pixels("uint8", (1, 1, 1, 40, 50))
    p = tmp_path / "c.tif"
    res = omr.write_tiled_tiff(p, a, tile=(16, 16), compression=5)
    raw = bytearray(p.read_bytes())
    seg = lzw_encode(a[0, 0, 0, :16, 16:32].tobytes())     # tile 1
    at = raw.index(seg)
    counts_at = struct.unpack_from("<I", raw, _entry_at(raw, res["ifds"][0], 325) + 8)[0]
    assert struct.unpack_from("<I", raw, counts_at + 4)[0] == len(seg)
    for name in ("bad_code", "ends_early"):
        b = bytearray(raw)
        if name == "bad_code":
            b[at + 1] = b[at + 2] = 0xFF                    # behind the Clear, a code far above 258
        else:
            struct.pack_into("<I", b, counts_at + 4, len(seg) // 2)
        p.write_bytes(b)
        with omr.TiffImage(p) as img:                                      # open succeeds: the table is sound
            with pytest.raises(omr.OmrError) as e:
                img.get_tile(0, 0, 0, 0, 0, 0, 50, 40)
            assert e.value.status == _lib.INTERNAL, name
            assert np.array_equal(img.get_tile(0, 0, 0, 0, 0, 0, 16, 16), a[0, 0, 0, :16, :16])   # other tiles read
