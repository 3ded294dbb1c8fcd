"""Blosc OME-Zarr chunks on the host (K15): omr_lz4_decode_host against streams of a real encoder
(tests/golden/lz4_blocks.npz), crafted and malformed ones, omr_blosc_decode_host against the
product's encoder over the container's variants, then omr_zarr_image_open_ex and the host route
(ZarrImage.get_tile) on Blosc groups against numpy, the open rules and the corrupt chunks with their
status codes.  Every comparison is byte equality.  No GPU."""
import ctypes
import json
import zlib

import numpy as np
import pytest

import omr
from omr import _lib
from blosc_streams import (bad_streams, chunk_pixels, crafted_streams, edge_streams, golden_streams, layout_image,
                           lz4_census, lz4_decode_py, mixed_streams)

TYPES = {"int8": _lib.PIXELS_INT8, "uint8": _lib.PIXELS_UINT8, "int16": _lib.PIXELS_INT16,
         "uint16": _lib.PIXELS_UINT16, "int32": _lib.PIXELS_INT32, "uint32": _lib.PIXELS_UINT32,
         "float32": _lib.PIXELS_FLOAT, "float64": _lib.PIXELS_DOUBLE}
W, H = 200, 150
BOTH = ("zlib", "blosc")


def internal(fn, *args):
    with pytest.raises(omr.OmrError) as e:
        fn(*args)
    return e.value.status == _lib.INTERNAL


# ---- the LZ4 block decoder ------------------------------------------------------------------------

GOOD = golden_streams() + crafted_streams()


def test_golden_file_holds_the_cases():
    names = [g[0] for g in golden_streams()]
    assert names == ["one_byte", "abc", "noise_3000", "equal_70000", "few_8000", "few_8000_hc", "ramp_8000",
                     "ramp_8000_hc", "chunk_high_bytes", "chunk_low_bytes"]
    sizes = {n: (len(d), len(s)) for n, d, s in golden_streams()}
    assert sizes["equal_70000"] == (70000, 285)            # offset 1 and a long length extension
    assert sizes["few_8000_hc"][1] < sizes["few_8000"][1] and sizes["chunk_low_bytes"][1] > 3072


@pytest.mark.parametrize("k", range(len(GOOD)), ids=[g[0] for g in GOOD])
def test_lz4_decode_host(k):
    name, data, stream = GOOD[k]
    assert lz4_decode_py(stream, len(data)) == data        # the rule of the issue, restated
    assert omr.lz4_decode_host(stream, len(data)) == data
    assert internal(omr.lz4_decode_host, stream, len(data) + 1)
    if data:
        assert internal(omr.lz4_decode_host, stream, len(data) - 1)


def test_lz4_decode_host_against_liblz4_when_present():
    try:
        lz = ctypes.CDLL("liblz4.so.1")
    except OSError:
        return                                             # the golden file stands in for it
    for name, data, stream in golden_streams():            # (liblz4 holds crafted ends to its encoder's margins)
        back = ctypes.create_string_buffer(len(data) + 1)
        assert lz.LZ4_decompress_safe(stream, back, len(stream), len(data)) == len(data), name
        assert back.raw[:len(data)] == data, name
    rng = np.random.default_rng(160)
    for n in (1, 12, 13, 64, 777, 20000):
        for d in (rng.integers(0, 256, n, dtype=np.uint8).tobytes(), rng.integers(0, 3, n, dtype=np.uint8).tobytes()):
            s = omr.lz4_encode(d)                          # the product's encoder writes what liblz4 reads
            back = ctypes.create_string_buffer(n + 1)
            assert lz.LZ4_decompress_safe(s, back, len(s), n) == n and back.raw[:n] == d
            cap = lz.LZ4_compressBound(n)
            buf = ctypes.create_string_buffer(cap)
            m = lz.LZ4_compress_default(d, buf, n, cap)
            assert omr.lz4_decode_host(buf.raw[:m], n) == d


def test_census_of_the_edge_streams():
    """Conditions on the inputs, judged by lz4_census alone: the edge streams hold every case they
    were written for.  A match is long when its body is more than 64 dwords, so that a lane steps
    its phase more than once; a copy's alignments are counted from the stream's and the slot's
    first bytes, and the device tests place both at every alignment."""
    parts = {name: lz4_census(stream) for name, data, stream in edge_streams()}
    matches = [m for c in parts.values() for m in c["matches"]]
    periods = (8, 9, 31, 63, 64, 65, 100, 127, 128, 129, 255, 256, 257, 300)
    for free in (True, False):
        long = {(dist, mpos % 4) for mlen, dist, mpos, f, _, _ in matches if mlen >= 1100 and f == free}
        assert long >= {(d, a) for d in periods for a in range(4)}, free
    assert {(dist, mpos % 4) for mlen, dist, mpos, _, _, _ in matches if mlen == 2 * dist + 1} >= {(d, a) for d in periods for a in range(4)}
    for mlen in (4, 5, 32, 33, 64, 65, 257):               # the switch between the plain copy and the period
        for free in (True, False):
            assert {m[1] - mlen for m in matches if m[0] == mlen and m[3] == free} >= {-1, 0, 1}, (mlen, free)
    # the sizes at which a lane hands over to the wave, and wave_copy's grid
    literals = set().union(*(c["literals"] for c in parts.values()))
    assert {n for n, _, _ in literals} >= {0, 1, 15, 16, 17, 270}
    assert literals >= {(n, da, sa) for n in range(17, 30) for da in range(4) for sa in range(4)}
    plain = {(mlen, mpos % 4, (mpos - dist) % 4) for mlen, dist, mpos, _, _, _ in matches if dist >= mlen}
    assert plain >= {(n, da, sa) for n in range(33, 46) for da in range(4) for sa in range(4)}
    for mlen in (32, 33):
        assert {m[3] for m in matches if m[0] == mlen} == {True, False}, mlen
    # the round's border
    assert {c["sequences"] for c in parts.values()} >= {63, 64, 65, 128, 129}
    closing = {(k, min(lits, 1)) for k, lits in (c["closing"] for c in parts.values())}
    assert closing >= {(62, 0), (62, 1), (63, 0), (63, 1), (0, 0), (0, 1)}
    # the rule of the free match, from both sides of both edges, for lane-sized and wave-sized matches
    edges = parts["free and dependent matches at the rule's edges"]["matches"]
    for size in (8, 40):
        mine = [m for m in edges if m[0] == size]
        assert any(f and over == 0 and below < 0 for _, _, _, f, below, over in mine)          # ends at `first`
        assert any(not f and over == 1 and below < 0 for _, _, _, f, below, over in mine)      # a byte above
        assert any(f and below == 0 and over > 0 for _, _, _, f, below, over in mine)          # starts at `pos`
        assert any(not f and below == -1 and over > 0 for _, _, _, f, below, over in mine)     # a byte below
        # and what a dependent match reads: an earlier sequence's literals alone, literals and a match that a
        # lane copied, a dependent match before it from below and from above
        reads = [s for m, s in zip(edges, parts["free and dependent matches at the rule's edges"]["sources"])
                 if m[0] == size and not m[3]]
        assert {"literals"} in reads
        assert any(s >= {"literals", "free lane match"} and "dependent match" not in s for s in reads)
        assert any(s >= {"literals", "dependent match, its first byte"} for s in reads)
        assert any("dependent match, its last byte" in s and "dependent match, its first byte" not in s for s in reads)
    # the window over the stream: every kind of byte is the first of a reload at every alignment
    for mis in range(4):
        kinds = set().union(*(c["reloads"][mis] for name, c in parts.items() if name.startswith("window reloads")))
        assert kinds == {"token", "lit ext", "offset 0", "offset 1", "match ext"}, (mis, kinds)
    sweep = [lz4_census(s) for name, _, s in crafted_streams() if name.startswith("sweep ")]
    assert len(sweep) == 16 and all(100 <= c["sequences"] <= 400 for c in sweep)


def test_lz4_mixed_streams_host():
    for data, stream in mixed_streams():
        assert omr.lz4_decode_host(stream, len(data)) == data


@pytest.mark.parametrize("name,stream,expected", bad_streams(), ids=[b[0] for b in bad_streams()])
def test_lz4_bad_stream_host(name, stream, expected):
    assert internal(omr.lz4_decode_host, stream, expected)


# ---- the container ----------------------------------------------------------------------------------

def test_blosc_round_trips():
    rng = np.random.default_rng(161)
    for n in (1, 7, 511, 512, 6144, 20001):
        for d in (rng.integers(0, 256, n, dtype=np.uint8).tobytes(), (np.arange(n) // 9).astype(np.uint8).tobytes()):
            for ts in (1, 2, 3, 4, 8, 16, 17):
                for shuffle in (0, 1):
                    for blocksize in (0, 2048, 4096, 100):
                        if blocksize > n or (blocksize % ts and blocksize // ts >= 128):
                            continue
                        for split in (None, False):
                            for memcpy in (False, True):
                                c = omr.blosc_encode(d, ts, shuffle, blocksize, split, memcpy)
                                assert omr.blosc_decode_host(c, n) == d, (n, ts, shuffle, blocksize, split, memcpy)
                                assert int.from_bytes(c[12:16], "little") == len(c)
    d = bytes(range(256)) * 24                             # 6144 bytes of uint16: the flags and the table
    c = omr.blosc_encode(d, 2, 1, 2048)
    assert c[:4] == bytes([2, 1, 0x21, 2]) and [int.from_bytes(c[k:k + 4], "little") for k in (4, 8)] == [6144, 2048]
    assert int.from_bytes(c[16:20], "little") == 16 + 12   # three blocks
    assert omr.blosc_encode(d, 2, 0, 2048, split=False)[2] == 0x30
    assert omr.blosc_encode(d, 2, 1, 0, memcpy=True)[16:] == d


def write_group(path, a, sep="/", byteorder="<", **blosc):
    omr.write_zarr(path, a, chunk=(64, 48), byteorder=byteorder, compressor="blosc", dimension_separator=sep,
                   blosc=blosc)


@pytest.mark.parametrize("name", list(TYPES))
@pytest.mark.parametrize("bo", ["<", ">"])
@pytest.mark.parametrize("split", [None, False], ids=["split", "nosplit"])
@pytest.mark.parametrize("shuffle", [0, 1])
@pytest.mark.parametrize("sep", ["/", "."])
def test_open_and_get_tile(tmp_path, name, bo, split, shuffle, sep):
    rng = np.random.default_rng(zlib.crc32(repr((name, bo, split, shuffle, sep)).encode()))
    a = chunk_pixels(name, rng, (1, 2, 1, H, W))
    path = tmp_path / "img.zarr" / "0"
    write_group(path, a, sep, bo, split=split, shuffle=shuffle)
    flags = (path / "0" / sep.join("00000")).read_bytes()[2]
    assert flags == 0x20 | shuffle | (0x10 if split is False else 0)
    with omr.ZarrImage(path, codecs=BOTH) as img:
        assert img.info == {"size_x": W, "size_y": H, "size_z": 1, "size_c": 2, "size_t": 1, "pixel_type": TYPES[name],
                            "big_endian": int(bo == ">" and a.itemsize > 1), "n_levels": 1, "compression": 2,
                            "chunk_width": 64, "chunk_height": 48, "dimension_separator": ord(sep)}
        for (c, x, y, w, h) in [(0, 0, 0, W, H), (1, 45, 33, 37, 29), (1, 199, 149, 1, 1), (0, 128, 96, 64, 48),
                                (0, 10, 10, 0, 0)]:
            got = img.get_tile(0, 0, c, 0, x, y, w, h)
            assert got.tobytes() == a[0, c, 0, y:y + h, x:x + w].astype(img.dtype).tobytes(), (c, x, y, w, h)


def test_block_layouts(tmp_path):
    path = tmp_path / "l.zarr"
    a, files = layout_image(path)
    with omr.ZarrImage(path, codecs=BOTH) as img:
        for c in range(6):
            assert img.get_tile(0, 0, c, 0, 0, 0, 64, 48).tobytes() == a[0, c, 0].astype("<u2").tobytes(), c
            assert img.get_tile(0, 0, c, 0, 13, 7, 30, 29).tobytes() == a[0, c, 0, 7:36, 13:43].astype("<u2").tobytes(), c
        assert not img.get_tile(0, 0, 5, 0, 0, 0, 64, 48).any()


def test_float64_block_of_64_elements_is_not_split(tmp_path):
    a = chunk_pixels("float64", np.random.default_rng(163), (1, 1, 1, 48, 64))
    path = tmp_path / "f.zarr"
    write_group(path, a, ".", blocksize=512)
    c = (path / "0" / "0.0.0.0.0").read_bytes()
    assert c[2] == 0x21 and c[3] == 8                      # 0x10 clear, yet 512 / 8 = 64 elements: one stream per block
    nblocks = 48 * 64 * 8 // 512
    first = int.from_bytes(c[16:20], "little")
    assert first == 16 + 4 * nblocks
    csize = int.from_bytes(c[first:first + 4], "little")
    assert int.from_bytes(c[20:24], "little") == first + 4 + csize
    with omr.ZarrImage(path, codecs=BOTH) as img:
        assert img.get_tile(0, 0, 0, 0, 0, 0, 64, 48).tobytes() == a[0, 0, 0].tobytes()


def test_level_1(tmp_path):
    rng = np.random.default_rng(164)
    a, lv1 = chunk_pixels("uint16", rng, (1, 2, 1, H, W)), chunk_pixels("uint16", rng, (1, 2, 1, 75, 100))
    omr.write_zarr(tmp_path / "p.zarr", a, levels=[lv1], chunk=(64, 48), byteorder=">", compressor="blosc")
    with omr.ZarrImage(tmp_path / "p.zarr", codecs=BOTH) as img:
        assert img.level_sizes == [[W, H], [100, 75]]
        assert img.get_tile(1, 0, 1, 0, 30, 20, 70, 55).tobytes() == lv1[0, 1, 0, 20:75, 30:100].astype(">u2").tobytes()


# ---- open rules ---------------------------------------------------------------------------------

def open_status(path, **kw):
    try:
        omr.ZarrImage(path, **kw).close()
    except omr.OmrError as e:
        return e.status
    return _lib.OK


def test_open_rules(tmp_path):
    a = chunk_pixels("uint16", np.random.default_rng(165), (1, 1, 1, 48, 64))
    omr.write_zarr(tmp_path / "b", a, chunk=(64, 48), compressor="blosc")
    omr.write_zarr(tmp_path / "z", a, chunk=(64, 48))
    omr.write_zarr(tmp_path / "n", a, chunk=(64, 48), compressor=None)
    assert open_status(tmp_path / "b") == _lib.INVALID_ARGUMENT           # omr_zarr_image_open keeps refusing Blosc
    assert open_status(tmp_path / "b", codecs=("zlib",)) == _lib.INVALID_ARGUMENT
    assert open_status(tmp_path / "b", codecs=BOTH) == _lib.OK
    assert open_status(tmp_path / "b", codecs=("blosc",)) == _lib.OK
    assert open_status(tmp_path / "z", codecs=BOTH) == _lib.OK
    assert open_status(tmp_path / "n", codecs=BOTH) == _lib.OK
    assert open_status(tmp_path / "z", codecs=("blosc",)) == _lib.INVALID_ARGUMENT   # named in .zarray, not in codecs
    assert open_status(tmp_path / "n", codecs=()) == _lib.OK and open_status(tmp_path / "z", codecs=()) == _lib.INVALID_ARGUMENT
    assert open_status(tmp_path / "b", codecs=("zstd",)) == _lib.INVALID_ARGUMENT
    for path in ("z", "n"):
        with omr.ZarrImage(tmp_path / path, codecs=BOTH) as img:
            assert img.info["compression"] == int(path == "z")
            assert img.get_tile(0, 0, 0, 0, 0, 0, 64, 48).tobytes() == a[0, 0, 0].tobytes()


def test_open_ex_arguments(tmp_path):
    a = chunk_pixels("uint16", np.random.default_rng(166), (1, 1, 1, 48, 64))
    omr.write_zarr(tmp_path / "b", a, chunk=(64, 48), compressor="blosc")
    omr.write_zarr(tmp_path / "z", a, chunk=(64, 48))

    def open_ex(path, opt):
        h = ctypes.c_void_p()
        st = _lib.lib.omr_zarr_image_open_ex(str(path).encode(), opt, ctypes.byref(h))
        if st == _lib.OK:
            _lib.lib.omr_zarr_image_close(h)
        else:
            assert not h.value
        return st

    size = ctypes.sizeof(_lib.ZarrOpenOptions)
    assert size == 8
    assert open_ex(tmp_path / "z", None) == _lib.OK                        # NULL: as omr_zarr_image_open
    assert open_ex(tmp_path / "b", None) == _lib.INVALID_ARGUMENT
    assert open_ex(tmp_path / "b", ctypes.byref(_lib.ZarrOpenOptions(size, 3))) == _lib.OK
    assert open_ex(tmp_path / "b", ctypes.byref(_lib.ZarrOpenOptions(size, 3 | 4))) == _lib.INVALID_ARGUMENT
    assert open_ex(tmp_path / "z", ctypes.byref(_lib.ZarrOpenOptions(size, 0x80000001))) == _lib.INVALID_ARGUMENT
    assert open_ex(tmp_path / "b", ctypes.byref(_lib.ZarrOpenOptions(size - 1, 3))) == _lib.INVALID_ARGUMENT
    assert open_ex(tmp_path / "b", ctypes.byref(_lib.ZarrOpenOptions(0, 3))) == _lib.INVALID_ARGUMENT
    big = (ctypes.c_uint32 * 4)(16, 3, 0, 0)                               # a larger struct of a later version
    assert open_ex(tmp_path / "b", ctypes.cast(big, ctypes.POINTER(_lib.ZarrOpenOptions))) == _lib.OK
    assert _lib.lib.omr_zarr_image_open_ex(str(tmp_path / "b").encode(), None, None) == _lib.INVALID_ARGUMENT


REFUSED = [("blosclz", "uint16", {"cname": "blosclz"}), ("zstd", "uint16", {"cname": "zstd"}),
           ("zlib inside", "uint16", {"cname": "zlib"}), ("snappy", "uint16", {"cname": "snappy"}),
           ("no cname", "uint16", {"cname": None}), ("bit shuffle", "uint16", {"shuffle": 2}),
           ("automatic shuffle on a one-byte type", "uint8", {"shuffle": -1}),
           ("shuffle 1.5", "uint16", {"shuffle": 1.5})]


@pytest.mark.parametrize("what,name,change", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_compressors(tmp_path, what, name, change):
    a = chunk_pixels(name, np.random.default_rng(167), (1, 1, 1, 48, 64))
    comp = {"id": "blosc", "cname": "lz4", "clevel": 5, "shuffle": 1, "blocksize": 0}
    comp.update(change)
    comp = {k: v for k, v in comp.items() if v is not None}
    omr.write_zarr(tmp_path / "g", a, chunk=(64, 48), compressor="blosc", zarray_overrides={"compressor": comp})
    assert open_status(tmp_path / "g", codecs=BOTH) == _lib.INVALID_ARGUMENT


def test_accepted_compressors(tmp_path):
    a = chunk_pixels("uint16", np.random.default_rng(168), (1, 1, 1, 48, 64))
    for k, comp in enumerate([{"id": "blosc", "cname": "lz4hc", "clevel": 9, "shuffle": 1, "blocksize": 0},
                              {"id": "blosc", "cname": "lz4", "shuffle": -1},          # wider than a byte: byte shuffle
                              {"id": "blosc", "cname": "lz4", "shuffle": 0, "blocksize": 12345},
                              {"id": "blosc", "cname": "lz4", "clevel": "x"}]):        # clevel is not looked at
        omr.write_zarr(tmp_path / f"g{k}", a, chunk=(64, 48), compressor="blosc", zarray_overrides={"compressor": comp})
        with omr.ZarrImage(tmp_path / f"g{k}", codecs=BOTH) as img:
            assert img.get_tile(0, 0, 0, 0, 0, 0, 64, 48).tobytes() == a[0, 0, 0].tobytes()


def test_levels_that_disagree(tmp_path):
    rng = np.random.default_rng(169)
    a, lv1 = chunk_pixels("uint16", rng, (1, 1, 1, 96, 128)), chunk_pixels("uint16", rng, (1, 1, 1, 48, 64))
    omr.write_zarr(tmp_path / "g", a, levels=[lv1], chunk=(64, 48), compressor="blosc")
    meta = json.loads((tmp_path / "g" / "1" / ".zarray").read_text())
    meta["compressor"] = {"id": "zlib", "level": 1}
    (tmp_path / "g" / "1" / ".zarray").write_text(json.dumps(meta))
    assert open_status(tmp_path / "g", codecs=BOTH) == _lib.INVALID_ARGUMENT


# ---- corrupt chunks -----------------------------------------------------------------------------

def put32(c, at, v):
    return c[:at] + int(v & 0xFFFFFFFF).to_bytes(4, "little") + c[at + 4:]


def corrupt_chunks():
    """[(name, chunk file bytes)] for a 64 x 48 uint16 chunk (6,144 bytes): each must read as
    OMR_INTERNAL."""
    a = chunk_pixels("uint16", np.random.default_rng(170), (1, 1, 1, 48, 64))
    raw = a[0, 0, 0].astype("<u2").tobytes()
    good = omr.blosc_encode(raw, 2, 1, 2048)               # three blocks of two splits
    assert omr.blosc_decode_host(good, 6144) == raw
    table_end = 16 + 12
    assert int.from_bytes(good[16:20], "little") == table_end
    cs0 = int.from_bytes(good[table_end:table_end + 4], "little")
    cs1 = int.from_bytes(good[table_end + 4 + cs0:table_end + 8 + cs0], "little")
    assert cs0 == 1024 and 0 < cs1 < 1024                  # "<u2" shuffled: the low bytes first, stored raw
    out = [("file under 16 bytes", good[:15]),
           ("version 3", b"\x03" + good[1:]),
           ("nbytes one more", put32(good, 4, 6145)), ("nbytes one less", put32(good, 4, 6143)),
           ("blocksize 0", put32(good, 8, 0)), ("blocksize nbytes + 1", put32(good, 8, 6145)),
           ("blocksize negative", put32(good, 8, -2048)),
           ("cbytes not the file size", put32(good, 12, len(good) + 1)), ("a byte appended", good + b"\0"),
           ("typesize 0", good[:3] + b"\0" + good[4:]),
           ("bstart inside the table", put32(good, 20, table_end - 4)),
           ("bstart past the file", put32(good, 24, len(good) + 1)), ("bstart negative", put32(good, 16, -1)),
           ("csize 0", put32(good, table_end, 0)), ("csize negative", put32(good, table_end, -5)),
           ("csize neblock + 1", put32(good, table_end, 1025)),
           ("csize past the file", good[:-1]),
           ("compressor format 0", good[:2] + bytes([good[2] & 0x1F]) + good[3:]),
           ("compressor format 4", good[:2] + bytes([good[2] & 0x1F | 4 << 5]) + good[3:]),
           ("bit-shuffle flag", good[:2] + bytes([good[2] | 4]) + good[3:]),
           ("memcpyed with a wrong cbytes", good[:2] + bytes([good[2] | 2]) + good[3:]),
           ("truncated table", good[:20])]
    out[16] = (out[16][0], put32(out[16][1], 12, len(out[16][1])))        # cbytes right, the last stream cut
    out[-1] = (out[-1][0], put32(out[-1][1], 12, 20))
    mem = omr.blosc_encode(raw, 2, 1, 0, memcpy=True)
    out.append(("memcpyed and cut", put32(mem[:-1], 12, len(mem) - 1)))
    # 6,144 blocks of one byte whose bstarts all point at one stored split: sound word by word, but the
    # streams listed add up to more than the file holds
    alias = bytes([2, 1, 0x30, 2]) + b"".join(int(v).to_bytes(4, "little") for v in (6144, 1, 16 + 4 * 6144 + 5))
    alias += (16 + 4 * 6144).to_bytes(4, "little") * 6144 + (1).to_bytes(4, "little") + b"\x07"
    out.append(("bstarts that all point at one split", alias))
    # each bad LZ4 stream as the one split of a one-block chunk whose size it claims (an empty stream,
    # and one longer than the chunk, are refused by the csize rule before the LZ4 decoder sees them)
    for name, s, e in bad_streams():
        head = bytes([2, 1, 0x30, 2]) + b"".join(int(v).to_bytes(4, "little") for v in (e, e, 16 + 4 + 4 + len(s)))
        out.append(("lz4: " + name, e, head + (20).to_bytes(4, "little") + len(s).to_bytes(4, "little") + s))
    return [(c[0], 6144, c[1]) if len(c) == 2 else c for c in out]


CORRUPT = corrupt_chunks()


@pytest.mark.parametrize("name,size,chunk", CORRUPT, ids=[c[0] for c in CORRUPT])
def test_corrupt_chunk(tmp_path, name, size, chunk):
    assert internal(omr.blosc_decode_host, chunk, size)
    # as a chunk of an image, of bytes so that a chunk may have any size (the decoder follows the
    # header's typesize, not the dtype's): get_tile refuses it, and a neighbour still reads
    a = chunk_pixels("uint8", np.random.default_rng(171), (1, 1, 1, 1, 2 * size))
    path = tmp_path / "c.zarr"
    omr.write_zarr(path, a, chunk=(size, 1), compressor="blosc", dimension_separator=".")
    (path / "0" / "0.0.0.0.1").write_bytes(chunk)
    with omr.ZarrImage(path, codecs=BOTH) as img:
        assert internal(img.get_tile, 0, 0, 0, 0, size, 0, 1, 1)
        assert internal(img.get_tile, 0, 0, 0, 0, 0, 0, 2 * size, 1)
        assert img.get_tile(0, 0, 0, 0, 0, 0, size, 1).tobytes() == a[0, 0, 0, 0, :size].tobytes()


def test_bad_stream_cases_reach_the_lz4_decoder():
    """Every bad stream is a case, and all but the two the csize rule stops are LZ4's to refuse."""
    lz4 = [c for c in CORRUPT if c[0].startswith("lz4: ")]
    assert len(lz4) == len(bad_streams()) == 13
    assert sum(0 < len(s) < e for _, s, e in bad_streams()) == 11
