"""OME-Zarr pixel data on the host (K14): the image model (omr_zarr_image_open, its JSON reader),
the host route (ZarrImage.get_tile) against numpy, the rejections and corrupt inputs with their
status codes, and omr_inflate_host against the stdlib zlib: on the stdlib compressor's streams, and on
the forms of RFC 1951 that it never writes (zarr_streams.rare_streams, the seeded sweep), whose
census is asserted here so that the list cannot lose a case unnoticed.  No GPU."""
import json
import os
import zlib

import numpy as np
import pytest

import omr
from omr import _lib
from zarr_streams import (DEXT, LEXT, bad_streams, deflate, deflate_census, good_streams, merge_census, mixed_streams,
                          rare_streams, sweep_streams)

TYPES = {"int8": _lib.PIXELS_INT8, "uint8": _lib.PIXELS_UINT8, "int16": _lib.PIXELS_INT16,
         "uint16": _lib.PIXELS_UINT16, "int32": _lib.PIXELS_INT32, "uint32": _lib.PIXELS_UINT32,
         "float32": _lib.PIXELS_FLOAT, "float64": _lib.PIXELS_DOUBLE}
W, H = 200, 150


def pixels(name, rng, shape=(1, 2, 1, H, W)):
    if name.startswith("float"):
        a = np.round(rng.standard_normal(shape) * 50)
    else:
        a = rng.integers(0, 120, shape) + np.arange(shape[-1])[None, None, None, None, :] // 8
    return a.astype(name)


def status_of(path):
    with pytest.raises(omr.OmrError) as e:
        omr.ZarrImage(path)
    return e.value.status


@pytest.mark.parametrize("name", list(TYPES))
@pytest.mark.parametrize("bo", ["<", ">"])
@pytest.mark.parametrize("compressor", ["zlib", None])
@pytest.mark.parametrize("sep", ["/", "."])
def test_open_and_get_tile(tmp_path, name, bo, compressor, sep):
    rng = np.random.default_rng(zlib.crc32(repr((name, bo, compressor, sep)).encode()))
    a = pixels(name, rng, (2, 2, 3, H, W))
    a[1, 1, 2, 96:144, 128:192] = 0                       # one chunk of zeros: left unwritten
    lv1 = pixels(name, rng, (2, 2, 3, 75, 100))
    path = tmp_path / "img.zarr" / "0"
    omr.write_zarr(path, a, levels=[lv1], chunk=(64, 48), byteorder=bo, compressor=compressor,
                   dimension_separator=sep, skip_zero_chunks=True)
    missing = path / "0" / sep.join("11222")
    assert not missing.exists() and (path / "0" / sep.join("11221")).exists()
    with omr.ZarrImage(path) as img:
        assert img.info == {"size_x": W, "size_y": H, "size_z": 3, "size_c": 2, "size_t": 2, "pixel_type": TYPES[name],
                            "big_endian": int(bo == ">" and a.itemsize > 1), "n_levels": 2,
                            "compression": int(compressor == "zlib"), "chunk_width": 64, "chunk_height": 48,
                            "dimension_separator": ord(sep)}
        assert img.level_sizes == [[W, H], [100, 75]]
        assert img.getResolutionLevels() == 2 and img.getResolutionDescriptions() == [[W, H], [100, 75]]
        for (t, c, z, x, y, w, h) in [(0, 0, 0, 0, 0, W, H), (1, 1, 2, 0, 0, W, H), (1, 0, 1, 45, 33, 37, 29),
                                      (0, 1, 2, 199, 149, 1, 1), (1, 1, 2, 128, 96, 64, 48), (0, 0, 0, 10, 10, 0, 0)]:
            got = img.get_tile(0, z, c, t, x, y, w, h)
            assert got.dtype.itemsize == a.itemsize
            assert got.tobytes() == a[t, c, z, y:y + h, x:x + w].astype(img.dtype).tobytes(), (t, c, z, x, y, w, h)
        assert not img.get_tile(0, 2, 1, 1, 128, 96, 64, 48).any()            # the missing chunk reads as zeros
        assert img.get_tile(1, 1, 1, 0, 30, 20, 70, 55).tobytes() == lv1[0, 1, 1, 20:75, 30:100].astype(img.dtype).tobytes()
        for bad in [(0, 0, 0, 0, 150, 0, 60, 10), (0, 0, 0, 0, 0, 0, W, H + 1), (0, 3, 0, 0, 0, 0, 1, 1),
                    (0, 0, 2, 0, 0, 0, 1, 1), (0, 0, 0, 2, 0, 0, 1, 1), (2, 0, 0, 0, 0, 0, 1, 1), (1, 0, 0, 0, 50, 50, 60, 10)]:
            with pytest.raises(omr.OmrError) as e:
                img.get_tile(*bad)
            assert e.value.status == _lib.INVALID_ARGUMENT, bad


def test_bare_route_and_axes(tmp_path):
    rng = np.random.default_rng(1)
    a, lv1, lv2 = pixels("uint16", rng), pixels("uint16", rng, (1, 2, 1, 75, 100)), pixels("uint16", rng, (1, 2, 1, 38, 50))
    path = tmp_path / "g"
    omr.write_zarr(path, a, levels=[lv1, lv2], chunk=(64, 48))
    attrs = json.loads((path / ".zattrs").read_text())
    # multiscales names the levels in its own order
    attrs["multiscales"][0]["datasets"] = [{"path": "0"}, {"path": "2"}]
    (path / ".zattrs").write_text(json.dumps(attrs))
    with omr.ZarrImage(path) as img:
        assert img.level_sizes == [[W, H], [50, 38]]
        assert img.get_tile(1, 0, 1, 0, 0, 0, 50, 38).tobytes() == lv2[0, 1, 0].tobytes()
    # NGFF 0.3 axes, a list of names
    attrs["multiscales"][0]["axes"] = ["t", "c", "z", "y", "x"]
    (path / ".zattrs").write_text(json.dumps(attrs))
    with omr.ZarrImage(path) as img:
        assert img.getResolutionLevels() == 2
    attrs["multiscales"][0]["axes"] = ["t", "z", "c", "y", "x"]
    (path / ".zattrs").write_text(json.dumps(attrs))
    assert status_of(path) == _lib.INVALID_ARGUMENT
    attrs["multiscales"][0]["axes"] = ["c", "z", "y", "x"]
    (path / ".zattrs").write_text(json.dumps(attrs))
    assert status_of(path) == _lib.INVALID_ARGUMENT
    del attrs["multiscales"][0]["axes"]
    attrs["multiscales"][0]["datasets"] = [{"path": "../g/0"}]
    (path / ".zattrs").write_text(json.dumps(attrs))
    assert status_of(path) == _lib.INVALID_ARGUMENT         # a path that leaves the group
    # without multiscales: 0, 1, ... as long as they hold a .zarray
    for text in ('{"omero": {"channels": []}}', None):
        if text is None:
            os.remove(path / ".zattrs")
        else:
            (path / ".zattrs").write_text(text)
        with omr.ZarrImage(str(path) + "/") as img:
            assert img.level_sizes == [[W, H], [100, 75], [50, 38]]
            assert img.get_tile(2, 0, 0, 0, 3, 5, 40, 30).tobytes() == lv2[0, 0, 0, 5:35, 3:43].tobytes()
    os.remove(path / "1" / ".zarray")
    with omr.ZarrImage(path) as img:
        assert img.level_sizes == [[W, H]]


REJECTED = [("blosc", {"compressor": {"id": "blosc", "cname": "lz4", "clevel": 5, "shuffle": 1}}),
            ("zstd", {"compressor": {"id": "zstd", "level": 3}}),
            ("lz4", {"compressor": {"id": "lz4", "acceleration": 1}}),
            ("gzip", {"compressor": {"id": "gzip", "level": 1}}),
            ("compressor without id", {"compressor": {"level": 1}}),
            ("filter", {"filters": [{"id": "delta", "dtype": "<u2"}]}),
            ("order F", {"order": "F"}),
            ("four dimensions", {"shape": [2, 1, H, W], "chunks": [1, 1, 48, 64]}),
            ("six dimensions", {"shape": [1, 1, 2, 1, H, W], "chunks": [1, 1, 1, 1, 48, 64]}),
            ("chunk deep in t", {"shape": [2, 2, 1, H, W], "chunks": [2, 1, 1, 48, 64]}),
            ("chunk deep in c", {"chunks": [1, 2, 1, 48, 64]}),
            ("chunk deep in z", {"shape": [1, 2, 4, H, W], "chunks": [1, 1, 4, 48, 64]}),
            ("non-zero fill", {"fill_value": 7}),
            ("NaN fill", {"fill_value": "NaN"}),
            ("bool dtype", {"dtype": "|b1"}),
            ("complex dtype", {"dtype": "<c8"}),
            ("u8 dtype", {"dtype": "<u8"}),
            ("two-byte type without a byte order", {"dtype": "|u2"}),
            ("zarr_format 3", {"zarr_format": 3}),
            ("separator", {"dimension_separator": "-"}),
            ("chunk above 256 MiB", {"chunks": [1, 1, 1, 16384, 16385]})]


@pytest.mark.parametrize("what,overrides", REJECTED, ids=[r[0] for r in REJECTED])
def test_rejections(tmp_path, what, overrides):
    a = pixels("uint16", np.random.default_rng(2))
    omr.write_zarr(tmp_path / "g", a, chunk=(64, 48), zarray_overrides=overrides)
    assert status_of(tmp_path / "g") == _lib.INVALID_ARGUMENT


def test_levels_that_disagree(tmp_path):
    rng = np.random.default_rng(3)
    a, lv1 = pixels("uint16", rng), pixels("uint16", rng, (1, 2, 1, 75, 100))
    for key, value in (("dtype", "<i2"), ("dtype", ">u2"), ("compressor", None), ("shape", [1, 3, 1, 75, 100])):
        path = tmp_path / f"g_{key}_{value}".replace(" ", "")
        omr.write_zarr(path, a, levels=[lv1], chunk=(64, 48))
        meta = json.loads((path / "1" / ".zarray").read_text())
        meta[key] = value
        (path / "1" / ".zarray").write_text(json.dumps(meta))
        assert status_of(path) == _lib.INVALID_ARGUMENT, (key, value)


def test_accepted_variants(tmp_path):
    """What the writer does not write but the reader takes: fill 0.0 and null, no separator entry,
    an empty filter list."""
    a = pixels("float32", np.random.default_rng(4))
    for k, ov in enumerate(({"fill_value": 0.0}, {"fill_value": None}, {"filters": []})):
        omr.write_zarr(tmp_path / f"g{k}", a, chunk=(64, 48), zarray_overrides=ov)
        with omr.ZarrImage(tmp_path / f"g{k}") as img:
            assert img.get_tile(0, 0, 1, 0, 0, 0, W, H).tobytes() == a[0, 1, 0].tobytes()
    path = tmp_path / "dot"
    omr.write_zarr(path, a, chunk=(64, 48), dimension_separator=".")
    meta = json.loads((path / "0" / ".zarray").read_text())
    del meta["dimension_separator"]
    (path / "0" / ".zarray").write_text(json.dumps(meta))
    with omr.ZarrImage(path) as img:
        assert img.info["dimension_separator"] == ord(".")
        assert img.get_tile(0, 0, 1, 0, 5, 6, 100, 100).tobytes() == a[0, 1, 0, 6:106, 5:105].tobytes()


def test_corrupt_metadata(tmp_path):
    a = pixels("uint8", np.random.default_rng(5))
    path = tmp_path / "g"
    omr.write_zarr(path, a, chunk=(64, 48))
    zarray = path / "0" / ".zarray"
    good = zarray.read_text()
    for text in (good[:len(good) // 2], good[:-2], "", "[1, 2", good + "x", good.replace(":", " ", 1), '{"a": "\\u12"}',
                 "[" * 300 + "]" * 300, '{"a":' * 300 + "1" + "}" * 300, "nul", '"abc', "-", "1e", "\x00"):
        zarray.write_text(text)
        assert status_of(path) == _lib.INTERNAL, text[:40]
    zarray.write_text(good)
    for text in ("[" * 300 + "]" * 300, "{", '{"multiscales": [{"datasets": [{"path": "0"}]}'):
        (path / ".zattrs").write_text(text)
        assert status_of(path) == _lib.INTERNAL, text[:40]
    os.remove(path / ".zattrs")
    for ov in ({"shape": [1, 1, 1, -5, 7]}, {"shape": [1, 2, 1, 0, W]}, {"shape": [1, 2, 1, 1.5, W]},
               {"shape": [1, 2, 1, "150", W]}, {"chunks": [1, 1, 1, 48, -64]}, {"chunks": [1, 1, 1, 2 ** 40, 2 ** 40]},
               {"chunks": [1, 1, 1, 2 ** 70, 64]}, {"shape": [1, 2, 1, 2 ** 40, 2 ** 40]}):
        meta = json.loads(good)
        meta.update(ov)
        zarray.write_text(json.dumps(meta))
        assert status_of(path) == _lib.INTERNAL, ov
    zarray.write_text(good)
    with omr.ZarrImage(path) as img:
        assert img.get_tile(0, 0, 0, 0, 0, 0, W, H).tobytes() == a[0, 0, 0].tobytes()


def test_wrong_sized_raw_chunk(tmp_path):
    a = pixels("uint16", np.random.default_rng(6))
    path = tmp_path / "g"
    omr.write_zarr(path, a, chunk=(64, 48), compressor=None, dimension_separator=".")
    chunk = path / "0" / "0.0.0.1.1"
    raw = chunk.read_bytes()
    assert len(raw) == 64 * 48 * 2
    for data in (raw[:-1], raw + b"\0", b""):
        chunk.write_bytes(data)
        with omr.ZarrImage(path) as img:
            with pytest.raises(omr.OmrError) as e:
                img.get_tile(0, 0, 0, 0, 60, 40, 20, 20)
            assert e.value.status == _lib.INTERNAL
            assert img.get_tile(0, 0, 0, 0, 0, 0, 64, 48).tobytes() == a[0, 0, 0, :48, :64].tobytes()


@pytest.mark.parametrize("name,stream,expected", bad_streams(), ids=[b[0] for b in bad_streams()])
def test_malformed_stream_as_chunk(tmp_path, name, stream, expected):
    """Each malformed stream placed as a chunk whose decoded size is the stream's `expected`."""
    a = np.zeros((1, 1, 1, 3, expected), dtype=np.uint8) + 1
    path = tmp_path / "g"
    omr.write_zarr(path, a, chunk=(expected, 1), dimension_separator=".")
    (path / "0" / "0.0.0.1.0").write_bytes(stream)
    with omr.ZarrImage(path) as img:
        with pytest.raises(omr.OmrError) as e:
            img.get_tile(0, 0, 0, 0, 0, 0, expected, 3)
        assert e.value.status == _lib.INTERNAL
        assert img.get_tile(0, 0, 0, 0, 0, 2, expected, 1).all()
    with pytest.raises(omr.OmrError) as e:
        omr.inflate_host(stream, expected)
    assert e.value.status == _lib.INTERNAL


def test_missing_group(tmp_path):
    assert status_of(tmp_path / "nothing") == _lib.NOT_FOUND
    os.makedirs(tmp_path / "empty")
    assert status_of(tmp_path / "empty") == _lib.NOT_FOUND           # no first .zarray
    omr.write_zarr(tmp_path / "g", pixels("uint8", np.random.default_rng(7)), chunk=(64, 48))
    os.remove(tmp_path / "g" / "0" / ".zarray")
    assert status_of(tmp_path / "g") == _lib.NOT_FOUND
    assert status_of(tmp_path / "g" / ".zattrs") == _lib.INVALID_ARGUMENT   # a file, not a group


def test_inflate_host_equals_zlib():
    for name, data, stream in good_streams():
        assert omr.inflate_host(stream, len(data)) == data, name
    for data, stream in mixed_streams():
        assert omr.inflate_host(stream, len(data)) == data
    assert omr.inflate_host(deflate(b""), 0) == b""
    assert omr.inflate_host(deflate(b"abc") + b"trailing", 3) == b"abc"       # bytes behind the Adler-32 are not read


RARE = rare_streams()


@pytest.mark.parametrize("k", range(len(RARE)), ids=[r[0] for r in RARE])
def test_inflate_host_rare_stream(k):
    name, data, stream = RARE[k]
    assert zlib.decompress(stream) == data                 # the reference, as where the stream was made
    assert omr.inflate_host(stream, len(data)) == data
    for expected in (len(data) + 1, len(data) - 1):
        with pytest.raises(omr.OmrError) as e:
            omr.inflate_host(stream, expected)
        assert e.value.status == _lib.INTERNAL


def test_inflate_host_sweep():
    assert len(sweep_streams()) == 16
    for name, data, stream in sweep_streams():
        assert zlib.decompress(stream) == data and 200 <= len(data) <= 72000, name
        assert omr.inflate_host(stream, len(data)) == data, name


def test_census_of_the_rare_streams():
    """Conditions on the inputs, judged by the census alone (deflate_census: a plain inflater of its
    own): the rare streams and the sweep hold every form they were written for."""
    parts = {name: deflate_census(stream) for name, data, stream in RARE + sweep_streams()}
    for name, data, stream in RARE + sweep_streams():
        assert parts[name]["data"] == data, name           # the census reads the streams as zlib does
    c = merge_census(parts.values())
    assert set(c["blocks"]) == {0, 1, 2}
    for sym in range(257, 286):                            # every symbol, its extra bits all zeros and all ones
        top = (1 << LEXT[sym - 257]) - 1
        assert c["length_symbols"].get(sym, set()) >= {0, top if sym != 284 else 30}, sym
    assert 31 not in c["length_symbols"][284]              # 258 is symbol 285
    for sym in range(30):
        assert c["distance_symbols"].get(sym, set()) >= {0, (1 << DEXT[sym]) - 1}, sym
    for l in range(1, 16):
        assert c["litlen_bits"].get(l, 0) > 0 and c["dist_bits"].get(l, 0) > 0, l
    assert c["codelen_bits"].get(7, 0) > 0 and set(c["codelen_bits"]) == set(range(1, 8))
    assert c["hclen"] >= {5, 6, 19}
    assert c["crossing_repeats"] == {16, 17, 18}
    assert c["distance_sets"] == {"empty", "single"}
    assert c["overlaps"] >= set(range(1, 71)) | {127, 128, 129, 255, 256, 257}
    # what single streams were written for
    chain = parts["litlen chain 1..15, HCLEN 19"]
    assert set(chain["litlen_bits"]) == set(range(1, 16)) and chain["hclen"] == {19} and chain["codelen_bits"].get(7, 0) > 0
    deep = parts["every match symbol, deep codes"]
    assert deep["litlen_bits"][15] >= 150 and set(deep["dist_bits"]) == set(range(2, 16))
    assert set(deep["length_symbols"]) == set(range(257, 286)) and set(deep["distance_symbols"]) == set(range(30))
    assert set(parts["distance chain 1..15"]["dist_bits"]) == set(range(1, 16))
    assert parts["HCLEN 6"]["hclen"] == {6} and set(parts["HCLEN 6"]["litlen_bits"]) <= {7, 8}
    for sym in (16, 17, 18):
        assert parts[f"repeat {sym} over the border"]["crossing_repeats"] == {sym}
    assert parts["a single distance code of one bit"]["distance_sets"] == {"single"}
    assert parts["a single distance code of one bit"]["dist_bits"] == {1: 100}
    assert 16 in parts["repeat 16 of the last literal/length length over the border"]["repeats_at_hlit"]
    assert not parts["repeat 16 of the last literal/length length over the border"]["crossing_repeats"]
    assert parts["stored blocks at every bit phase"]["blocks"][0] == 8
