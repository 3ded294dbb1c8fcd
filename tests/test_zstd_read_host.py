"""Zstandard OME-Zarr chunks on the host (K16): omr_zstd_decode_host against frames of libzstd 1.4.8
(tests/golden/zstd_frames.npz), crafted and malformed ones, truncations and seeded damage;
omr_zstd_frame_forms over the fixture (the condition that the fixture reaches every branch of the
decoder); the project's encoder; omr_blosc_decode_host_ex; then omr_zarr_image_open_ex and the host
route (ZarrImage.get_tile) on Blosc-Zstd and zstd groups.  Every comparison is byte equality.  No GPU."""
import ctypes
import json

import numpy as np
import pytest

import omr
from omr import _lib
from blosc_streams import chunk_pixels
import zstd_streams as zs

ALL = ("zlib", "blosc", "blosc-zstd", "zstd")


def internal(fn, *args, **kw):
    with pytest.raises(omr.OmrError) as e:
        fn(*args, **kw)
    return e.value.status == _lib.INTERNAL


def open_status(path, **kw):
    try:
        omr.ZarrImage(path, **kw).close()
        return _lib.OK
    except omr.OmrError as e:
        return e.status


def libzstd():
    try:
        z = ctypes.CDLL("libzstd.so.1")
    except OSError:
        pytest.skip("libzstd.so.1 does not load")
    z.ZSTD_decompress.restype = ctypes.c_size_t
    z.ZSTD_decompress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]
    z.ZSTD_isError.argtypes = [ctypes.c_size_t]

    def decode(frame, cap):
        """The bytes, or None when libzstd refuses the frame."""
        out = ctypes.create_string_buffer(max(cap, 1))
        n = z.ZSTD_decompress(out, cap, frame, len(frame))
        return None if z.ZSTD_isError(n) else out.raw[:n]
    return decode


# ---- the frame decoder ----------------------------------------------------------------------------

GOOD = zs.all_good()


@pytest.mark.parametrize("k", range(len(GOOD)), ids=[g[0] for g in GOOD])
def test_zstd_decode_host(k):
    name, data, frame = GOOD[k]
    assert omr.zstd_decode_host(frame, len(data)) == data


def test_fixture_reaches_the_decoders_branches():
    """The forms libzstd wrote cover the required set, and the crafted frames the three it was not
    seen to write; every form the decoder knows is met by one of them."""
    golden, crafted = set(), set()
    for name, data, frame in zs.golden_frames():
        golden |= omr.zstd_frame_forms(frame)
    for name, data, frame in zs.crafted_frames():
        crafted |= omr.zstd_frame_forms(frame)
    assert zs.REQUIRED_FORMS <= golden, zs.REQUIRED_FORMS - golden
    assert zs.CRAFTED_FORMS <= crafted, zs.CRAFTED_FORMS - crafted
    assert golden | crafted == set(_lib.ZSTD_FORM_NAMES), set(_lib.ZSTD_FORM_NAMES) - golden - crafted
    assert np.load(zs.GOLDEN)["frame/three@l1"].size == 12


def test_frame_forms_arguments():
    assert omr.zstd_frame_forms(omr.zstd_encode(b"")) == {"BLOCK_RAW", "SINGLE_SEGMENT", "FCS_1"}
    assert internal(omr.zstd_frame_forms, b"\x28\xb5\x2f\xfd")
    words = (ctypes.c_uint32 * 2)()
    assert _lib.lib.omr_zstd_frame_forms(None, 4, words) == _lib.INVALID_ARGUMENT
    assert _lib.lib.omr_zstd_frame_forms(b"abcd", 4, None) == _lib.INVALID_ARGUMENT
    assert _lib.lib.omr_zstd_decode_host(None, 4, None, 0) == _lib.INVALID_ARGUMENT


BAD = zs.bad_frames()


@pytest.mark.parametrize("name,frame,expected", BAD, ids=[b[0] for b in BAD])
def test_zstd_bad_frame_host(name, frame, expected):
    assert internal(omr.zstd_decode_host, frame, expected)


def test_bad_frames_fail_where_they_are_meant_to():
    """The malformed frames are one change away from good ones: the unchanged ones decode."""
    d = zs.rbytes(600, 13, 5)
    assert omr.zstd_decode_host(omr.zstd_encode(d), 600) == d
    assert omr.zstd_decode_host(omr.zstd_encode(d, checksum=True), 600) == d
    hdr, blk = omr.zarrimage.zstd_frame_header, omr.zarrimage.zstd_block
    assert omr.zstd_decode_host(hdr(8, content_size=False, single_segment=False) + blk(0, b"x" * 8, True), 8) == b"x" * 8
    assert omr.zstd_decode_host(hdr(8, content_size=False, single_segment=False) + blk(1, b"x", True, 8), 8) == b"x" * 8
    # a window of 1 KiB bounds the block size: 1024 is taken, 1025 is the oversize_block case
    f = hdr(1024, content_size=False, single_segment=False) + blk(0, b"x" * 1024, True)
    assert f[5] == 0 and omr.zstd_decode_host(f, 1024) == b"x" * 1024
    # a dictionary id field that holds zero is no dictionary
    good = omr.zstd_encode(d)
    assert omr.zstd_decode_host(good[:4] + bytes([good[4] | 1]) + b"\0" + good[5:], 600) == d


@pytest.mark.parametrize("k", range(len(GOOD)), ids=[g[0] for g in GOOD])
def test_truncated_frames(k):
    name, data, frame = GOOD[k]
    for cut in zs.truncations(frame):
        assert internal(omr.zstd_decode_host, frame[:cut], len(data)), cut


def test_damaged_frames():
    """Seeded byte damage never crashes; a damaged frame that is accepted and carries a checksum
    holds the original bytes; where libzstd loads and accepts the same frame, the bytes agree."""
    try:
        ref = libzstd()
    except pytest.skip.Exception:
        ref = None
    accepted = 0
    for k, (name, data, frame) in enumerate(GOOD):
        if len(frame) > 6000:
            continue
        has_checksum = "CHECKSUM" in omr.zstd_frame_forms(frame)
        for bad in zs.damaged(frame, 60, 100 + k):
            try:
                got = omr.zstd_decode_host(bad, len(data))
            except omr.OmrError as e:
                assert e.status == _lib.INTERNAL
                continue
            accepted += 1
            if has_checksum and bad[4] & 4:
                assert got == data, name
            if ref is not None:
                theirs = ref(bad, len(data))
                if theirs is not None and len(theirs) == len(data):
                    assert theirs == got, name
    assert accepted > 0


# ---- the project's encoder ------------------------------------------------------------------------

def encoder_inputs():
    d = zs.inputs()
    return [b"", b"a", b"ab" * 3, b"abcdefgh" * 20, d["three"], d["image_5000"], d["runs_short"], d["alternating_short"], d["constant"],
            d["sparse_short"], zs.period4(40000), zs.rbytes(5000, 40), d["image_small_shuffled"] * 3,
            b"\x07" * (128 << 10) + d["runs_short"] + b"\x07" * 1000]


def test_zstd_encode_round_trips():
    for data in encoder_inputs():
        for kw in ({}, {"checksum": True}, {"single_segment": False}, {"single_segment": False, "content_size": False, "checksum": True}):
            frame = omr.zstd_encode(data, **kw)
            assert omr.zstd_decode_host(frame, len(data)) == data, (len(data), kw)
            forms = omr.zstd_frame_forms(frame)
            assert ("CHECKSUM" in forms) == bool(kw.get("checksum")) and ("WINDOWED" in forms) == (not kw.get("single_segment", True))
    forms = set()
    for data in encoder_inputs():
        forms |= omr.zstd_frame_forms(omr.zstd_encode(data))
    assert {"BLOCK_RAW", "BLOCK_RLE", "BLOCK_COMPRESSED", "LIT_RAW", "LL_PREDEFINED", "MULTI_BLOCK", "SEQ_SHORT", "SEQ_2BYTE"} <= forms
    assert len(omr.zstd_encode(zs.inputs()["runs_short"])) < 3000          # it does compress


def test_libzstd_decodes_the_projects_encoder():
    ref = libzstd()
    for data in encoder_inputs():
        for kw in ({}, {"checksum": True}, {"single_segment": False, "content_size": False}):
            assert ref(omr.zstd_encode(data, **kw), len(data)) == data, (len(data), kw)
    for name, data, frame in list(zs.crafted_frames()) + list(zs.edge_frames()):
        assert ref(frame, len(data)) == data, name
    a = zs.chunk_image()[:48, :64].tobytes()
    chunk = omr.blosc_encode(a, 2, codec="zstd")
    at = int.from_bytes(chunk[16:20], "little")
    frames = 0
    for _ in range(2):                                     # the two splits: each one frame
        csize = int.from_bytes(chunk[at:at + 4], "little")
        if csize < 3072:                                   # else the split is stored raw
            frames += 1
            assert ref(chunk[at + 4:at + 4 + csize], 3072) is not None
        at += 4 + csize
    assert at == len(chunk) and frames >= 1


# ---- Blosc with Zstd inside -----------------------------------------------------------------------

def test_blosc_decode_host_inner():
    d = zs.inputs()["image_small_shuffled"][:20000]
    zc, lc = omr.blosc_encode(d, 2, codec="zstd"), omr.blosc_encode(d, 2)
    assert zc[2] >> 5 == 4 and lc[2] >> 5 == 1
    assert omr.blosc_decode_host(zc, len(d), inner=("zstd",)) == d
    assert omr.blosc_decode_host(zc, len(d), inner=("lz4", "zstd")) == d
    assert omr.blosc_decode_host(lc, len(d), inner=("lz4", "zstd")) == d
    assert omr.blosc_decode_host(lc, len(d)) == d
    assert internal(omr.blosc_decode_host, zc, len(d))                     # LZ4 only: format 4 refused
    assert internal(omr.blosc_decode_host, zc, len(d), inner=("lz4",))
    assert internal(omr.blosc_decode_host, lc, len(d), inner=("zstd",))
    with pytest.raises(omr.OmrError) as e:
        omr.blosc_decode_host(zc, len(d), inner=())
    assert e.value.status == _lib.INVALID_ARGUMENT
    with pytest.raises(omr.OmrError) as e:
        omr.blosc_decode_host(zc, len(d), inner=("snappy",))
    assert e.value.status == _lib.INVALID_ARGUMENT
    out = np.zeros(len(d), dtype=np.uint8)
    src = np.frombuffer(zc, dtype=np.uint8)
    assert _lib.lib.omr_blosc_decode_host_ex(src.ctypes.data, src.size, out.ctypes.data, len(d), 4) == _lib.INVALID_ARGUMENT
    for shuffle in (0, 1):
        for split in (None, False):
            for ts in (1, 2, 3, 4):
                for n in (1, 700, 6144):
                    c = omr.blosc_encode(d[:n], ts, shuffle=shuffle, split=split, codec="zstd")
                    assert omr.blosc_decode_host(c, n, inner=("zstd",)) == d[:n], (shuffle, split, ts, n)
    # a damaged frame inside a sound container
    runs = zs.inputs()["runs_short"]
    rc = omr.blosc_encode(runs, 1, codec="zstd")
    bad = bytearray(rc)
    at = int.from_bytes(rc[16:20], "little") + 4           # the one stream's frame
    assert rc[at:at + 4] == b"\x28\xb5\x2f\xfd" and omr.blosc_decode_host(rc, len(runs), inner=("zstd",)) == runs
    bad[at + 1] ^= 0x55
    assert internal(omr.blosc_decode_host, bytes(bad), len(runs), inner=("zstd",))
    golden = omr.blosc_encode(zs.chunk_image()[:48, :64].tobytes(), 2, codec=zs.golden_codec)
    assert omr.blosc_decode_host(golden, 6144, inner=("zstd",)) == zs.chunk_image()[:48, :64].tobytes()


# ---- groups ---------------------------------------------------------------------------------------

W, H = 200, 150


@pytest.mark.parametrize("kind", ["blosc-zstd", "zstd"])
@pytest.mark.parametrize("bo", ["<", ">"])
@pytest.mark.parametrize("name", ["uint8", "uint16", "float32"])
def test_open_and_get_tile(tmp_path, name, bo, kind):
    a = chunk_pixels(name, np.random.default_rng(200 + len(name) + (bo == ">")), (1, 2, 1, H, W))
    a[0, 1, 0, 96:144, 128:192] = 0
    path = tmp_path / "g"
    if kind == "zstd":
        omr.write_zarr(path, a, chunk=(64, 48), byteorder=bo, compressor="zstd", skip_zero_chunks=True)
    else:
        omr.write_zarr(path, a, chunk=(64, 48), byteorder=bo, compressor="blosc", skip_zero_chunks=True, blosc={"cname": "zstd"})
    meta = json.loads((path / "0" / ".zarray").read_text())["compressor"]
    assert meta["id"] == ("zstd" if kind == "zstd" else "blosc") and meta.get("cname", "zstd") == "zstd"
    with omr.ZarrImage(path, codecs=(kind,)) as img:
        assert img.info["compression"] == (3 if kind == "zstd" else 2)
        for (x, y, w, h) in ((0, 0, W, H), (45, 33, 37, 29), (150, 110, 50, 40), (199, 149, 1, 1), (5, 5, 0, 0)):
            for c in (0, 1):
                assert img.get_tile(0, 0, c, 0, x, y, w, h).tobytes() == a[0, c, 0, y:y + h, x:x + w].astype(img.dtype).tobytes()


def test_open_rules(tmp_path):
    a = chunk_pixels("uint16", np.random.default_rng(210), (1, 1, 1, 48, 64))
    omr.write_zarr(tmp_path / "bz", a, chunk=(64, 48), compressor="blosc", blosc={"cname": "zstd"})
    omr.write_zarr(tmp_path / "bl", a, chunk=(64, 48), compressor="blosc")
    omr.write_zarr(tmp_path / "zs", a, chunk=(64, 48), compressor="zstd")
    omr.write_zarr(tmp_path / "zl", a, chunk=(64, 48))
    ok, inv = _lib.OK, _lib.INVALID_ARGUMENT
    table = {  # group: the codec sets under which it opens
        "bz": [("blosc-zstd",), ("blosc", "blosc-zstd"), ALL],
        "bl": [("blosc",), ("zlib", "blosc"), ("blosc", "blosc-zstd"), ("blosc", "zstd"), ALL],
        "zs": [("zstd",), ("zlib", "zstd"), ("blosc", "zstd"), ALL],
        "zl": [("zlib",), ("zlib", "blosc"), ("zlib", "zstd"), ALL]}
    sets = [("zlib",), ("blosc",), ("blosc-zstd",), ("zstd",), ("zlib", "blosc"), ("blosc", "blosc-zstd"), ("zlib", "zstd"),
            ("blosc", "zstd"), ALL]
    for g, opens in table.items():
        for codecs in sets:
            assert open_status(tmp_path / g, codecs=codecs) == (ok if codecs in opens else inv), (g, codecs)
    # with OMR_ZARR_CODEC_BLOSC alone a zstd group is still refused, as omr_zarr_image_open refuses all but zlib
    assert open_status(tmp_path / "bz") == inv and open_status(tmp_path / "zs") == inv
    # bit 4 stays unknown, alone and beside known bits
    for mask in (4, 3 | 4, 8 | 4, 16 | 4, 32, 31):
        opt = _lib.ZarrOpenOptions(ctypes.sizeof(_lib.ZarrOpenOptions), mask)
        h = ctypes.c_void_p()
        assert _lib.lib.omr_zarr_image_open_ex(str(tmp_path / "zl").encode(), ctypes.byref(opt), ctypes.byref(h)) == inv, mask
    with pytest.raises(omr.OmrError):
        omr.ZarrImage(tmp_path / "zl", codecs=("zstandard",))
    assert set(omr.ZarrImage.CODECS) == {"zlib", "blosc", "blosc-zstd", "zstd"}


BLOSC_REFUSED = [{"cname": "blosclz"}, {"cname": "zlib"}, {"cname": "snappy"}, {"cname": None}, {"shuffle": 2}, {"shuffle": 1.5},
                 {"cname": "lz4"}]


def test_refused_and_accepted_compressors(tmp_path):
    """Every case the Blosc open refuses stays refused with the new bits; cname lz4 is refused
    under the Zstd bit alone, as zstd is under the LZ4 bit alone."""
    a = chunk_pixels("uint16", np.random.default_rng(211), (1, 1, 1, 48, 64))
    for k, change in enumerate(BLOSC_REFUSED):
        comp = {"id": "blosc", "cname": "zstd", "clevel": 5, "shuffle": 1, "blocksize": 0}
        comp.update(change)
        comp = {key: v for key, v in comp.items() if v is not None}
        omr.write_zarr(tmp_path / f"r{k}", a, chunk=(64, 48), compressor="blosc", blosc={"cname": "zstd"},
                       zarray_overrides={"compressor": comp})
        assert open_status(tmp_path / f"r{k}", codecs=("zlib", "blosc-zstd", "zstd")) == _lib.INVALID_ARGUMENT, change
    b = chunk_pixels("uint8", np.random.default_rng(212), (1, 1, 1, 48, 64))
    omr.write_zarr(tmp_path / "u8", b, chunk=(64, 48), compressor="blosc", blosc={"cname": "zstd"},
                   zarray_overrides={"compressor": {"id": "blosc", "cname": "zstd", "shuffle": -1}})
    assert open_status(tmp_path / "u8", codecs=ALL) == _lib.INVALID_ARGUMENT
    for k, comp in enumerate([{"id": "blosc", "cname": "zstd", "shuffle": -1}, {"id": "blosc", "cname": "zstd", "clevel": "x"},
                              {"id": "zstd"}, {"id": "zstd", "level": 22, "checksum": True}]):
        kind = comp["id"]
        omr.write_zarr(tmp_path / f"a{k}", a, chunk=(64, 48), compressor=kind, blosc={"cname": "zstd"},
                       zarray_overrides={"compressor": comp})
        with omr.ZarrImage(tmp_path / f"a{k}", codecs=ALL) as img:
            assert img.get_tile(0, 0, 0, 0, 0, 0, 64, 48).tobytes() == a[0, 0, 0].tobytes()
    for other in ("lz4", "gzip", "bz2"):
        omr.write_zarr(tmp_path / other, a, chunk=(64, 48), compressor="zstd", zarray_overrides={"compressor": {"id": other}})
        assert open_status(tmp_path / other, codecs=ALL) == _lib.INVALID_ARGUMENT


def test_chunk_format_outside_the_open_set_is_corrupt(tmp_path):
    """One group holding an LZ4 chunk and a Zstd chunk: each reads only when its bit was open."""
    a = chunk_pixels("uint16", np.random.default_rng(213), (1, 1, 1, 48, 128))
    path = tmp_path / "m"
    omr.write_zarr(path, a, chunk=(64, 48), compressor="blosc", dimension_separator=".")
    (path / "0" / "0.0.0.0.1").write_bytes(omr.blosc_encode(a[0, 0, 0, :, 64:].tobytes(), 2, codec="zstd"))
    with omr.ZarrImage(path, codecs=("blosc", "blosc-zstd")) as img:
        assert img.get_tile(0, 0, 0, 0, 0, 0, 128, 48).tobytes() == a[0, 0, 0].tobytes()
    with omr.ZarrImage(path, codecs=("blosc",)) as img:
        assert img.get_tile(0, 0, 0, 0, 0, 0, 64, 48).tobytes() == a[0, 0, 0, :, :64].tobytes()
        assert internal(img.get_tile, 0, 0, 0, 0, 64, 0, 64, 48)
    meta = json.loads((path / "0" / ".zarray").read_text())
    meta["compressor"]["cname"] = "zstd"
    (path / "0" / ".zarray").write_text(json.dumps(meta))
    with omr.ZarrImage(path, codecs=("blosc-zstd",)) as img:
        assert img.get_tile(0, 0, 0, 0, 64, 0, 64, 48).tobytes() == a[0, 0, 0, :, 64:].tobytes()
        assert internal(img.get_tile, 0, 0, 0, 0, 0, 0, 64, 48)


def test_corrupt_chunks(tmp_path):
    a = chunk_pixels("uint16", np.random.default_rng(214), (1, 1, 1, 48, 128))
    for kind in ("zstd", "blosc"):
        path = tmp_path / kind
        omr.write_zarr(path, a, chunk=(64, 48), compressor=kind, dimension_separator=".", blosc={"cname": "zstd"})
        f = path / "0" / "0.0.0.0.0"
        good = f.read_bytes()
        for what, data in (("truncated", good[:-5]), ("damaged", good[:-4] + bytes([good[-4] ^ 0xFF]) + good[-3:]), ("empty frame", good[:30])):
            f.write_bytes(data)
            with omr.ZarrImage(path, codecs=ALL) as img:
                assert internal(img.get_tile, 0, 0, 0, 0, 0, 0, 64, 48), (kind, what)
                assert img.get_tile(0, 0, 0, 0, 64, 0, 64, 48).tobytes() == a[0, 0, 0, :, 64:].tobytes()
