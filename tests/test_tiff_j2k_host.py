"""Reversible JPEG 2000 TIFF segments on the host (K19): omr_j2k_decode_host gives OpenJPEG's pixels
for every stream of tests/golden/tiff_j2k.npz, byte for byte (the truncated ones included, which pin
the mid-point rule); TiffImage.get_tile gives the stored pixels of every file; the fixture reaches
every coding form omr_j2k_stream_forms knows; every form out of scope is refused by name and every
visible damage is OMR_INTERNAL; the plain open and an open_ex without the bit still refuse the
files.  No tolerance anywhere, no Pillow, no GPU."""
import os

import numpy as np
import pytest

import omr
import tiff_j2k_cases as jc
from omr import _lib


@pytest.mark.parametrize("name", jc.STREAMS)
def test_host_decoder_equals_openjpeg(name):
    w, h, n, bits = jc.shape_of(name)
    got = omr.j2k_decode_host(jc.stream(name), w, h, n, bits)
    want = jc.stream_pixels(name)
    assert got.dtype == want.dtype and got.shape == want.shape
    assert got.tobytes() == want.tobytes()


def test_fixture_covers_the_cases_of_the_issue():
    assert len(jc.TRUNCATED) == 2
    assert {"rgb_101x75_" + p for p in ("lrcp", "rlcp", "rpcl", "pcrl", "cprl")} <= set(jc.STREAMS)
    assert {"grey_1x1", "grey_33x40_nodwt", "grey_41x37_cb4", "grey_150x70_cb64x16", "grey_1100x9_cb1024x4", "grey_zero_64",
            "rgb_white_50", "u16_noise_64", "u16_smooth_128"} <= set(jc.STREAMS)
    assert any(n.startswith("grey_5x3_res") for n in jc.STREAMS)
    assert os.path.getsize(jc.GOLDEN) < 400 * 1024


def test_every_form_is_met_somewhere():
    met = set()
    for name in jc.STREAMS:
        met |= omr.j2k_stream_forms(jc.stream(name))
    assert len(_lib.J2K_FORM_NAMES) == 39 and len(set(_lib.J2K_FORM_NAMES)) == 39
    assert sorted(met) == sorted(_lib.J2K_FORM_NAMES)


@pytest.mark.parametrize("name", jc.FILES)
def test_get_tile_equals_stored_pixels(tmp_path, name):
    px = jc.pixels(name)
    n, H, W = px.shape
    with omr.TiffImage(jc.write(tmp_path, name), 1, n, 1, accept=jc.ACCEPT) as img:
        assert img.info["compression"] == 34712 and img.samples_per_pixel == n
        assert img.big_endian == name.startswith("u16be")
        for c in range(n):
            assert np.array_equal(img.get_tile(0, 0, c, 0, 0, 0, W, H), px[c]), c
            got = img.get_tile(0, 0, c, 0, 60, 29, 37, 11)           # across tile and strip borders
            assert got.tobytes() == np.ascontiguousarray(px[c, 29:40, 60:97]).astype(img.dtype).tobytes()
            assert img.get_tile(0, 0, c, 0, W - 1, H - 1, 1, 1)[0, 0] == px[c, H - 1, W - 1]


def test_files_use_every_compression_number():
    import struct
    seen = set()
    for name in jc.FILES:
        data = jc.raw(name)
        bo = "<" if data[:2] == b"II" else ">"
        at = struct.unpack_from(bo + "I", data, 4)[0]
        for k in range(struct.unpack_from(bo + "H", data, at)[0]):
            tag, typ, cnt, val = struct.unpack_from(bo + "HHIH", data, at + 2 + 12 * k)
            if tag == 259:
                seen.add(val)
    assert seen == set(_lib.J2K_COMPRESSIONS)


@pytest.mark.parametrize("name", jc.FILES)
def test_open_without_the_bit_still_refuses(tmp_path, name):
    n = jc.pixels(name).shape[0]
    path = jc.write(tmp_path, name)
    for accept in ((), ("samples",), ("deflate", "zstd", "predictor3", "samples", "jpeg")):
        with pytest.raises(omr.OmrError) as e:
            omr.TiffImage(path, 1, n, 1, accept=accept)
        assert e.value.status == _lib.INVALID_ARGUMENT


def test_open_ex_unknown_bits_and_photometric_6(tmp_path):
    import ctypes
    name = "rgb_tiles_33005"
    path = jc.write(tmp_path, name)
    h = ctypes.c_void_p()
    for bits, want in ((32 | 8, _lib.OK), (64, _lib.INVALID_ARGUMENT), (32 | 8 | 128, _lib.INVALID_ARGUMENT)):
        opt = _lib.TiffOpenOptions(ctypes.sizeof(_lib.TiffOpenOptions), bits)
        st = _lib.lib.omr_tiff_image_open_ex(path.encode(), 1, 3, 1, b"XYZCT", ctypes.byref(opt), ctypes.byref(h))
        assert st == want, bits
        if st == _lib.OK:
            _lib.lib.omr_tiff_image_close(h)
    # Photometric 6, Predictor 2 and 16-bit RGB are no JPEG 2000 forms of this reader
    px = jc.pixels(name)
    import struct
    data = bytearray(jc.raw(name))
    at = struct.unpack_from("<I", data, 4)[0]
    for k in range(struct.unpack_from("<H", data, at)[0]):
        if struct.unpack_from("<H", data, at + 2 + 12 * k)[0] == 262:
            struct.pack_into("<H", data, at + 2 + 12 * k + 8, 6)
    with pytest.raises(omr.OmrError) as e:
        omr.TiffImage(jc.write(tmp_path, "ycc", bytes(data)), 1, 3, 1, accept=jc.ACCEPT)
    assert e.value.status == _lib.INVALID_ARGUMENT
    assert px.shape[0] == 3


@pytest.mark.parametrize("what", sorted(jc.REFUSED))
def test_forms_out_of_scope_are_refused_by_name(what):
    variant, words = jc.REFUSED[what]
    name = "rgb_101x75_rpcl"
    w, h, n, bits = jc.shape_of(name)
    with pytest.raises(omr.OmrError) as e:
        omr.j2k_decode_host(variant(jc.stream(name)), w, h, n, bits)
    assert e.value.status == _lib.INVALID_ARGUMENT, what
    assert words in str(e.value) and "j2k:" in str(e.value), (what, str(e.value))


def test_sixteen_bit_rgb_and_mismatched_streams_are_refused():
    name = "rgb_101x75_lrcp"
    s = jc.stream(name)
    for c in range(3):
        s = jc.edited(s, jc.SIZ, 36 + 3 * c, 15)
    with pytest.raises(omr.OmrError) as e:
        omr.j2k_decode_host(s, 101, 75, 3, 16)
    assert e.value.status == _lib.INVALID_ARGUMENT and "16-bit samples with three components" in str(e.value)
    for args, words in (((101, 75, 1, 8), "component count"), ((101, 75, 3, 16), "precision")):
        with pytest.raises(omr.OmrError) as e:
            omr.j2k_decode_host(jc.stream(name), *args)
        assert e.value.status == _lib.INVALID_ARGUMENT and words in str(e.value)
    with pytest.raises(omr.OmrError) as e:                          # more than 30 magnitude bit-planes: guard bits 7, exponent 31
        t = jc.edited(jc.stream(name), jc.QCD, 0, 7 << 5, 0xE0)
        omr.j2k_decode_host(jc.edited(t, jc.QCD, 1, 31 << 3), 101, 75, 3, 8)
    assert e.value.status == _lib.INVALID_ARGUMENT and "30 magnitude bit-planes" in str(e.value)


@pytest.mark.parametrize("what", sorted(jc.DAMAGED))
@pytest.mark.parametrize("name", ["rgb_101x75_cprl", "u16_noise_64"])
def test_visible_damage_is_internal(name, what):
    w, h, n, bits = jc.shape_of(name)
    with pytest.raises(omr.OmrError) as e:
        omr.j2k_decode_host(jc.DAMAGED[what](jc.stream(name)), w, h, n, bits)
    assert e.value.status == _lib.INTERNAL, (what, str(e.value))
    assert str(e.value).count("j2k:") == 1


def test_frame_size_other_than_the_segments_is_internal():
    with pytest.raises(omr.OmrError) as e:
        omr.j2k_decode_host(jc.stream("grey_41x37_cb4"), 41, 38, 1, 8)
    assert e.value.status == _lib.INTERNAL and "frame size" in str(e.value)


def test_every_truncation_fails_cleanly():
    for name in ("grey_41x37_cb4", "rgb_white_50", "grey_5x3_res2" if "grey_5x3_res2" in jc.STREAMS else "grey_1x1"):
        s = jc.stream(name)
        w, h, n, bits = jc.shape_of(name)
        for k in range(len(s)):
            with pytest.raises(omr.OmrError) as e:
                omr.j2k_decode_host(s[:k], w, h, n, bits)
            assert e.value.status in (_lib.INTERNAL, _lib.INVALID_ARGUMENT), k


def test_empty_packet_decodes_to_the_flat_picture():
    """OpenJPEG writes `nothing included` where the standard also allows an empty packet: the same pixels."""
    name = "grey_flat128_8_nodwt"
    got = omr.j2k_decode_host(jc.with_empty_packet(jc.stream(name)), 8, 8, 1, 8)
    assert got.tobytes() == jc.stream_pixels(name).tobytes() and (got == 128).all()


def test_damaged_packet_body_is_defined_garbage():
    """A code-block's bytes cannot be checked without the refused termination styles: OMR_OK, pixels
    in range, and the same pixels on every run."""
    name = "grey_33x40_nodwt"                                       # one packet: the second half of it is body
    s = jc.with_body_damage(jc.stream(name), 5)
    a = omr.j2k_decode_host(s, 33, 40, 1, 8)
    b = omr.j2k_decode_host(s, 33, 40, 1, 8)
    assert a.tobytes() == b.tobytes() and a.tobytes() != jc.stream_pixels(name).tobytes()


def test_damaged_segment_of_a_file(tmp_path):
    name = "grey_tiles_33003"
    px = jc.pixels(name)
    bad = jc.patched_file(name, 1, lambda s: s[:len(s) // 2] + bytes(len(s) - len(s) // 2))
    with omr.TiffImage(jc.write(tmp_path, "bad", bad), 1, 1, 1, accept=jc.ACCEPT) as img:
        with pytest.raises(omr.OmrError) as e:
            img.get_tile(0, 0, 0, 0, 64, 0, 64, 32)
        assert e.value.status == _lib.INTERNAL
        assert np.array_equal(img.get_tile(0, 0, 0, 0, 0, 0, 64, 32), px[0, :32, :64])     # its neighbours read on
    nine_seven = jc.patched_file(name, 2, lambda s: jc.edited(s, jc.COD, 9, 0))
    with omr.TiffImage(jc.write(tmp_path, "lossy", nine_seven), 1, 1, 1, accept=jc.ACCEPT) as img:
        with pytest.raises(omr.OmrError) as e:
            img.get_tile(0, 0, 0, 0, 128, 0, 22, 32)
        assert e.value.status == _lib.INVALID_ARGUMENT
