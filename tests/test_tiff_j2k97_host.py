"""Irreversible JPEG 2000 (K20) on the host: the float path of omr_j2kdec.h -- dequantiser, inverse
9/7 lifting, inverse ICT, rounding and clamp -- through omr.j2k.decode_host and TiffImage.get_tile
against OpenJPEG's pixels in tests/golden/tiff_j2k97.npz, under the rule the fixture's tool states
(tiff_j2k97_cases.assert_agrees_with_openjpeg); the switches that open the path and what stays
refused behind them.  No GPU, no Pillow."""
import ctypes

import numpy as np
import pytest

import omr
import tiff_j2k_cases as jc53
import tiff_j2k97_cases as jc
from omr import _lib, j2k


@pytest.mark.parametrize("name", jc.STREAMS)
def test_host_decoder_against_openjpeg(name):
    w, h, n, bits = jc.shape_of(name)
    got = j2k.decode_host(jc.stream(name), w, h, n, bits)
    jc.assert_agrees_with_openjpeg(got, jc.stream_pixels(name), name)
    assert got.tobytes() == j2k.decode_host(jc.stream(name), w, h, n, bits).tobytes()     # deterministic


def test_the_fixture_pins_what_it_says():
    assert jc.OPENJPEG.startswith("2.")
    assert len(jc.STREAMS) >= 16 and len(jc.FILES) == 6
    px = jc.stream_pixels("grey_grid_101x75")
    assert px.min() == 0 and px.max() == 255                     # the clamp at both ends
    assert all(jc.differing(n) >= 0 for n in jc.STREAMS + jc.FILES)


def test_every_lossy_form_is_met():
    met, plain = set(), set()
    for name in jc.STREAMS:
        forms, lossy = j2k.stream_forms(jc.stream(name))
        assert "W97" in lossy and "RCT" not in forms, name
        met |= lossy
        plain |= forms
    assert met == set(_lib.J2K_LOSSY_FORM_NAMES)
    assert {"ZC0", "MR16", "RUN_BROKEN", "LATE_INCLUSION", "TAG_TREE_DEEP", "PARTIAL_BLOCK"} <= plain   # tier 1 and 2 are K19's
    forms, lossy = j2k.stream_forms(jc53.stream("rgb_101x75_rpcl"))                                     # a reversible stream
    assert lossy == set() and forms == omr.j2k_stream_forms(jc53.stream("rgb_101x75_rpcl"))
    kinds = [bool(j2k.stream_forms(jc.segment_bytes(jc.MIXED, k))[1]) for k in range(9)]
    assert kinds == [True, False] * 4 + [True]


@pytest.mark.parametrize("name", jc.FILES)
def test_get_tile_against_openjpeg(tmp_path, name):
    px = jc.pixels(name)
    n, H, W = px.shape
    with omr.TiffImage(jc.write(tmp_path, name), 1, n, 1, accept=jc.ACCEPT) as img:
        whole = np.stack([img.get_tile(0, 0, c, 0, 0, 0, W, H) for c in range(n)])
        jc.assert_agrees_with_openjpeg(whole.astype(px.dtype), px, name)
        for (x, y, w, h) in ((50, 20, 37, 29), (149, 69, 1, 1), (0, 13, 150, 7), (64, 32, 1, 1)):
            for c in range(n):
                assert np.array_equal(img.get_tile(0, 0, c, 0, x, y, w, h), whole[c, y:y + h, x:x + w]), (x, y, c)


def test_without_the_lossy_bit_a_lossy_file_is_still_refused(tmp_path):
    name = "grey_tiles_33003"
    with omr.TiffImage(jc.write(tmp_path, name), 1, 1, 1, accept=("jpeg2000", "samples")) as img:   # it opens: the transform is a segment's
        with pytest.raises(omr.OmrError) as e:
            img.get_tile(0, 0, 0, 0, 0, 0, 64, 32)
        assert e.value.status == _lib.INVALID_ARGUMENT
    with pytest.raises(omr.OmrError) as e:
        j2k.decode_host(jc.segment_bytes(name, 0), 64, 32, irreversible=False)
    assert e.value.status == _lib.INVALID_ARGUMENT and "9/7" in str(e.value)
    for accept in ((), ("samples", "jpeg")):
        with pytest.raises(omr.OmrError) as e:
            omr.TiffImage(jc.write(tmp_path, name), 1, 1, 1, accept=accept)
        assert e.value.status == _lib.INVALID_ARGUMENT


def test_the_lossy_bit_alone_refuses_reversible_segments(tmp_path):
    px = jc.pixels(jc.MIXED)
    with omr.TiffImage(jc.write(tmp_path, jc.MIXED), 1, 1, 1, accept=("jpeg2000-lossy",)) as img:
        assert np.array_equal(img.get_tile(0, 0, 0, 0, 0, 0, 64, 32), px[0, :32, :64])               # segment 0: 9/7
        with pytest.raises(omr.OmrError) as e:
            img.get_tile(0, 0, 0, 0, 64, 0, 64, 32)                                                  # segment 1: 5/3
        assert e.value.status == _lib.INVALID_ARGUMENT
    with omr.TiffImage(jc53.write(tmp_path, "grey_tiles_33003"), 1, 1, 1, accept=("jpeg2000-lossy",)) as img:   # K19's file
        with pytest.raises(omr.OmrError) as e:
            img.get_tile(0, 0, 0, 0, 0, 0, 64, 32)
        assert e.value.status == _lib.INVALID_ARGUMENT
    with omr.TiffImage(jc.write(tmp_path, jc.MIXED), 1, 1, 1, accept=("jpeg2000",)) as img:
        assert np.array_equal(img.get_tile(0, 0, 0, 0, 64, 0, 64, 32), px[0, :32, 64:128])
        with pytest.raises(omr.OmrError) as e:
            img.get_tile(0, 0, 0, 0, 0, 0, 64, 32)
        assert e.value.status == _lib.INVALID_ARGUMENT


def test_transform_and_quantisation_style_must_match():
    s = jc.stream("grey_41x37_cb4")
    with pytest.raises(omr.OmrError) as e:                          # 9/7 with QCD style 0
        j2k.decode_host(jc.edited(s, jc.QCD, 0, 0, 31), 41, 37)
    assert e.value.status == _lib.INVALID_ARGUMENT and "9/7 transform without quantisation" in str(e.value)
    r = jc53.stream("grey_41x37_cb4")
    for style in (1, 2):                                            # 5/3 with style 1 or 2
        with pytest.raises(omr.OmrError) as e:
            j2k.decode_host(jc.edited(r, jc.QCD, 0, style, 31), 41, 37)
        assert e.value.status == _lib.INVALID_ARGUMENT and "5/3 transform with scalar quantisation" in str(e.value)
    with pytest.raises(omr.OmrError) as e:                          # 5/3 with its style kept, the transform byte 0
        j2k.decode_host(jc.edited(r, jc.COD, 9, 0), 41, 37)
    assert e.value.status == _lib.INVALID_ARGUMENT and "9/7 transform without quantisation" in str(e.value)
    with pytest.raises(omr.OmrError) as e:
        j2k.decode_host(jc.edited(s, jc.COD, 9, 2), 41, 37)
    assert e.value.status == _lib.INVALID_ARGUMENT and "transform other than" in str(e.value)
    assert np.array_equal(j2k.decode_host(r, 41, 37), jc53.stream_pixels("grey_41x37_cb4"))   # the flag takes reversible streams too


@pytest.mark.parametrize("what", sorted(set(jc.REFUSED) - set(jc.NOW_ALLOWED)))
def test_forms_out_of_scope_stay_refused_under_the_flag(what):
    variant, words = jc.REFUSED[what]
    name = "rgb_101x75_rpcl"
    w, h, n, bits = jc.shape_of(name)
    with pytest.raises(omr.OmrError) as e:
        j2k.decode_host(variant(jc.stream(name)), w, h, n, bits)
    assert e.value.status == _lib.INVALID_ARGUMENT, what
    assert words in str(e.value) and "j2k:" in str(e.value), (what, str(e.value))


@pytest.mark.parametrize("what", sorted(jc.DAMAGED))
@pytest.mark.parametrize("name", ["rgb_101x75_cprl", "u16_noise_64"])
def test_visible_damage_is_internal(name, what):
    w, h, n, bits = jc.shape_of(name)
    with pytest.raises(omr.OmrError) as e:
        j2k.decode_host(jc.DAMAGED[what](jc.stream(name)), w, h, n, bits)
    assert e.value.status == _lib.INTERNAL, (what, str(e.value))


def test_bad_quantisation_segments():
    s = jc.stream("grey_41x37_derived")
    at = jc.marker_at(s, jc.QCD)
    longer = s[:at + 2] + b"\x00\x06" + s[at + 4:at + 7] + b"\x00" + s[at + 7:]      # style 1 with three bytes behind Sqcd
    with pytest.raises(omr.OmrError) as e:
        j2k.decode_host(longer, 41, 37)
    assert e.value.status == _lib.INTERNAL and "bad QCD" in str(e.value)
    t = jc.stream("grey_41x37_cb4")
    at = jc.marker_at(t, jc.QCD)
    n = int.from_bytes(t[at + 2:at + 4], "big")
    shorter = t[:at + 2] + (n - 2).to_bytes(2, "big") + t[at + 4:at + 2 + n - 2] + t[at + 2 + n:]   # style 2 without its last subband
    with pytest.raises(omr.OmrError) as e:
        j2k.decode_host(shorter, 41, 37)
    assert e.value.status == _lib.INTERNAL and "too few subbands" in str(e.value)


def test_every_truncation_fails():
    for name in ("grey_41x37_derived", "grey_9x1_res2", "grey_5x2_res2"):
        s = jc.stream(name)
        w, h, n, bits = jc.shape_of(name)
        for k in range(len(s)):
            with pytest.raises(omr.OmrError) as e:
                j2k.decode_host(s[:k], w, h, n, bits)
            assert e.value.status in (_lib.INTERNAL, _lib.INVALID_ARGUMENT), k


def test_a_damaged_body_is_defined_garbage():
    name = "grey_33x40_nodwt"
    s = jc.with_body_damage(jc.stream(name), 5)
    assert j2k.decode_host(s, 33, 40).tobytes() == j2k.decode_host(s, 33, 40).tobytes()


@pytest.mark.parametrize("name", jc.STREAMS)
def test_the_old_entry_points_refuse_lossy_streams(name):
    w, h, n, bits = jc.shape_of(name)
    with pytest.raises(omr.OmrError) as e:
        omr.j2k_decode_host(jc.stream(name), w, h, n, bits)
    assert e.value.status == _lib.INVALID_ARGUMENT and "j2k: the irreversible 9/7 transform" in str(e.value)
    with pytest.raises(omr.OmrError) as e:
        j2k.decode_host(jc.stream(name), w, h, n, bits, irreversible=False)
    assert e.value.status == _lib.INVALID_ARGUMENT and "j2k: the irreversible 9/7 transform" in str(e.value)
    with pytest.raises(omr.OmrError) as e:
        omr.j2k_stream_forms(jc.stream(name))
    assert e.value.status == _lib.INVALID_ARGUMENT


def test_unknown_flags_and_the_public_names():
    s = np.frombuffer(jc.stream("grey_5x2_res2"), np.uint8)
    out = np.zeros(10, np.uint8)
    st = _lib.lib.omr_j2k_decode_host_ex(s.ctypes.data, s.size, 5, 2, 1, 8, 2, out.ctypes.data, None, 0)
    assert st == _lib.INVALID_ARGUMENT
    bits = ctypes.c_uint64(0)
    assert _lib.lib.omr_j2k_stream_forms_ex(s.ctypes.data, s.size, 4, ctypes.byref(bits), None) == _lib.INVALID_ARGUMENT
    assert _lib.lib.omr_j2k_stream_forms_ex(s.ctypes.data, s.size, 1, ctypes.byref(bits), None) == _lib.OK   # lossy_forms may be NULL
    assert _lib.TIFF_ACCEPT["jpeg2000-lossy"] == 64 and _lib.J2K_ALLOW_IRREVERSIBLE == 1
    assert len(_lib.J2K_LOSSY_FORM_NAMES) == 9
    assert omr.j2k is j2k and "j2k" not in omr.__all__
    assert not hasattr(omr.tiffimage, "decode_host")


def test_write_tiled_tiff_irreversible_option(tmp_path):
    pytest.importorskip("PIL")
    a = np.arange(64 * 32, dtype=np.uint32).reshape(32, 64).astype(np.uint8)
    for irreversible in (False, True):
        path = tmp_path / ("w%d.tif" % irreversible)
        omr.write_tiled_tiff(path, a[None, None, None], tile=(64, 32), compression=34712,
                             jpeg2000={"irreversible": irreversible, "num_resolutions": 2})
        seg = jc.segments_of(open(path, "rb").read())[0]
        data = open(path, "rb").read()[seg[4]:seg[4] + seg[5]]
        assert bool(j2k.stream_forms(data)[1]) == irreversible
