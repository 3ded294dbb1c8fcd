"""The forms omr_tiff_image_open_ex adds to the TIFF reader, on the GPU: for every file of
tiff_codec_cases.CASES and every golden file of libtiff, TiffImage.read_regions (K14a / K16a / K13a
decoders, K13b with the strided samples, k_tiff_place_fp for Predictor 3) equals the host route
TiffImage.get_tile byte for byte, and TiffImage.render_tiles gives the ARGB words of files that
hold the same pixels in the forms the reader had before.  No tolerance anywhere.  Every region of
a read is followed by canary bytes that must come back unchanged."""
import struct

import numpy as np
import pytest

import omr
import tiff_codec_cases as tc
from omr import _lib
from omr.context import make_qdef
from omr.synthetic import c2_channels

pytestmark = pytest.mark.gpu

CANARY = 0xA5
# (w, h, origins) at level 0 (150 x 70; tiles (80, 16) or strips of 16 rows) and level 1 (75 x 35)
SHAPES0 = [(37, 29, [(0, 0), (70, 10), (113, 41), (60, 30)]),     # across segment borders, the right and bottom edge
           (150, 7, [(0, 0), (0, 63), (0, 13)]),                  # full width
           (1, 1, [(149, 69), (79, 15), (80, 16), (64, 0)])]
SHAPES1 = [(20, 9, [(0, 0), (55, 26), (30, 10)]), (75, 35, [(0, 0)])]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return tc.Files(tmp_path_factory.mktemp("tiff_codecs_gpu"))


@pytest.fixture(scope="module")
def golden(tmp_path_factory):
    return tc.load_golden(tmp_path_factory.mktemp("tiff_golden_gpu"))


def read_checked(ctx, img, level, reqs, w, h):
    """read_regions into a buffer of canaries: [n][w * h * bpp] bytes, nothing written behind a region."""
    import torch
    bpp = img.dtype.itemsize
    nbytes = w * h * bpp
    stride = (nbytes + 15) // 16 * 16 + 16
    out = torch.full((len(reqs), stride), CANARY, dtype=torch.uint8, device="cuda")
    ctx.order_after_torch()
    got = img.read_regions(ctx, level, reqs, w, h, out=out, region_stride=stride).cpu().numpy()
    assert (got[:, nbytes:] == CANARY).all(), "bytes behind a region overwritten"
    return got[:, :nbytes]


def check_image(ctx, img, size_c, shapes_by_level, pixels_by_level):
    for level, shapes in shapes_by_level.items():
        for w, h, origins in shapes:
            # all samples of the same pixels in one call: the channels of a pixel share their segments
            reqs = [(0, c, 0, x, y) for (x, y) in origins for c in range(size_c)]
            got = read_checked(ctx, img, level, reqs, w, h)
            for i, (z, c, t, x, y) in enumerate(reqs):
                ref = img.get_tile(level, z, c, t, x, y, w, h)
                want = pixels_by_level[level][c][y:y + h, x:x + w]
                assert ref.tobytes() == np.ascontiguousarray(want.astype(ref.dtype)).tobytes(), (level, w, h, x, y, c)
                assert got[i].tobytes() == ref.tobytes(), (level, w, h, x, y, c)


@pytest.mark.parametrize("case", tc.CASES, ids=repr)
def test_read_regions_equal_get_tile(ctx, files, case):
    path, lv0, lv1, _ = files.get(case)
    with case.open(path) as img:
        check_image(ctx, img, case.size_c, {0: SHAPES0, 1: SHAPES1}, {0: lv0[0, :, 0], 1: lv1[0, :, 0]})


@pytest.mark.parametrize("name", list(tc.GOLDEN_FILES))
def test_golden_read_regions_equal_get_tile(ctx, golden, name):
    path, px = golden[name]
    spp = tc.GOLDEN_FILES[name][1]
    with omr.TiffImage(path, 1, spp, 1, accept=tc.golden_need(name)) as img:
        check_image(ctx, img, spp, {0: SHAPES0}, {0: px})


def test_segments_shared_between_samples_are_decoded_once(ctx, files):
    """Three channels of one pixel: the decoder sees each segment once (one K14a launch with the
    segments of one plane), the place kernel three placements per segment."""
    case = next(c for c in tc.CASES if (c.spp, c.dtype, c.compression, c.predictor) == (3, "uint8", 8, 1))
    path, lv0, _, _ = files.get(case)
    ctx.enable_kernel_timing(True)
    try:
        ctx.kernel_timings()
        with case.open(path) as img:
            reqs = [(0, c, 0, 0, 0) for c in range(3)]
            got = read_checked(ctx, img, 0, reqs, tc.W, tc.H)
            for c in range(3):
                assert got[c].tobytes() == lv0[0, c, 0].tobytes()
        assert [k for _, k in ctx.kernel_timings()] == [32, 31]      # inflate, place: no LZW launch
    finally:
        ctx.enable_kernel_timing(False)


@pytest.mark.parametrize("comp,how", [(8, "bit"), (50000, "truncated")])
def test_read_regions_damaged_segment(ctx, tmp_path, comp, how):
    """A mid-stream byte of a zlib stream changed and a Zstandard frame cut in half: inputs of the
    kinds the K14 and K16 tests feed their decoders.  The call answers OMR_INTERNAL like the host."""
    a = tc.pixels("uint8", 2, tc.W, tc.H, 5)
    path = tmp_path / "d.tif"
    res = omr.write_tiled_tiff(path, a, tile=(80, 16), compression=comp)
    raw = bytearray(path.read_bytes())
    offs, cnts, n = tc.segment_table(raw, res["ifds"][0])
    off, cnt = struct.unpack_from("<I", raw, offs)[0], struct.unpack_from("<I", raw, cnts)[0]
    if how == "truncated":
        struct.pack_into("<I", raw, cnts, cnt // 2)
    else:
        raw[off + cnt // 2] ^= 0x55
    path.write_bytes(raw)
    with omr.TiffImage(path, 1, 2, 1, accept=("deflate", "zstd")) as img:
        with pytest.raises(omr.OmrError) as e:
            img.get_tile(0, 0, 0, 0, 0, 0, 80, 16)
        assert e.value.status == _lib.INTERNAL
        with pytest.raises(omr.OmrError) as e:
            img.read_regions(ctx, 0, [(0, 0, 0, 0, 0), (0, 1, 0, 0, 0)], 80, 16)
        assert e.value.status == _lib.INTERNAL
        assert "tiff: corrupt %s segment" % ("zlib" if comp == 8 else "zstd") in str(e.value)
        got = img.read_regions(ctx, 0, [(0, 1, 0, 0, 0)], 80, 16)    # the context goes on working
        assert got.cpu().numpy()[0, :80 * 16].tobytes() == a[0, 1, 0, :16, :80].tobytes()


# ---- render -------------------------------------------------------------------------------------

REQS = [(0, 0, 0, 0), (0, 0, 86, 6), (0, 0, 43, 3), (0, 0, 17, 5)]


def rgb_bindings():
    """Red, green and blue over the whole range of 8-bit samples."""
    chans = c2_channels(3)
    for ch, rgba in zip(chans, ((255, 0, 0, 255), (0, 255, 0, 255), (0, 0, 255, 255))):
        ch.update(rgba=rgba, input_start=0.0, input_end=255.0, global_min=0.0, global_max=255.0)
    return chans


@pytest.mark.parametrize("bo", ["<", ">"])
def test_render_rgb_deflate_equals_three_lzw_planes(ctx, tmp_path, bo):
    a = tc.pixels("uint8", 3, tc.W, tc.H, 21)
    omr.write_tiled_tiff(tmp_path / "rgb.tif", a, tile=(80, 16), byteorder=bo, compression=8, predictor=2,
                         samples_per_pixel=3)
    omr.write_tiled_tiff(tmp_path / "lzw.tif", a, tile=(80, 16), byteorder=bo, compression=5, predictor=2)
    qdef, chans = make_qdef("rgb"), rgb_bindings()
    with omr.TiffImage(tmp_path / "rgb.tif", 1, 3, 1, accept=("deflate", "samples")) as rgb, \
            omr.TiffImage(tmp_path / "lzw.tif", 1, 3, 1) as lzw:
        assert rgb.samples_per_pixel == 3 and lzw.samples_per_pixel == 1
        for fh, fv in ((False, False), (True, True)):
            ref = lzw.render_tiles(ctx, qdef, chans, 0, REQS, 64, 64, flip_h=fh, flip_v=fv)
            got = rgb.render_tiles(ctx, qdef, chans, 0, REQS, 64, 64, flip_h=fh, flip_v=fv)
            assert np.array_equal(got, ref), (fh, fv)
        assert len(np.unique(ref)) > 100                      # a picture, not a constant
        two = [dict(chans[0], active=False), chans[1], chans[2]]
        assert np.array_equal(rgb.render_tiles(ctx, qdef, two, 0, REQS, 64, 64), lzw.render_tiles(ctx, qdef, two, 0, REQS, 64, 64))


@pytest.mark.parametrize("bo", ["<", ">"])
def test_render_float_predictor3_equals_stored(ctx, tmp_path, bo):
    a = tc.pixels("float32", 2, tc.W, tc.H, 22)
    omr.write_tiled_tiff(tmp_path / "p3.tif", a, tile=(80, 16), byteorder=bo, compression=8, predictor=3)
    omr.write_tiled_tiff(tmp_path / "raw.tif", a, tile=(80, 16), byteorder=bo, compression=1)
    qdef, chans = make_qdef("rgb"), c2_channels(2)
    for ch in chans:
        ch.update(input_start=float(a.min()), input_end=float(a.max()), global_min=float(a.min()), global_max=float(a.max()))
    with omr.TiffImage(tmp_path / "p3.tif", 1, 2, 1, accept=("deflate", "predictor3")) as p3, \
            omr.TiffImage(tmp_path / "raw.tif", 1, 2, 1) as raw:
        ref = raw.render_tiles(ctx, qdef, chans, 0, REQS, 64, 64)
        got = p3.render_tiles(ctx, qdef, chans, 0, REQS, 64, 64)
        assert np.array_equal(got, ref)
        assert len(np.unique(ref)) > 20
