"""JPEG-compressed TIFF segments on the GPU (K17): for every file of tests/golden/tiff_jpeg.npz,
TiffImage.read_regions (K17a entropy decode, K17b IDCT, K17c upsample / colour / store, K13b place)
equals the host route TiffImage.get_tile and the pixels libtiff and libjpeg-turbo agree on, byte for
byte; TiffImage.render_tiles gives the ARGB words of the same pixels stored uncompressed;
omr_jpeg_decode_batch_device equals omr_jpeg_decode_host.  No tolerance anywhere, no Pillow.  Every
region of a read is followed by canary bytes that must come back unchanged."""
import numpy as np
import pytest

import omr
import tiff_jpeg_cases as jc
from omr import _lib
from omr.context import make_qdef
from test_tiff_codecs_gpu import CANARY, REQS, SHAPES0, read_checked, rgb_bindings

pytestmark = pytest.mark.gpu

# 101 x 75 in strips of 16 rows: across strip borders and the right and bottom edge, full width, 1 x 1 at corners and seams
SHAPES_ODD = [(37, 29, [(0, 0), (64, 46), (30, 10)]), (101, 7, [(0, 0), (0, 68), (0, 13)]),
              (1, 1, [(100, 74), (50, 15), (50, 16), (0, 64)])]


@pytest.mark.parametrize("name", jc.NAMES)
def test_read_regions_equal_get_tile_and_stored_pixels(ctx, tmp_path, name):
    px = jc.pixels(name)
    n, H, W = px.shape
    with omr.TiffImage(jc.write(tmp_path, name), 1, n, 1, accept=jc.ACCEPT) as img:
        for w, h, origins in (SHAPES0 if (W, H) == (150, 70) else SHAPES_ODD):
            # all samples of the same pixels in one call: the channels of a pixel share their segments
            reqs = [(0, c, 0, x, y) for (x, y) in origins for c in range(n)]
            got = read_checked(ctx, img, 0, reqs, w, h)
            for i, (z, c, t, x, y) in enumerate(reqs):
                want = np.ascontiguousarray(px[c, y:y + h, x:x + w]).tobytes()
                assert img.get_tile(0, z, c, t, x, y, w, h).tobytes() == want, (w, h, x, y, c)
                assert got[i].tobytes() == want, (w, h, x, y, c)


def test_whole_image_in_one_region(ctx, tmp_path):
    for name in ("ycc420_strips_odd", "ycc420_rst_q95_opt", "grey_strips"):
        px = jc.pixels(name)
        n, H, W = px.shape
        with omr.TiffImage(jc.write(tmp_path, name), 1, n, 1, accept=jc.ACCEPT) as img:
            got = read_checked(ctx, img, 0, [(0, c, 0, 0, 0) for c in range(n)], W, H)
            for c in range(n):
                assert got[c].tobytes() == px[c].tobytes(), (name, c)


def test_render_rgb_jpeg_equals_uncompressed_chunky(ctx, tmp_path):
    name = "ycc420_tiles_shared"
    px = jc.pixels(name)
    omr.write_tiled_tiff(tmp_path / "raw.tif", px[None, :, None], tile=(80, 16), samples_per_pixel=3)
    qdef, chans = make_qdef("rgb"), rgb_bindings()
    with omr.TiffImage(jc.write(tmp_path, name), 1, 3, 1, accept=jc.ACCEPT) as jpg, \
            omr.TiffImage(tmp_path / "raw.tif", 1, 3, 1, accept=("samples",)) as raw:
        for fh, fv in ((False, False), (True, True)):
            ref = raw.render_tiles(ctx, qdef, chans, 0, REQS, 64, 64, flip_h=fh, flip_v=fv)
            got = jpg.render_tiles(ctx, qdef, chans, 0, REQS, 64, 64, flip_h=fh, flip_v=fv)
            assert np.array_equal(got, ref), (fh, fv)
        assert len(np.unique(ref)) > 100                      # a picture, not a constant


def test_segments_shared_between_samples_are_decoded_once(ctx, tmp_path):
    """Three channels of one pixel: one launch of each decode stage with the segments of one plane,
    then the place kernel with three placements per segment."""
    name = "ycc422_tiles"
    px = jc.pixels(name)
    ctx.enable_kernel_timing(True)
    try:
        ctx.kernel_timings()
        with omr.TiffImage(jc.write(tmp_path, name), 1, 3, 1, accept=jc.ACCEPT) as img:
            got = read_checked(ctx, img, 0, [(0, c, 0, 0, 0) for c in range(3)], 150, 70)
            for c in range(3):
                assert got[c].tobytes() == px[c].tobytes()
        assert [k for _, k in ctx.kernel_timings()] == [36, 37, 38, 31]
    finally:
        ctx.enable_kernel_timing(False)


@pytest.mark.parametrize("name,variant", [("ycc420_tiles", jc.with_undefined_code), ("ycc420_rst_q30", jc.with_swapped_rst),
                                          ("grey_strips", jc.with_undefined_code)], ids=["code", "rst", "code-grey"])
def test_read_regions_damaged_segment(ctx, tmp_path, name, variant):
    """One damaged segment among good ones (an undefined code reaches K17a; a restart marker out of
    order is found by the host's pass): OMR_INTERNAL, nothing written behind any region, and the same
    context then reads a good file."""
    import torch
    px = jc.pixels(name)
    n, H, W = px.shape
    with omr.TiffImage(jc.write(tmp_path, "bad", jc.patched_file(name, 1, variant)), 1, n, 1, accept=jc.ACCEPT) as img:
        with pytest.raises(omr.OmrError) as e:
            img.get_tile(0, 0, 0, 0, 0, 0, W, H)
        assert e.value.status == _lib.INTERNAL
        nbytes = W * H
        stride = (nbytes + 15) // 16 * 16 + 16
        out = torch.full((n, stride), CANARY, dtype=torch.uint8, device="cuda")
        ctx.order_after_torch()
        with pytest.raises(omr.OmrError) as e:
            img.read_regions(ctx, 0, [(0, c, 0, 0, 0) for c in range(n)], W, H, out=out, region_stride=stride)
        assert e.value.status == _lib.INTERNAL and "tiff: corrupt JPEG segment" in str(e.value)
        ctx.synchronize()
        assert (out.cpu().numpy()[:, nbytes:] == CANARY).all(), "bytes behind a region overwritten"
    with omr.TiffImage(jc.write(tmp_path, name), 1, n, 1, accept=jc.ACCEPT) as img:    # the context goes on working
        got = read_checked(ctx, img, 0, [(0, c, 0, 0, 0) for c in range(n)], W, H)
        for c in range(n):
            assert got[c].tobytes() == px[c].tobytes()


def test_unsupported_segment_is_invalid_argument(ctx, tmp_path):
    with omr.TiffImage(jc.write(tmp_path, "p", jc.patched_file("ycc420_tiles", 1, jc.as_progressive)), 1, 3, 1,
                       accept=jc.ACCEPT) as img:
        with pytest.raises(omr.OmrError) as e:
            img.read_regions(ctx, 0, [(0, 0, 0, 70, 0)], 32, 16)
        assert e.value.status == _lib.INVALID_ARGUMENT and "progressive" in str(e.value)
        got = read_checked(ctx, img, 0, [(0, 1, 0, 0, 0)], 80, 16)
        assert got[0].tobytes() == np.ascontiguousarray(jc.pixels("ycc420_tiles")[1, :16, :80]).tobytes()


@pytest.mark.parametrize("name", jc.NAMES)
def test_decode_batch_device_equals_host(ctx, name):
    tables, segs, n, ycc = jc.streams_of(name)
    streams = [s[4] for s in segs]
    sizes = [(s[2], s[3]) for s in segs]
    got, status = omr.jpeg_decode_batch_device(ctx, streams, sizes, n, ycc, tables)
    assert status == [_lib.OK] * len(segs)
    for (x, y, w, h, stream), g in zip(segs, got):
        assert g.tobytes() == omr.jpeg_decode_host(stream, w, h, n, ycc, tables).tobytes(), (x, y)


def test_decode_batch_device_statuses(ctx):
    """A damaged, an unsupported and a good stream in one call: each its own status, the good one decoded."""
    tables, segs, n, ycc = jc.streams_of("ycc420_tiles")
    x, y, w, h, stream = segs[0]
    streams = [jc.with_undefined_code(stream), jc.as_progressive(stream), stream, stream[:len(stream) // 2]]
    got, status = omr.jpeg_decode_batch_device(ctx, streams, [(w, h)] * 4, n, ycc, tables)
    assert status == [_lib.INTERNAL, _lib.INVALID_ARGUMENT, _lib.OK, _lib.INTERNAL]
    assert got[2].tobytes() == omr.jpeg_decode_host(stream, w, h, n, ycc, tables).tobytes()
    assert (got[1] == CANARY).all() and (got[3] == CANARY).all()     # a stream refused on the host is never decoded
