"""Reversible JPEG 2000 TIFF segments on the GPU (K19): for every file of tests/golden/tiff_j2k.npz,
TiffImage.read_regions (K19a code-blocks, K19b inverse 5/3 per level, K19c colour / level shift /
store, K13b place) equals the host route TiffImage.get_tile and the stored pixels, byte for byte,
on regions that cross tile and strip edges; TiffImage.render_tiles gives the ARGB words of the same
pixels stored uncompressed; omr_j2k_decode_batch_device equals omr_j2k_decode_host on every stream,
the truncated ones included.  No tolerance anywhere, no Pillow.  Every region of a read is followed
by canary bytes that must come back unchanged."""
import numpy as np
import pytest

import omr
import tiff_j2k_cases as jc
from omr import _lib
from omr.context import make_qdef
from omr.synthetic import c2_channels
from test_tiff_codecs_gpu import CANARY, REQS, read_checked, rgb_bindings

pytestmark = pytest.mark.gpu

# 150 x 70 in tiles of 64 x 32 or strips of 16 rows (the last of 6): across segment borders and the
# right and bottom edge, full width, 1 x 1 at corners and seams
SHAPES = [(37, 29, [(0, 0), (50, 20), (113, 41), (60, 30)]), (150, 7, [(0, 0), (0, 63), (0, 13)]),
          (1, 1, [(149, 69), (63, 31), (64, 32), (64, 0), (0, 15), (0, 16)])]


@pytest.mark.parametrize("name", jc.FILES)
def test_read_regions_equal_get_tile_and_stored_pixels(ctx, tmp_path, name):
    px = jc.pixels(name)
    n, H, W = px.shape
    with omr.TiffImage(jc.write(tmp_path, name), 1, n, 1, accept=jc.ACCEPT) as img:
        for w, h, origins in SHAPES:
            # all samples of the same pixels in one call: the channels of a pixel share their segments
            reqs = [(0, c, 0, x, y) for (x, y) in origins for c in range(n)]
            got = read_checked(ctx, img, 0, reqs, w, h)
            for i, (z, c, t, x, y) in enumerate(reqs):
                want = np.ascontiguousarray(px[c, y:y + h, x:x + w]).astype(img.dtype).tobytes()
                assert img.get_tile(0, z, c, t, x, y, w, h).tobytes() == want, (w, h, x, y, c)
                assert got[i].tobytes() == want, (w, h, x, y, c)
        got = read_checked(ctx, img, 0, [(0, c, 0, 0, 0) for c in range(n)], W, H)      # the whole image in one region
        for c in range(n):
            assert got[c].tobytes() == px[c].astype(img.dtype).tobytes(), c


def test_render_rgb_equals_uncompressed_chunky(ctx, tmp_path):
    name = "rgb_tiles_33005"
    px = jc.pixels(name)
    omr.write_tiled_tiff(tmp_path / "raw.tif", px[None, :, None], tile=(64, 32), samples_per_pixel=3)
    qdef, chans = make_qdef("rgb"), rgb_bindings()
    with omr.TiffImage(jc.write(tmp_path, name), 1, 3, 1, accept=jc.ACCEPT) as j2k, \
            omr.TiffImage(tmp_path / "raw.tif", 1, 3, 1, accept=("samples",)) as raw:
        for fh, fv in ((False, False), (True, True)):
            ref = raw.render_tiles(ctx, qdef, chans, 0, REQS, 64, 64, flip_h=fh, flip_v=fv)
            got = j2k.render_tiles(ctx, qdef, chans, 0, REQS, 64, 64, flip_h=fh, flip_v=fv)
            assert np.array_equal(got, ref), (fh, fv)
        assert len(np.unique(ref)) > 100                      # a picture, not a constant


@pytest.mark.parametrize("name", ["u16le_tiles_33004", "u16be_strips_34712"])
def test_render_16_bit_equals_uncompressed(ctx, tmp_path, name):
    px = jc.pixels(name)
    bo = ">" if name.startswith("u16be") else "<"
    omr.write_tiled_tiff(tmp_path / "raw.tif", px[None, :, None], tile=(64, 32), byteorder=bo)
    chans = c2_channels(1)
    chans[0].update(input_start=5000.0, input_end=52000.0, global_min=0.0, global_max=65535.0)
    qdef = make_qdef("greyscale")
    with omr.TiffImage(jc.write(tmp_path, name), 1, 1, 1, accept=jc.ACCEPT) as j2k, omr.TiffImage(tmp_path / "raw.tif", 1, 1, 1) as raw:
        ref = raw.render_tiles(ctx, qdef, chans, 0, REQS, 64, 64)
        got = j2k.render_tiles(ctx, qdef, chans, 0, REQS, 64, 64)
        assert np.array_equal(got, ref)
        assert len(np.unique(ref)) > 50


def test_three_channels_decode_their_segments_once(ctx, tmp_path):
    """Three channels of one pixel: one launch of K19a and of K19c with the segments of one plane,
    one launch of K19b per decomposition level (the fixture's files have two), then the place kernel."""
    name = "rgb_tiles_33005"
    px = jc.pixels(name)
    ctx.enable_kernel_timing(True)
    try:
        ctx.kernel_timings()
        with omr.TiffImage(jc.write(tmp_path, name), 1, 3, 1, accept=jc.ACCEPT) as img:
            got = read_checked(ctx, img, 0, [(0, c, 0, 0, 0) for c in range(3)], 150, 70)
            for c in range(3):
                assert got[c].tobytes() == px[c].tobytes()
        kinds = [k for _, k in ctx.kernel_timings()]
        assert kinds == [41, 42, 42, 43, 31]
    finally:
        ctx.enable_kernel_timing(False)


def test_one_segment_cut_short_fails_alone(ctx, tmp_path):
    """One damaged segment among good ones: the call that touches it is OMR_INTERNAL with nothing
    written behind any region, calls that touch its neighbours alone give their bytes, and the
    same context then reads the good file."""
    import torch
    name = "grey_tiles_33003"
    px = jc.pixels(name)
    n, H, W = px.shape
    bad = jc.patched_file(name, 1, lambda s: s[:len(s) // 2] + bytes(len(s) - len(s) // 2))
    with omr.TiffImage(jc.write(tmp_path, "bad", bad), 1, 1, 1, accept=jc.ACCEPT) as img:
        nbytes = W * H
        stride = (nbytes + 15) // 16 * 16 + 16
        out = torch.full((1, stride), CANARY, dtype=torch.uint8, device="cuda")
        ctx.order_after_torch()
        with pytest.raises(omr.OmrError) as e:
            img.read_regions(ctx, 0, [(0, 0, 0, 0, 0)], W, H, out=out, region_stride=stride)
        assert e.value.status == _lib.INTERNAL and "tiff: corrupt JPEG 2000 segment" in str(e.value)
        ctx.synchronize()
        assert (out.cpu().numpy()[:, nbytes:] == CANARY).all(), "bytes behind a region overwritten"
        got = read_checked(ctx, img, 0, [(0, 0, 0, 0, 0), (0, 0, 0, 128, 0), (0, 0, 0, 0, 32)], 22, 32)   # tiles 0, 2 and 3
        for g, (x, y) in zip(got, ((0, 0), (128, 0), (0, 32))):
            assert g.tobytes() == np.ascontiguousarray(px[0, y:y + 32, x:x + 22]).tobytes(), (x, y)
    with omr.TiffImage(jc.write(tmp_path, name), 1, 1, 1, accept=jc.ACCEPT) as img:        # the context goes on working
        assert read_checked(ctx, img, 0, [(0, 0, 0, 0, 0)], W, H)[0].tobytes() == px[0].tobytes()


def test_unsupported_segment_is_invalid_argument(ctx, tmp_path):
    name = "grey_tiles_33003"
    lossy = jc.patched_file(name, 2, lambda s: jc.edited(s, jc.COD, 9, 0))
    with omr.TiffImage(jc.write(tmp_path, "lossy", lossy), 1, 1, 1, accept=jc.ACCEPT) as img:
        with pytest.raises(omr.OmrError) as e:
            img.read_regions(ctx, 0, [(0, 0, 0, 128, 0)], 22, 16)
        assert e.value.status == _lib.INVALID_ARGUMENT and "9/7" in str(e.value)
        got = read_checked(ctx, img, 0, [(0, 0, 0, 0, 0)], 64, 32)
        assert got[0].tobytes() == np.ascontiguousarray(jc.pixels(name)[0, :32, :64]).tobytes()


@pytest.fixture(scope="module")
def host_pixels():
    """The host decoder's pixels of every stream, computed once."""
    return {name: omr.j2k_decode_host(jc.stream(name), *jc.shape_of(name)) for name in jc.STREAMS}


@pytest.mark.parametrize("samples,bits", [(1, 8), (3, 8), (1, 16)])
def test_decode_batch_device_equals_host(ctx, host_pixels, samples, bits):
    """Every stream of a sample type in one call: streams of 0, 1, 2 and 5 levels, code-blocks of 4 x 4
    up to 1024 x 4, and the truncated ones, side by side."""
    names = [n for n in jc.STREAMS if jc.shape_of(n)[2:] == (samples, bits)]
    assert len(names) >= 3
    got, status = omr.j2k_decode_batch_device(ctx, [jc.stream(n) for n in names], [jc.shape_of(n)[:2] for n in names], samples, bits)
    assert status == [_lib.OK] * len(names)
    for n, g in zip(names, got):
        assert g.dtype == host_pixels[n].dtype and g.tobytes() == host_pixels[n].tobytes(), n
        assert g.tobytes() == jc.stream_pixels(n).tobytes(), n


def test_decode_batch_device_statuses(ctx, host_pixels):
    """A damaged, an unsupported and a good stream in one call: each its own status, the good ones decoded."""
    name = "grey_41x37_cb4"
    s = jc.stream(name)
    streams = [s[:len(s) // 2], jc.edited(s, jc.COD, 9, 0), s, s]
    got, status = omr.j2k_decode_batch_device(ctx, streams, [(41, 37)] * 4, 1, 8)
    assert status == [_lib.INTERNAL, _lib.INVALID_ARGUMENT, _lib.OK, _lib.OK]
    assert got[2].tobytes() == host_pixels[name].tobytes() and got[3].tobytes() == host_pixels[name].tobytes()
    assert (got[0] == CANARY).all() and (got[1] == CANARY).all()     # a stream refused on the host is never decoded


def test_damaged_body_is_the_same_garbage_on_both_routes(ctx):
    name = "grey_33x40_nodwt"
    s = jc.with_body_damage(jc.stream(name), 5)
    got, status = omr.j2k_decode_batch_device(ctx, [s], [(33, 40)], 1, 8)
    assert status == [_lib.OK]
    assert got[0].tobytes() == omr.j2k_decode_host(s, 33, 40, 1, 8).tobytes()
