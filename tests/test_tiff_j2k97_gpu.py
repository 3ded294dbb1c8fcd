"""Irreversible JPEG 2000 TIFF segments on the GPU (K20): for every file of
tests/golden/tiff_j2k97.npz, TiffImage.read_regions (K19a code-blocks with the dequantiser, K20b
inverse 9/7 per level, K19c inverse ICT / rounding / level shift / store, K13b place) equals the
host route TiffImage.get_tile byte for byte, on regions that cross tile and strip edges;
omr.j2k.decode_batch_device equals omr.j2k.decode_host on every stream, reversible and irreversible
ones side by side.  Both routes run the float functions of omr_j2kdec.h without contraction, so
there is no tolerance here: the one towards OpenJPEG is the host test's.  Every region of a read is
followed by canary bytes that must come back unchanged."""
import numpy as np
import pytest

import omr
import tiff_j2k_cases as jc53
import tiff_j2k97_cases as jc
from omr import _lib, j2k
from omr.context import make_qdef
from test_tiff_codecs_gpu import CANARY, REQS, read_checked, rgb_bindings
from test_tiff_j2k_gpu import SHAPES

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", jc.FILES)
def test_read_regions_equal_get_tile(ctx, tmp_path, name):
    n, H, W = jc.pixels(name).shape
    with omr.TiffImage(jc.write(tmp_path, name), 1, n, 1, accept=jc.ACCEPT) as img:
        host = [img.get_tile(0, 0, c, 0, 0, 0, W, H) for c in range(n)]
        for w, h, origins in SHAPES:
            reqs = [(0, c, 0, x, y) for (x, y) in origins for c in range(n)]
            got = read_checked(ctx, img, 0, reqs, w, h)
            for i, (z, c, t, x, y) in enumerate(reqs):
                assert got[i].tobytes() == np.ascontiguousarray(host[c][y:y + h, x:x + w]).tobytes(), (w, h, x, y, c)
        got = read_checked(ctx, img, 0, [(0, c, 0, 0, 0) for c in range(n)], W, H)      # the whole image in one region
        for c in range(n):
            assert got[c].tobytes() == host[c].tobytes(), c
        assert len(np.unique(host[0])) > 50                       # a picture, not a constant


@pytest.fixture(scope="module")
def host_pixels():
    """The host decoder's pixels of every stream of both fixtures, computed once."""
    out = {("97", name): j2k.decode_host(jc.stream(name), *jc.shape_of(name)) for name in jc.STREAMS}
    out.update({("53", name): j2k.decode_host(jc53.stream(name), *jc53.shape_of(name)) for name in jc53.STREAMS})
    return out


@pytest.mark.parametrize("samples,bits", [(1, 8), (3, 8), (1, 16)])
def test_decode_batch_device_equals_host(ctx, host_pixels, samples, bits):
    """Every irreversible stream of a sample type in one call -- 0 to 5 levels, lines of one and two
    samples, code-blocks of 4 x 4 up to 64 x 16, truncated blocks, derived steps -- with the
    reversible streams of that type between them: K19b and K20b side by side."""
    lossy = [("97", n) for n in jc.STREAMS if jc.shape_of(n)[2:] == (samples, bits)]
    plain = [("53", n) for n in jc53.STREAMS if jc53.shape_of(n)[2:] == (samples, bits)]
    assert len(lossy) >= 2 and len(plain) >= 2
    keys = [k for pair in zip(lossy, plain) for k in pair] + lossy[len(plain):] + plain[len(lossy):]
    mod = {"97": jc, "53": jc53}
    got, status = j2k.decode_batch_device(ctx, [mod[f].stream(n) for f, n in keys], [mod[f].shape_of(n)[:2] for f, n in keys], samples, bits)
    assert status == [_lib.OK] * len(keys)
    for k, g in zip(keys, got):
        assert g.dtype == host_pixels[k].dtype and g.tobytes() == host_pixels[k].tobytes(), k
    got, status = j2k.decode_batch_device(ctx, [jc.stream(n) for _, n in lossy], [jc.shape_of(n)[:2] for _, n in lossy], samples, bits)
    assert status == [_lib.OK] * len(lossy)                    # the irreversible ones alone
    for k, g in zip(lossy, got):
        assert g.tobytes() == host_pixels[k].tobytes(), k


def test_mixed_file_in_one_call(ctx, tmp_path):
    """Segments that alternate between 9/7 and 5/3 in one read: per level one launch of K19b and one of K20b."""
    px = jc.pixels(jc.MIXED)
    ctx.enable_kernel_timing(True)
    try:
        ctx.kernel_timings()
        with omr.TiffImage(jc.write(tmp_path, jc.MIXED), 1, 1, 1, accept=jc.ACCEPT) as img:
            got = read_checked(ctx, img, 0, [(0, 0, 0, 0, 0)], 150, 70)
            assert got[0].tobytes() == img.get_tile(0, 0, 0, 0, 0, 0, 150, 70).tobytes()
            assert jc.differing(jc.MIXED) != 0 or got[0].tobytes() == px[0].tobytes()
        assert [k for _, k in ctx.kernel_timings()] == [41, 42, 44, 42, 44, 43, 31]
    finally:
        ctx.enable_kernel_timing(False)


def test_kernel_kinds_of_a_lossy_and_of_a_reversible_file(ctx, tmp_path):
    """A two-level lossy file: K19a, K20b twice, K19c, place; the reversible file through the same
    accept bits: K19b in K20b's place, the launch list of before."""
    ctx.enable_kernel_timing(True)
    try:
        for mod, want in ((jc, [41, 44, 44, 43, 31]), (jc53, [41, 42, 42, 43, 31])):
            name = "rgb_tiles_33005"
            ctx.kernel_timings()
            with omr.TiffImage(mod.write(tmp_path, name), 1, 3, 1, accept=jc.ACCEPT) as img:
                got = read_checked(ctx, img, 0, [(0, c, 0, 0, 0) for c in range(3)], 150, 70)
                for c in range(3):
                    assert got[c].tobytes() == img.get_tile(0, 0, c, 0, 0, 0, 150, 70).tobytes()
            assert [k for _, k in ctx.kernel_timings()] == want
        s = jc53.stream("grey_41x37_cb4")                          # two levels, through the new entry point
        ctx.kernel_timings()
        got, status = j2k.decode_batch_device(ctx, [s], [(41, 37)])
        assert status == [_lib.OK] and got[0].tobytes() == jc53.stream_pixels("grey_41x37_cb4").tobytes()
        assert [k for _, k in ctx.kernel_timings()] == [41, 42, 42, 43]
    finally:
        ctx.enable_kernel_timing(False)


def test_one_segment_cut_short_fails_alone(ctx, tmp_path):
    import torch
    name = "grey_tiles_33003"
    n, H, W = jc.pixels(name).shape
    bad = jc.patched_file(name, 1, lambda s: s[:len(s) // 2] + bytes(len(s) - len(s) // 2))
    with omr.TiffImage(jc.write(tmp_path, name), 1, 1, 1, accept=jc.ACCEPT) as img:
        host = img.get_tile(0, 0, 0, 0, 0, 0, W, H)
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
            assert g.tobytes() == np.ascontiguousarray(host[y:y + 32, x:x + 22]).tobytes(), (x, y)


def test_segments_of_a_kind_the_open_did_not_take_are_refused_by_name(ctx, tmp_path):
    with omr.TiffImage(jc.write(tmp_path, jc.MIXED), 1, 1, 1, accept=("jpeg2000-lossy",)) as img:
        with pytest.raises(omr.OmrError) as e:
            img.read_regions(ctx, 0, [(0, 0, 0, 64, 0)], 22, 16)                 # segment 1: reversible
        assert e.value.status == _lib.INVALID_ARGUMENT and "the reversible 5/3 transform" in str(e.value)
        got = read_checked(ctx, img, 0, [(0, 0, 0, 0, 0)], 64, 32)
        assert got[0].tobytes() == img.get_tile(0, 0, 0, 0, 0, 0, 64, 32).tobytes()
    with omr.TiffImage(jc.write(tmp_path, jc.MIXED), 1, 1, 1, accept=("jpeg2000", "samples")) as img:
        with pytest.raises(omr.OmrError) as e:
            img.read_regions(ctx, 0, [(0, 0, 0, 0, 0)], 22, 16)                  # segment 0: 9/7
        assert e.value.status == _lib.INVALID_ARGUMENT and "9/7" in str(e.value)


def test_decode_batch_device_statuses(ctx, host_pixels):
    """Refused, damaged and good streams in one call: each its own status, the good ones decoded."""
    name = "grey_41x37_cb4"
    s, r = jc.stream(name), jc53.stream(name)
    streams = [s[:len(s) // 2], jc.edited(s, jc.QCD, 0, 0, 31), s, jc.edited(s, jc.COD, 8, 1), r, s]
    got, status = j2k.decode_batch_device(ctx, streams, [(41, 37)] * 6, 1, 8)
    assert status == [_lib.INTERNAL, _lib.INVALID_ARGUMENT, _lib.OK, _lib.INVALID_ARGUMENT, _lib.OK, _lib.OK]
    assert got[2].tobytes() == host_pixels[("97", name)].tobytes() and got[5].tobytes() == got[2].tobytes()
    assert got[4].tobytes() == host_pixels[("53", name)].tobytes()
    for k in (0, 1, 3):
        assert (got[k] == CANARY).all()                        # a stream refused on the host is never decoded
    got, status = j2k.decode_batch_device(ctx, [s, r], [(41, 37)] * 2, 1, 8, irreversible=False)
    assert status == [_lib.INVALID_ARGUMENT, _lib.OK] and got[1].tobytes() == host_pixels[("53", name)].tobytes()
    got, status = omr.j2k_decode_batch_device(ctx, [s], [(41, 37)], 1, 8)       # the old entry point
    assert status == [_lib.INVALID_ARGUMENT]


def test_damaged_body_is_the_same_garbage_on_both_routes(ctx):
    s = jc.with_body_damage(jc.stream("grey_33x40_nodwt"), 5)
    got, status = j2k.decode_batch_device(ctx, [s], [(33, 40)], 1, 8)
    assert status == [_lib.OK]
    assert got[0].tobytes() == j2k.decode_host(s, 33, 40, 1, 8).tobytes()
    t = jc.with_body_damage(jc.stream("grey_150x70_cb64x16"), 6)                # through five levels of K20b
    got, status = j2k.decode_batch_device(ctx, [t], [(150, 70)], 1, 8)
    host = j2k.decode_host(t, 150, 70, 1, 8) if status == [_lib.OK] else None
    assert status != [_lib.OK] or got[0].tobytes() == host.tobytes()


def test_render_rgb_equals_uncompressed_chunky(ctx, tmp_path):
    name = "rgb_tiles_33005"
    with omr.TiffImage(jc.write(tmp_path, name), 1, 3, 1, accept=jc.ACCEPT) as img:
        px = np.stack([img.get_tile(0, 0, c, 0, 0, 0, 150, 70) for c in range(3)])
    omr.write_tiled_tiff(tmp_path / "raw.tif", px[None, :, None], tile=(64, 32), samples_per_pixel=3)
    qdef, chans = make_qdef("rgb"), rgb_bindings()
    with omr.TiffImage(jc.write(tmp_path, name), 1, 3, 1, accept=jc.ACCEPT) as lossy, \
            omr.TiffImage(tmp_path / "raw.tif", 1, 3, 1, accept=("samples",)) as raw:
        for fh, fv in ((False, False), (True, True)):
            ref = raw.render_tiles(ctx, qdef, chans, 0, REQS, 64, 64, flip_h=fh, flip_v=fv)
            got = lossy.render_tiles(ctx, qdef, chans, 0, REQS, 64, 64, flip_h=fh, flip_v=fv)
            assert np.array_equal(got, ref), (fh, fv)
        assert len(np.unique(ref)) > 100                      # a picture, not a constant
