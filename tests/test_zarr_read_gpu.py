"""OME-Zarr pixel data on the GPU (K14): omr_inflate_batch_device (K14a) on its own against the
stdlib zlib and the host decoder, then ZarrImage.read_regions against the host route
(ZarrImage.get_tile) and numpy, then ZarrImage.render_tiles against the TIFF and ROMIO paths on the
same pixels.  No tolerance anywhere: decoded bytes and ARGB words are compared for equality.  Every
output slot of the bare decoder is followed by sixteen canary bytes that must come back unchanged."""
import zlib

import numpy as np
import pytest

import omr
from omr import _lib
from omr.context import make_qdef
from omr.synthetic import c2_channels
from zarr_streams import bad_streams, deflate, good_streams, mixed_streams, rare_streams, sweep_streams

pytestmark = pytest.mark.gpu

CANARY = 0xA5
TYPES = {"int8": _lib.PIXELS_INT8, "uint8": _lib.PIXELS_UINT8, "int16": _lib.PIXELS_INT16,
         "uint16": _lib.PIXELS_UINT16, "int32": _lib.PIXELS_INT32, "uint32": _lib.PIXELS_UINT32,
         "float32": _lib.PIXELS_FLOAT, "float64": _lib.PIXELS_DOUBLE}


def decode_batch(ctx, streams, expected, mis=None):
    """Streams through K14a in one call: [(status, bytes)], after checking every slot's canary.
    Streams are packed byte to byte, or with `mis` each `mis` bytes behind a dword boundary."""
    import torch
    n = len(streams)
    src_off, pos, gaps = [], 0, []
    for s in streams:
        gaps.append(b"" if mis is None else b"\xEE" * ((mis - pos) % 4))
        pos += len(gaps[-1])
        src_off.append(pos)
        pos += len(s)
    dst_off, dpos = [], 0
    for e in expected:
        dst_off.append(dpos)
        dpos += e + 16
    src = torch.from_numpy(np.frombuffer(b"".join(g + s for g, s in zip(gaps, streams)) + b"\0", dtype=np.uint8).copy()).cuda()
    assert src.data_ptr() % 4 == 0
    dst = torch.full((dpos,), CANARY, dtype=torch.uint8, device="cuda")
    offs = torch.tensor(src_off, dtype=torch.int64, device="cuda")
    lens = torch.tensor([len(s) for s in streams], dtype=torch.int32, device="cuda")
    exps = torch.tensor(expected, dtype=torch.int32, device="cuda")
    doff = torch.tensor(dst_off, dtype=torch.int64, device="cuda")
    stat = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    ctx.order_after_torch()
    _lib.check(_lib.lib.omr_inflate_batch_device(ctx.h, src.data_ptr(), offs.data_ptr(), lens.data_ptr(),
                                                 exps.data_ptr(), n, dst.data_ptr(), doff.data_ptr(),
                                                 stat.data_ptr()), ctx.h)
    ctx.synchronize()
    out, st = dst.cpu().numpy(), stat.cpu().numpy()
    res = []
    for i in range(n):
        o, e = dst_off[i], expected[i]
        assert (out[o + e:o + e + 16] == CANARY).all(), f"canary behind stream {i} overwritten"
        res.append((int(st[i]), out[o:o + e].tobytes()))
    return res


def check_equal(ctx, datas, streams, mis=None):
    res = decode_batch(ctx, streams, [len(d) for d in datas], mis)
    for i, ((st, got), d, s) in enumerate(zip(res, datas, streams)):
        assert zlib.decompress(s) == d
        assert st == _lib.OK, (i, st)
        assert got == d, f"stream {i} ({len(d)} bytes) differs"
        assert omr.inflate_host(s, len(d)) == d           # the host decoder agrees


@pytest.mark.parametrize("k", range(len(good_streams())), ids=[g[0] for g in good_streams()])
def test_inflate_stream(ctx, k):
    name, data, stream = good_streams()[k]
    check_equal(ctx, [data], [stream])


def test_inflate_empty_output(ctx):
    check_equal(ctx, [b"", b"x"], [deflate(b""), deflate(b"x")])


def test_inflate_300_mixed_streams(ctx):
    datas, streams = zip(*mixed_streams())
    check_equal(ctx, list(datas), list(streams))


@pytest.mark.parametrize("k", range(len(rare_streams())), ids=[r[0] for r in rare_streams()])
def test_inflate_rare_stream(ctx, k):
    """What RFC 1951 allows and the stdlib compressor never writes, stream by stream."""
    name, data, stream = rare_streams()[k]
    check_equal(ctx, [data], [stream])


def test_inflate_rare_streams_and_sweep_in_one_call(ctx):
    both = rare_streams() + sweep_streams()
    check_equal(ctx, [b[1] for b in both], [b[2] for b in both])


@pytest.mark.parametrize("mis", [1, 2, 3])
def test_inflate_rare_streams_misaligned(ctx, mis):
    """Every rare stream `mis` bytes behind a dword boundary: the bit reader's window and the seek
    behind a stored block count from the aligned dword below the stream."""
    check_equal(ctx, [r[1] for r in rare_streams()], [r[2] for r in rare_streams()], mis)


def test_inflate_malformed_between_good(ctx):
    """Inputs the decoder must survive: the bad streams report OMR_INTERNAL, their neighbours
    decode, and nothing is written behind any slot."""
    rng = np.random.default_rng(9)
    good = [rng.integers(0, 9, 3000, dtype=np.uint8).tobytes() for _ in range(3)]
    gs = [deflate(g, lv) for g, lv in zip(good, (1, 6, 9))]
    streams, expected, bad_at = [], [], []
    for k, (name, s, e) in enumerate(bad_streams()):
        streams.append(gs[k % 3])
        expected.append(3000)
        bad_at.append(len(streams))
        streams.append(s)
        expected.append(e)
    streams.append(gs[0])
    expected.append(3000)
    res = decode_batch(ctx, streams, expected)
    for i in range(len(streams)):
        if i in bad_at:
            continue
        assert res[i] == (_lib.OK, good[(i // 2) % 3]), i
    for i, (name, s, e) in zip(bad_at, bad_streams()):
        assert res[i][0] == _lib.INTERNAL, (name, res[i][0])
        with pytest.raises(omr.OmrError) as err:
            omr.inflate_host(s, e)
        assert err.value.status == _lib.INTERNAL, name


# ---- regions ------------------------------------------------------------------------------------

W, H = 200, 150
SHAPES = [(1, 1, [(0, 0), (199, 149), (64, 48)]),             # 1 x 1
          (37, 29, [(45, 33), (101, 77)]),                    # odd origin, across four chunks
          (50, 40, [(150, 110)]),                             # the bottom-right edge chunks
          (200, 7, [(0, 0), (0, 143), (0, 45)])]              # full width


def _pixels(name, rng, shape=(1, 2, 1, H, W)):
    if name.startswith("float"):
        a = np.round(rng.standard_normal(shape) * 50)
    else:
        a = rng.integers(0, 120, shape) + np.arange(shape[-1])[None, None, None, None, :] // 8
    return a.astype(name)


@pytest.mark.parametrize("sep", ["/", "."])
@pytest.mark.parametrize("compressor", ["zlib", None])
@pytest.mark.parametrize("bo", ["<", ">"])
@pytest.mark.parametrize("name", list(TYPES))
def test_read_regions_equal_get_tile(ctx, tmp_path, name, bo, compressor, sep):
    a = _pixels(name, np.random.default_rng(zlib.crc32(repr((name, bo, compressor, sep)).encode())))
    a[0, 1, 0, 96:144, 128:192] = 0                        # one chunk of zeros: left unwritten
    path = tmp_path / "r.zarr"
    omr.write_zarr(path, a, chunk=(64, 48), byteorder=bo, compressor=compressor, dimension_separator=sep,
                   skip_zero_chunks=True, level=1 + len(name) % 9)
    assert not (path / "0" / sep.join("01022")).exists()
    with omr.ZarrImage(path) as img:
        assert img.pixel_type == TYPES[name]
        bpp = a.dtype.itemsize
        for w, h, origins in SHAPES:
            reqs = [(0, c, 0, x, y) for c in (0, 1) for (x, y) in origins]
            got = img.read_regions(ctx, 0, reqs, w, h).cpu().numpy()
            for i, (z, c, t, x, y) in enumerate(reqs):
                ref = img.get_tile(0, z, c, t, x, y, w, h)
                assert ref.tobytes() == a[0, c, 0, y:y + h, x:x + w].astype(img.dtype).tobytes()
                assert got[i, :w * h * bpp].tobytes() == ref.tobytes(), (w, h, x, y, c)
        # requests that share chunks, and the missing chunk
        reqs = [(0, 1, 0, x, y) for (x, y) in ((100, 60), (110, 70), (100, 60), (120, 90), (0, 0))]
        got = img.read_regions(ctx, 0, reqs, 80, 60).cpu().numpy()
        for i, (z, c, t, x, y) in enumerate(reqs):
            ref = img.get_tile(0, z, c, t, x, y, 80, 60)
            assert ref.tobytes() == a[0, c, 0, y:y + 60, x:x + 80].astype(img.dtype).tobytes()
            assert got[i, :80 * 60 * bpp].tobytes() == ref.tobytes()


def test_read_regions_arguments(ctx, tmp_path):
    import torch
    a = _pixels("uint16", np.random.default_rng(3))
    omr.write_zarr(tmp_path / "a.zarr", a, chunk=(64, 48))
    with omr.ZarrImage(tmp_path / "a.zarr") as img:
        for bad in [(0, 0, 0, 190, 0), (0, 2, 0, 0, 0), (0, 0, 0, -1, 0), (1, 0, 0, 0, 0)]:
            out = torch.full((2, 16 * 16 * 2), CANARY, dtype=torch.uint8, device="cuda")
            ctx.order_after_torch()
            with pytest.raises(omr.OmrError) as e:
                img.read_regions(ctx, 0, [(0, 0, 0, 0, 0), bad], 16, 16, out=out)
            assert e.value.status == _lib.INVALID_ARGUMENT
            assert (out.cpu().numpy() == CANARY).all()     # nothing written
        with pytest.raises(omr.OmrError):
            img.read_regions(ctx, 1, [(0, 0, 0, 0, 0)], 16, 16)
        assert img.read_regions(ctx, 0, [], 16, 16).shape[0] == 0


def test_read_regions_corrupt_chunk(ctx, tmp_path):
    a = _pixels("uint8", np.random.default_rng(4))
    path = tmp_path / "c.zarr"
    omr.write_zarr(path, a, chunk=(64, 48), dimension_separator=".")
    chunk = path / "0" / "0.0.0.0.0"
    raw = bytearray(chunk.read_bytes())
    raw[len(raw) // 2] ^= 0x55
    chunk.write_bytes(raw)
    with omr.ZarrImage(path) as img:
        with pytest.raises(omr.OmrError) as e:
            img.get_tile(0, 0, 0, 0, 0, 0, 64, 48)
        assert e.value.status == _lib.INTERNAL
        with pytest.raises(omr.OmrError) as e:
            img.read_regions(ctx, 0, [(0, 0, 0, 0, 0)], 64, 48)
        assert e.value.status == _lib.INTERNAL
        got = img.read_regions(ctx, 0, [(0, 1, 0, 0, 0)], 64, 48)    # the context goes on working
        assert got.cpu().numpy()[0].tobytes() == a[0, 1, 0, :48, :64].tobytes()
    # an uncompressed chunk of the wrong size
    omr.write_zarr(tmp_path / "u.zarr", a, chunk=(64, 48), compressor=None, dimension_separator=".")
    chunk = tmp_path / "u.zarr" / "0" / "0.0.0.0.0"
    chunk.write_bytes(chunk.read_bytes()[:-1])
    with omr.ZarrImage(tmp_path / "u.zarr") as img:
        with pytest.raises(omr.OmrError) as e:
            img.read_regions(ctx, 0, [(0, 0, 0, 0, 0)], 64, 48)
        assert e.value.status == _lib.INTERNAL


def test_read_regions_level_1(ctx, tmp_path):
    rng = np.random.default_rng(5)
    a, lv1 = _pixels("uint16", rng), _pixels("uint16", rng, (1, 2, 1, 75, 100))
    omr.write_zarr(tmp_path / "p.zarr", a, levels=[lv1], chunk=(64, 48), byteorder=">")
    with omr.ZarrImage(tmp_path / "p.zarr") as img:
        assert img.level_sizes == [[W, H], [100, 75]]
        reqs = [(0, 0, 0, 0, 0), (0, 1, 0, 40, 15), (0, 1, 0, 60, 35)]
        got = img.read_regions(ctx, 1, reqs, 40, 40).cpu().numpy()
        for i, (z, c, t, x, y) in enumerate(reqs):
            assert got[i, :40 * 40 * 2].tobytes() == lv1[0, c, 0, y:y + 40, x:x + 40].astype(">u2").tobytes()
            assert got[i, :40 * 40 * 2].tobytes() == img.get_tile(1, z, c, t, x, y, 40, 40).tobytes()
        with pytest.raises(omr.OmrError) as e:
            img.read_regions(ctx, 1, [(0, 0, 0, 61, 0)], 40, 40)
        assert e.value.status == _lib.INVALID_ARGUMENT


# ---- render -------------------------------------------------------------------------------------

REQS = [(0, 0, 0, 0), (0, 0, 64, 64), (0, 0, 136, 86), (0, 0, 17, 33)]


@pytest.mark.parametrize("bo", ["<", ">"])
def test_render_tiles_equal_tiff_and_romio(ctx, tmp_path, bo):
    from omr.synthetic import microscopy_u16
    rng = np.random.default_rng(11)
    lv0 = np.stack([microscopy_u16(H, W, rng, blobs=6) for _ in range(4)])[None, :, None]
    omr.write_zarr(tmp_path / "p.zarr", lv0, chunk=(64, 48), byteorder=bo, level=6)
    omr.write_tiled_tiff(tmp_path / "p.tif", lv0, tile=(64, 48), byteorder=bo, compression=5)
    omr.write_romio(tmp_path / "l0.raw", lv0, _lib.PIXELS_UINT16)
    qdef, chans = make_qdef("rgb"), c2_channels(4)
    with omr.ZarrImage(tmp_path / "p.zarr") as img, omr.TiffImage(tmp_path / "p.tif", 1, 4, 1) as tif, \
            omr.PixelBuffer(tmp_path / "l0.raw", W, H, 1, 4, 1, _lib.PIXELS_UINT16) as pb:
        for fh, fv in ((False, False), (True, False), (False, True), (True, True)):
            got = img.render_tiles(ctx, qdef, chans, 0, REQS, 64, 64, flip_h=fh, flip_v=fv)
            assert np.array_equal(got, tif.render_tiles(ctx, qdef, chans, 0, REQS, 64, 64, flip_h=fh, flip_v=fv)), (fh, fv)
            assert np.array_equal(got, ctx.render_pixel_buffer_tiles(qdef, chans, pb, REQS, 64, 64, flip_h=fh, flip_v=fv)), (fh, fv)
        # one channel switched off, greyscale model: the first active channel only
        grey = [dict(chans[0], active=False)] + list(chans[1:])
        assert np.array_equal(img.render_tiles(ctx, make_qdef("greyscale"), grey, 0, REQS, 64, 64),
                              ctx.render_pixel_buffer_tiles(make_qdef("greyscale"), grey, pb, REQS, 64, 64))


def test_kernel_timing_kinds(ctx, tmp_path):
    a = _pixels("uint16", np.random.default_rng(12))
    omr.write_zarr(tmp_path / "k.zarr", a, chunk=(64, 48))
    omr.write_zarr(tmp_path / "u.zarr", a, chunk=(64, 48), compressor=None)
    ctx.enable_kernel_timing(True)
    try:
        ctx.kernel_timings()
        with omr.ZarrImage(tmp_path / "k.zarr") as img:
            img.read_regions(ctx, 0, [(0, 0, 0, 10, 10)], 100, 100)
        assert sorted(k for _, k in ctx.kernel_timings()) == [31, 32]
        with omr.ZarrImage(tmp_path / "u.zarr") as img:
            img.read_regions(ctx, 0, [(0, 0, 0, 10, 10)], 100, 100)
        assert [k for _, k in ctx.kernel_timings()] == [31]      # stored chunks skip K14a
    finally:
        ctx.enable_kernel_timing(False)
