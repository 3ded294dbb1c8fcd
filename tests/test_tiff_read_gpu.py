"""Tiled TIFF pixel data on the GPU (K13): omr_lzw_decode_batch_device (K13a) on its own, then
TiffImage.read_regions against the host route (TiffImage.get_tile), then TiffImage.render_tiles
against the ROMIO path on the same pixels.  No tolerance anywhere: decoded bytes, ARGB words and
encoded files are compared for equality.  Every output slot of the bare decoder is followed by
sixteen canary bytes that must come back unchanged."""
import zlib

import numpy as np
import pytest

import omr
from omr import _lib
from omr.context import make_qdef
from omr.synthetic import c2_channels
from omr.tiffimage import lzw_encode

pytestmark = pytest.mark.gpu

CANARY = 0xA5
TYPES = {"int8": _lib.PIXELS_INT8, "uint8": _lib.PIXELS_UINT8, "int16": _lib.PIXELS_INT16,
         "uint16": _lib.PIXELS_UINT16, "int32": _lib.PIXELS_INT32, "uint32": _lib.PIXELS_UINT32,
         "float32": _lib.PIXELS_FLOAT, "float64": _lib.PIXELS_DOUBLE}


def decode_batch(ctx, streams, expected):
    """Streams through K13a in one call: [(status, bytes)], after checking every slot's canary."""
    import torch
    n = len(streams)
    src_off, pos = [], 0
    for s in streams:
        src_off.append(pos)
        pos += len(s)
    dst_off, dpos = [], 0
    for e in expected:
        dst_off.append(dpos)
        dpos += e + 16
    src = torch.from_numpy(np.frombuffer(b"".join(streams) + b"\0", dtype=np.uint8).copy()).cuda()
    dst = torch.full((dpos,), CANARY, dtype=torch.uint8, device="cuda")
    offs = torch.tensor(src_off, dtype=torch.int64, device="cuda")
    lens = torch.tensor([len(s) for s in streams], dtype=torch.int32, device="cuda")
    exps = torch.tensor(expected, dtype=torch.int32, device="cuda")
    doff = torch.tensor(dst_off, dtype=torch.int64, device="cuda")
    stat = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    ctx.order_after_torch()
    _lib.check(_lib.lib.omr_lzw_decode_batch_device(ctx.h, src.data_ptr(), offs.data_ptr(), lens.data_ptr(),
                                                    exps.data_ptr(), n, dst.data_ptr(), doff.data_ptr(),
                                                    stat.data_ptr()), ctx.h)
    ctx.synchronize()
    out, st = dst.cpu().numpy(), stat.cpu().numpy()
    res = []
    for i in range(n):
        o, e = dst_off[i], expected[i]
        assert (out[o + e:o + e + 16] == CANARY).all(), f"canary behind segment {i} overwritten"
        res.append((int(st[i]), out[o:o + e].tobytes()))
    return res


def check_equal(ctx, datas, streams=None, expected=None):
    streams = streams or [lzw_encode(d) for d in datas]
    expected = expected or [len(d) for d in datas]
    res = decode_batch(ctx, streams, expected)
    for i, ((st, got), d, e) in enumerate(zip(res, datas, expected)):
        assert st == _lib.OK, (i, st)
        assert got == bytes(d[:e]), f"segment {i} ({e} bytes) differs"
    # the host decoder agrees
    for s, d, e in zip(streams, datas, expected):
        assert omr.lzw_decode_host(s, e) == bytes(d[:e])


def test_lzw_one_byte(ctx):
    check_equal(ctx, [b"\x07"])


def test_lzw_equal_bytes(ctx):
    # every code names the entry made just before it (code == next free), strings past 64 and 256 bytes
    check_equal(ctx, [b"\x3c" * 5000])


def test_lzw_noise_all_widths_and_table_full(ctx):
    data = np.random.default_rng(5).integers(0, 256, 65536, dtype=np.uint8).tobytes()
    stream = lzw_encode(data)
    assert len(stream) > len(data)          # noise: 9..12-bit codes, a Clear every 3836 codes
    check_equal(ctx, [data], [stream])


def test_lzw_without_eoi(ctx):
    data = np.random.default_rng(6).integers(0, 7, 3000, dtype=np.uint8).tobytes()
    with_eoi, without = lzw_encode(data), lzw_encode(data, eoi=False)
    assert len(without) <= len(with_eoi)
    check_equal(ctx, [data, data], [without, with_eoi])


def test_lzw_early_clears(ctx):
    data = np.random.default_rng(7).integers(0, 40, 20000, dtype=np.uint8).tobytes()
    check_equal(ctx, [data], [lzw_encode(data, early_clear=100)])


def test_lzw_last_string_overruns(ctx):
    data = b"\x11" * 1000 + bytes(range(200))
    for cut in (777, 999, 1001, 1100):
        check_equal(ctx, [data], [lzw_encode(data)], [cut])


def test_lzw_300_mixed_segments(ctx):
    rng = np.random.default_rng(8)
    sizes = [1 + (i * i * 37) % 4000 for i in range(296)] + [65536, 100000, 131072, 1]
    datas = []
    for i, n in enumerate(sizes):
        kind = i % 3
        if kind == 0:
            d = rng.integers(0, 256, n, dtype=np.uint8)
        elif kind == 1:
            d = rng.integers(0, 4, n, dtype=np.uint8)
        else:
            d = (np.arange(n) // (1 + i % 7)).astype(np.uint8)
        datas.append(d.tobytes())
    check_equal(ctx, datas)


def test_lzw_malformed_between_good(ctx):
    """Inputs the decoder must survive: the bad segments report OMR_INTERNAL, their neighbours
    decode, and nothing is written behind any slot."""
    rng = np.random.default_rng(9)
    good = [rng.integers(0, 9, 5000, dtype=np.uint8).tobytes() for _ in range(4)]
    gs = [lzw_encode(g) for g in good]
    # Clear, literal 5, then code 300 while the next free entry is 258
    bits = "100000000" + "000000101" + "100101100" + "100000001"
    bad_code = int(bits.ljust(40, "0"), 2).to_bytes(5, "big")
    short = gs[0][:len(gs[0]) // 2]                       # the stream ends early
    eoi_early = lzw_encode(good[1][:100])                 # EOI long before the segment is full
    lsb_first = b"\x00\x01" + gs[2][2:]                   # old-style stream
    streams = [gs[0], bad_code, gs[1], short, gs[2], eoi_early, lsb_first, gs[3], b""]
    expected = [5000, 64, 5000, 5000, 5000, 5000, 5000, 5000, 10]
    res = decode_batch(ctx, streams, expected)
    for i, g in ((0, 0), (2, 1), (4, 2), (7, 3)):
        assert res[i] == (_lib.OK, good[g]), i
    for i in (1, 3, 5, 6, 8):
        assert res[i][0] == _lib.INTERNAL, (i, res[i][0])
        with pytest.raises(omr.OmrError) as e:
            omr.lzw_decode_host(streams[i], expected[i])
        assert e.value.status == _lib.INTERNAL


# ---- regions ------------------------------------------------------------------------------------

W, H = 200, 150
SHAPES = [(1, 1, [(0, 0), (199, 149), (64, 48)]),             # 1 x 1
          (37, 29, [(45, 33), (101, 77)]),                    # odd origin, across four tiles
          (50, 40, [(150, 110)]),                             # the bottom-right edge tiles
          (200, 7, [(0, 0), (0, 143), (0, 45)])]              # full width


def _pixels(name, rng):
    if name.startswith("float"):
        a = np.round(rng.standard_normal((1, 2, 1, H, W)) * 50)
    else:
        a = rng.integers(0, 120, (1, 2, 1, H, W)) + np.arange(W)[None, None, None, None, :] // 8
    return a.astype(name)


def _region_cases():
    for name in TYPES:
        for bo in "<>":
            for pred in (1, 2):
                if name == "float64" and pred == 2:
                    continue
                for layout in ("tiles", "strips"):
                    yield name, bo, pred, layout, 5
    yield "uint16", "<", 2, "tiles", 1
    yield "uint16", ">", 1, "strips", 1
    yield "uint8", "<", 1, "tiles", 1


@pytest.mark.parametrize("name,bo,pred,layout,comp", list(_region_cases()))
def test_read_regions_equal_get_tile(ctx, tmp_path, name, bo, pred, layout, comp):
    a = _pixels(name, np.random.default_rng(zlib.crc32(repr((name, bo, pred, layout)).encode())))
    a[0, 1, 0, 96:144, 128:192] = 0                        # one tile of zeros: written with byte count 0
    path = tmp_path / "r.tif"
    kw = {"tile": (64, 48)} if layout == "tiles" else {"rows_per_strip": 48}
    omr.write_tiled_tiff(path, a, byteorder=bo, compression=comp, predictor=pred, skip_zero_segments=True, **kw)
    with omr.TiffImage(path, 1, 2, 1) as img:
        assert img.pixel_type == TYPES[name]
        bpp = a.dtype.itemsize
        for w, h, origins in SHAPES:
            reqs = [(0, c, 0, x, y) for c in (0, 1) for (x, y) in origins]
            got = img.read_regions(ctx, 0, reqs, w, h).cpu().numpy()
            for i, (z, c, t, x, y) in enumerate(reqs):
                ref = img.get_tile(0, z, c, t, x, y, w, h)
                assert ref.tobytes() == a[0, c, 0, y:y + h, x:x + w].astype(img.dtype).tobytes()
                assert got[i, :w * h * bpp].tobytes() == ref.tobytes(), (w, h, x, y, c)
        # requests that share segments, and the zero tile
        reqs = [(0, 1, 0, x, y) for (x, y) in ((100, 60), (110, 70), (100, 60), (120, 90), (0, 0))]
        got = img.read_regions(ctx, 0, reqs, 80, 60).cpu().numpy()
        for i, (z, c, t, x, y) in enumerate(reqs):
            assert got[i, :80 * 60 * bpp].tobytes() == img.get_tile(0, z, c, t, x, y, 80, 60).tobytes()


def test_read_regions_arguments(ctx, tmp_path):
    a = _pixels("uint16", np.random.default_rng(3))
    omr.write_tiled_tiff(tmp_path / "a.tif", a, tile=(64, 48), compression=5)
    with omr.TiffImage(tmp_path / "a.tif", 1, 2, 1) as img:
        for bad in [(0, 0, 0, 190, 0), (0, 2, 0, 0, 0), (0, 0, 0, -1, 0), (1, 0, 0, 0, 0)]:
            with pytest.raises(omr.OmrError) as e:
                img.read_regions(ctx, 0, [(0, 0, 0, 0, 0), bad], 16, 16)
            assert e.value.status == _lib.INVALID_ARGUMENT
        with pytest.raises(omr.OmrError):
            img.read_regions(ctx, 1, [(0, 0, 0, 0, 0)], 16, 16)
        assert img.read_regions(ctx, 0, [], 16, 16).shape[0] == 0


def test_read_regions_corrupt_segment(ctx, tmp_path):
    a = _pixels("uint8", np.random.default_rng(4))
    path = tmp_path / "c.tif"
    omr.write_tiled_tiff(path, a, tile=(64, 48), compression=5)
    with omr.TiffImage(path, 1, 2, 1) as img:
        good = img.get_tile(0, 0, 0, 0, 0, 0, 64, 48).tobytes()
    raw = bytearray(path.read_bytes())
    at = raw.index(lzw_encode(a[0, 0, 0, :48, :64].tobytes()))
    raw[at + 1] = 0xFF                                     # Clear, then a code far above 258
    raw[at + 2] = 0xFF
    path.write_bytes(raw)
    with omr.TiffImage(path, 1, 2, 1) as img:
        with pytest.raises(omr.OmrError) as e:
            img.get_tile(0, 0, 0, 0, 0, 0, 64, 48)
        assert e.value.status == _lib.INTERNAL
        with pytest.raises(omr.OmrError) as e:
            img.read_regions(ctx, 0, [(0, 0, 0, 0, 0)], 64, 48)
        assert e.value.status == _lib.INTERNAL
        got = img.read_regions(ctx, 0, [(0, 1, 0, 0, 0)], 64, 48)    # the context goes on working
        assert got.cpu().numpy()[0].tobytes() == img.get_tile(0, 0, 1, 0, 0, 0, 64, 48).tobytes()
    assert good


# ---- render -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def render_pixels():
    rng = np.random.default_rng(11)
    from omr.synthetic import microscopy_u16
    lv0 = np.stack([microscopy_u16(H, W, rng, blobs=6) for _ in range(2)])[None, :, None]
    lv1 = np.stack([microscopy_u16(75, 100, rng, blobs=4) for _ in range(2)])[None, :, None]
    return lv0, lv1


REQS0 = [(0, 0, 0, 0), (0, 0, 64, 64), (0, 0, 136, 86), (0, 0, 17, 33)]
REQS1 = [(0, 0, 0, 0), (0, 0, 36, 11)]


@pytest.mark.parametrize("bo", ["<", ">"])
def test_render_tiles_equal_romio(ctx, tmp_path, render_pixels, bo):
    import torch
    lv0, lv1 = render_pixels
    omr.write_tiled_tiff(tmp_path / "p.tif", lv0, levels=[lv1], tile=(64, 48), byteorder=bo, compression=5, predictor=2)
    omr.write_romio(tmp_path / "l0.raw", lv0, _lib.PIXELS_UINT16)
    omr.write_romio(tmp_path / "l1.raw", lv1, _lib.PIXELS_UINT16)
    qdef, chans = make_qdef("rgb"), c2_channels(2)
    with omr.TiffImage(tmp_path / "p.tif", 1, 2, 1) as img, \
            omr.PixelBuffer(tmp_path / "l0.raw", W, H, 1, 2, 1, _lib.PIXELS_UINT16) as pb0, \
            omr.PixelBuffer(tmp_path / "l1.raw", 100, 75, 1, 2, 1, _lib.PIXELS_UINT16) as pb1:
        assert img.level_sizes == [[W, H], [100, 75]]
        for fh, fv in ((False, False), (True, False), (False, True), (True, True)):
            ref = ctx.render_pixel_buffer_tiles(qdef, chans, pb0, REQS0, 64, 64, flip_h=fh, flip_v=fv)
            got = img.render_tiles(ctx, qdef, chans, 0, REQS0, 64, 64, flip_h=fh, flip_v=fv)
            assert np.array_equal(got, ref), (fh, fv)
        ref1 = ctx.render_pixel_buffer_tiles(qdef, chans, pb1, REQS1, 64, 64, flip_h=True)
        got1 = img.render_tiles(ctx, qdef, chans, 1, REQS1, 64, 64, flip_h=True)
        assert np.array_equal(got1, ref1)
        # one channel switched off, greyscale model: the first active channel only
        grey = [dict(chans[0], active=False), chans[1]]
        assert np.array_equal(img.render_tiles(ctx, make_qdef("greyscale"), grey, 0, REQS0, 64, 64),
                              ctx.render_pixel_buffer_tiles(make_qdef("greyscale"), grey, pb0, REQS0, 64, 64))

        # the device output feeds the encoders: JPEG and raw grey PNG files equal the ROMIO path's
        n = len(REQS0)
        d_ref = torch.empty((n, 64, 64), dtype=torch.int32, device="cuda")
        d_got = torch.empty((n, 64, 64), dtype=torch.int32, device="cuda")
        ctx.order_after_torch()
        ctx.render_pixel_buffer_tiles(qdef, chans, pb0, REQS0, 64, 64, out=d_ref)
        img.render_tiles(ctx, qdef, chans, 0, REQS0, 64, 64, out=d_got)
        assert ctx.encode_jpeg_batch(d_got, n, 64, 64, 0.9) == ctx.encode_jpeg_batch(d_ref, n, 64, 64, 0.9)
        raw_reqs = [(0, 1, 0, x, y) for (_, _, x, y) in REQS0]
        ref_png = pb0.tiles_png(ctx, raw_reqs, 64, 64)
        regions = img.read_regions(ctx, 0, raw_reqs, 64, 64)
        cap = _lib.lib.omr_png_gray_batch_max_bytes(64, 64, 2, n)
        out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        offs = torch.zeros(n, dtype=torch.int64, device="cuda")
        lens = torch.zeros(n, dtype=torch.int32, device="cuda")
        stat = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        ctx.order_after_torch()
        ctx.encode_png_gray_batch_device([(regions[i], 64, 0, 0) for i in range(n)], _lib.PIXELS_UINT16, 64, 64, out,
                                         offs, lens, stat, big_endian=img.big_endian)
        ctx.synchronize()
        o, l, b = offs.cpu().numpy(), lens.cpu().numpy(), out.cpu().numpy()
        assert (stat.cpu().numpy() == 0).all()
        assert [b[int(o[i]):int(o[i]) + int(l[i])].tobytes() for i in range(n)] == ref_png


def test_kernel_timing_kinds(ctx, tmp_path):
    a = _pixels("uint16", np.random.default_rng(12))
    omr.write_tiled_tiff(tmp_path / "k.tif", a, tile=(64, 48), compression=5, predictor=2)
    omr.write_tiled_tiff(tmp_path / "u.tif", a, tile=(64, 48), compression=1)
    ctx.enable_kernel_timing(True)
    try:
        ctx.kernel_timings()
        with omr.TiffImage(tmp_path / "k.tif", 1, 2, 1) as img:
            img.read_regions(ctx, 0, [(0, 0, 0, 10, 10)], 100, 100)
        assert sorted(k for _, k in ctx.kernel_timings()) == [30, 31]
        with omr.TiffImage(tmp_path / "u.tif", 1, 2, 1) as img:
            img.read_regions(ctx, 0, [(0, 0, 0, 10, 10)], 100, 100)
        assert [k for _, k in ctx.kernel_timings()] == [31]      # stored segments skip K13a
    finally:
        ctx.enable_kernel_timing(False)
