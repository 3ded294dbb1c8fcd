"""Blosc OME-Zarr chunks on the GPU (K15): omr_lz4_decode_batch_device (K15a) on its own against
streams of a real encoder, crafted and malformed ones and the host decoder, then
ZarrImage.read_regions on Blosc groups against the host route (ZarrImage.get_tile) and numpy, then
ZarrImage.render_tiles against the same pixels in a zlib group.  No tolerance anywhere: decoded
bytes and ARGB words are compared for equality.  Every output slot of the bare decoder is followed
by sixteen canary bytes that must come back unchanged."""
import zlib

import numpy as np
import pytest

import omr
from omr import _lib
from omr.context import make_qdef
from omr.synthetic import c2_channels
from blosc_streams import (bad_streams, chunk_pixels, crafted_streams, edge_streams, golden_streams, layout_image,
                           mixed_streams)

pytestmark = pytest.mark.gpu

CANARY = 0xA5
BOTH = ("zlib", "blosc")
TYPES = {"int8": _lib.PIXELS_INT8, "uint8": _lib.PIXELS_UINT8, "int16": _lib.PIXELS_INT16,
         "uint16": _lib.PIXELS_UINT16, "int32": _lib.PIXELS_INT32, "uint32": _lib.PIXELS_UINT32,
         "float32": _lib.PIXELS_FLOAT, "float64": _lib.PIXELS_DOUBLE}


def decode_batch(ctx, streams, expected, mis=None):
    """Streams through K15a in one call: [(status, bytes)], after checking every slot's canary.
    Streams and slots are packed byte to byte, so they begin at every alignment; with `mis` every
    stream begins `mis` bytes behind a dword boundary."""
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
    _lib.check(_lib.lib.omr_lz4_decode_batch_device(ctx.h, src.data_ptr(), offs.data_ptr(), lens.data_ptr(),
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
        assert st == _lib.OK, (i, st)
        assert got == d, f"stream {i} ({len(d)} bytes) differs"
        assert omr.lz4_decode_host(s, len(d)) == d         # the host decoder agrees


GOOD = golden_streams() + crafted_streams()


@pytest.mark.parametrize("k", range(len(GOOD)), ids=[g[0] for g in GOOD])
def test_lz4_stream(ctx, k):
    name, data, stream = GOOD[k]
    check_equal(ctx, [data], [stream])


def test_lz4_all_good_streams_at_odd_alignments(ctx):
    datas, streams = [g[1] for g in GOOD], [g[2] for g in GOOD]
    check_equal(ctx, datas + datas[::-1], streams + streams[::-1])


@pytest.mark.parametrize("mis", [0, 1, 2, 3])
def test_lz4_edge_streams_at_each_source_alignment(ctx, mis):
    """Every edge stream `mis` bytes behind a dword boundary: the 256-byte window counts from the
    aligned dword below the stream, so its reloads fall on other bytes at each, and so do the
    source dwords of the literal copies."""
    check_equal(ctx, [e[1] for e in edge_streams()], [e[2] for e in edge_streams()], mis)


def test_lz4_300_mixed_streams(ctx):
    datas, streams = zip(*mixed_streams())
    check_equal(ctx, list(datas), list(streams))


def test_lz4_malformed_between_good(ctx):
    """Inputs the decoder must survive: the bad streams report OMR_INTERNAL, their neighbours
    decode, and nothing is written behind any slot."""
    rng = np.random.default_rng(180)
    good = [rng.integers(0, 9, 3000, dtype=np.uint8).tobytes() for _ in range(3)]
    gs = [omr.lz4_encode(g) for g in good]
    streams, expected, bad_at = [], [], []
    for k, (name, s, e) in enumerate(bad_streams()):
        streams.append(gs[k % 3])
        expected.append(3000)
        bad_at.append(len(streams))
        streams.append(s)
        expected.append(e)
    streams.append(gs[len(bad_streams()) % 3])
    expected.append(3000)
    res = decode_batch(ctx, streams, expected)
    for i in range(len(streams)):
        if i in bad_at:
            continue
        assert res[i] == (_lib.OK, good[(i // 2) % 3]), i
    for i, (name, s, e) in zip(bad_at, bad_streams()):
        assert res[i][0] == _lib.INTERNAL, (name, res[i][0])
        with pytest.raises(omr.OmrError) as err:
            omr.lz4_decode_host(s, e)
        assert err.value.status == _lib.INTERNAL, name


def test_lz4_arguments(ctx):
    assert _lib.lib.omr_lz4_decode_batch_device(ctx.h, None, None, None, None, 0, None, None, None) == _lib.OK
    assert _lib.lib.omr_lz4_decode_batch_device(ctx.h, None, None, None, None, 1, None, None, None) == _lib.INVALID_ARGUMENT
    assert _lib.lib.omr_lz4_decode_batch_device(ctx.h, None, None, None, None, -1, None, None, None) == _lib.INVALID_ARGUMENT


# ---- regions ------------------------------------------------------------------------------------

W, H = 200, 150
SHAPES = [(1, 1, [(0, 0), (199, 149), (64, 48)]),             # 1 x 1
          (37, 29, [(45, 33), (101, 77)]),                    # odd origin, across four chunks
          (50, 40, [(150, 110)]),                             # the bottom-right edge chunks
          (200, 7, [(0, 0), (0, 143), (0, 45)])]              # full width
ROWS = 3                                                      # sentinel rows behind each region


@pytest.mark.parametrize("shuffle", [0, 1])
@pytest.mark.parametrize("split", [None, False], ids=["split", "nosplit"])
@pytest.mark.parametrize("bo", ["<", ">"])
@pytest.mark.parametrize("name", list(TYPES))
def test_read_regions_equal_get_tile(ctx, tmp_path, name, bo, split, shuffle):
    import torch
    a = chunk_pixels(name, np.random.default_rng(zlib.crc32(repr((name, bo, split, shuffle)).encode())), (1, 2, 1, H, W))
    a[0, 1, 0, 96:144, 128:192] = 0                        # one chunk of zeros: left unwritten
    path = tmp_path / "r.zarr"
    omr.write_zarr(path, a, chunk=(64, 48), byteorder=bo, compressor="blosc", skip_zero_chunks=True,
                   blosc={"split": split, "shuffle": shuffle})
    assert not (path / "0" / "0/1/0/2/2").exists()
    with omr.ZarrImage(path, codecs=BOTH) as img:
        assert img.pixel_type == TYPES[name] and img.info["compression"] == 2
        bpp = a.dtype.itemsize
        for w, h, origins in SHAPES:
            reqs = [(0, c, 0, x, y) for c in (0, 1) for (x, y) in origins]
            stride = (w * (h + ROWS) * bpp + 15) // 16 * 16
            out = torch.full((len(reqs), stride), CANARY, dtype=torch.uint8, device="cuda")
            ctx.order_after_torch()
            got = img.read_regions(ctx, 0, reqs, w, h, out=out, region_stride=stride).cpu().numpy()
            for i, (z, c, t, x, y) in enumerate(reqs):
                ref = img.get_tile(0, z, c, t, x, y, w, h)
                assert ref.tobytes() == a[0, c, 0, y:y + h, x:x + w].astype(img.dtype).tobytes()
                assert got[i, :w * h * bpp].tobytes() == ref.tobytes(), (w, h, x, y, c)
                assert (got[i, w * h * bpp:] == CANARY).all(), "sentinel rows behind the region overwritten"
        # requests that share chunks, and the missing chunk
        reqs = [(0, 1, 0, x, y) for (x, y) in ((100, 60), (110, 70), (100, 60), (120, 90), (0, 0))]
        got = img.read_regions(ctx, 0, reqs, 80, 60).cpu().numpy()
        for i, (z, c, t, x, y) in enumerate(reqs):
            assert got[i, :80 * 60 * bpp].tobytes() == a[0, c, 0, y:y + 60, x:x + 80].astype(img.dtype).tobytes()


def test_read_regions_block_layouts(ctx, tmp_path):
    """Three blocks, a leftover block, unshuffled small blocks, memcpyed, a raw split and a missing
    chunk, in one image and one call; and the float64 chunk whose blocks are too small to split."""
    path = tmp_path / "l.zarr"
    a, files = layout_image(path)
    with omr.ZarrImage(path, codecs=BOTH) as img:
        for (x, y, w, h) in ((0, 0, 64, 48), (13, 7, 30, 29), (63, 47, 1, 1)):
            reqs = [(0, c, 0, x, y) for c in range(6)]
            got = img.read_regions(ctx, 0, reqs, w, h).cpu().numpy()
            for c in range(6):
                assert got[c, :w * h * 2].tobytes() == a[0, c, 0, y:y + h, x:x + w].astype("<u2").tobytes(), (c, x, y)
                assert got[c, :w * h * 2].tobytes() == img.get_tile(0, 0, c, 0, x, y, w, h).tobytes()
    f = chunk_pixels("float64", np.random.default_rng(181), (1, 1, 1, 48, 64))
    omr.write_zarr(tmp_path / "f.zarr", f, chunk=(64, 48), compressor="blosc", blosc={"blocksize": 512})
    with omr.ZarrImage(tmp_path / "f.zarr", codecs=BOTH) as img:
        got = img.read_regions(ctx, 0, [(0, 0, 0, 5, 3)], 50, 40).cpu().numpy()
        assert got[0, :50 * 40 * 8].tobytes() == f[0, 0, 0, 3:43, 5:55].tobytes()


def test_read_regions_typesize_other_than_the_sample(ctx, tmp_path):
    """The decoder follows the header's typesize: uint16 pixels in chunks written with typesize 4
    and 3 (a block tail that stays in place), shuffled."""
    a = chunk_pixels("uint16", np.random.default_rng(182), (1, 2, 1, 48, 64))
    for ts, bs in ((4, 0), (3, 2048), (1, 0)):
        path = tmp_path / f"t{ts}.zarr"
        omr.write_zarr(path, a, chunk=(64, 48), compressor="blosc", blosc={"typesize": ts, "blocksize": bs, "split": False})
        with omr.ZarrImage(path, codecs=BOTH) as img:
            got = img.read_regions(ctx, 0, [(0, 0, 0, 3, 5), (0, 1, 0, 3, 5)], 60, 40).cpu().numpy()
            for c in (0, 1):
                assert img.get_tile(0, 0, c, 0, 3, 5, 60, 40).tobytes() == a[0, c, 0, 5:45, 3:63].tobytes()
                assert got[c, :60 * 40 * 2].tobytes() == a[0, c, 0, 5:45, 3:63].tobytes(), (ts, c)


def test_read_regions_corrupt_chunk(ctx, tmp_path):
    a = chunk_pixels("uint16", np.random.default_rng(183), (1, 2, 1, H, W))
    path = tmp_path / "c.zarr"
    omr.write_zarr(path, a, chunk=(64, 48), compressor="blosc", dimension_separator=".")
    chunk = path / "0" / "0.0.0.1.1"
    good = chunk.read_bytes()
    at = int.from_bytes(good[16:20], "little")
    low = int.from_bytes(good[at:at + 4], "little")
    high_at = at + 4 + low + 4                             # the LZ4 stream of the high bytes
    csize = int.from_bytes(good[high_at - 4:high_at], "little")
    assert csize < 3072 and high_at + csize == len(good)
    bad_stream = good[:high_at] + b"\xff" * csize          # a literal length that never ends: the container is sound
    for what, data in (("stream", bytes(bad_stream)), ("container", good[:8] + b"\0\0\0\0" + good[12:])):
        chunk.write_bytes(data)
        with omr.ZarrImage(path, codecs=BOTH) as img:
            with pytest.raises(omr.OmrError) as e:
                img.get_tile(0, 0, 0, 0, 64, 48, 64, 48)
            assert e.value.status == _lib.INTERNAL, what
            with pytest.raises(omr.OmrError) as e:
                img.read_regions(ctx, 0, [(0, 0, 0, 0, 0), (0, 0, 0, 40, 30), (0, 1, 0, 0, 0)], 64, 48)
            assert e.value.status == _lib.INTERNAL, what
            assert "zarr: corrupt blosc chunk" in str(e.value), what
            got = img.read_regions(ctx, 0, [(0, 1, 0, 40, 30)], 64, 48)    # the context goes on working
            assert got.cpu().numpy()[0].tobytes() == a[0, 1, 0, 30:78, 40:104].astype("<u2").tobytes()


def test_read_regions_level_1(ctx, tmp_path):
    rng = np.random.default_rng(184)
    a, lv1 = chunk_pixels("uint16", rng, (1, 2, 1, H, W)), chunk_pixels("uint16", rng, (1, 2, 1, 75, 100))
    omr.write_zarr(tmp_path / "p.zarr", a, levels=[lv1], chunk=(64, 48), byteorder=">", compressor="blosc")
    with omr.ZarrImage(tmp_path / "p.zarr", codecs=BOTH) as img:
        reqs = [(0, 0, 0, 0, 0), (0, 1, 0, 40, 15), (0, 1, 0, 60, 35)]
        got = img.read_regions(ctx, 1, reqs, 40, 40).cpu().numpy()
        for i, (z, c, t, x, y) in enumerate(reqs):
            assert got[i, :40 * 40 * 2].tobytes() == lv1[0, c, 0, y:y + 40, x:x + 40].astype(">u2").tobytes()


# ---- render -------------------------------------------------------------------------------------

REQS = [(0, 0, 0, 0), (0, 0, 64, 64), (0, 0, 136, 86), (0, 0, 17, 33)]


@pytest.mark.parametrize("bo", ["<", ">"])
def test_render_tiles_equal_zlib_group(ctx, tmp_path, bo):
    from omr.synthetic import microscopy_u16
    rng = np.random.default_rng(185)
    lv0 = np.stack([microscopy_u16(H, W, rng, blobs=6) for _ in range(4)])[None, :, None]
    omr.write_zarr(tmp_path / "b.zarr", lv0, chunk=(64, 48), byteorder=bo, compressor="blosc")
    omr.write_zarr(tmp_path / "z.zarr", lv0, chunk=(64, 48), byteorder=bo, level=6)
    qdef, chans = make_qdef("rgb"), c2_channels(4)
    with omr.ZarrImage(tmp_path / "b.zarr", codecs=BOTH) as img, omr.ZarrImage(tmp_path / "z.zarr") as ref:
        for fh, fv in ((False, False), (True, True)):
            got = img.render_tiles(ctx, qdef, chans, 0, REQS, 64, 64, flip_h=fh, flip_v=fv)
            assert np.array_equal(got, ref.render_tiles(ctx, qdef, chans, 0, REQS, 64, 64, flip_h=fh, flip_v=fv)), (fh, fv)
        assert got.any()


def test_kernel_timing_kinds(ctx, tmp_path):
    a = chunk_pixels("uint16", np.random.default_rng(186), (1, 2, 1, H, W))
    omr.write_zarr(tmp_path / "b.zarr", a, chunk=(64, 48), compressor="blosc")
    omr.write_zarr(tmp_path / "m.zarr", a, chunk=(64, 48), compressor="blosc", blosc={"memcpy": True})
    omr.write_zarr(tmp_path / "z.zarr", a, chunk=(64, 48))
    ctx.enable_kernel_timing(True)
    try:
        ctx.kernel_timings()
        with omr.ZarrImage(tmp_path / "b.zarr", codecs=BOTH) as img:
            img.read_regions(ctx, 0, [(0, 0, 0, 10, 10)], 100, 100)
        assert sorted(k for _, k in ctx.kernel_timings()) == [33, 34]
        with omr.ZarrImage(tmp_path / "m.zarr", codecs=BOTH) as img:
            img.read_regions(ctx, 0, [(0, 0, 0, 10, 10)], 100, 100)
        assert [k for _, k in ctx.kernel_timings()] == [34]      # memcpyed chunks skip K15a
        with omr.ZarrImage(tmp_path / "z.zarr", codecs=BOTH) as img:
            img.read_regions(ctx, 0, [(0, 0, 0, 10, 10)], 100, 100)
        assert sorted(k for _, k in ctx.kernel_timings()) == [31, 32]
    finally:
        ctx.enable_kernel_timing(False)
