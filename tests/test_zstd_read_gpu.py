"""Zstandard OME-Zarr chunks on the GPU (K16): omr_zstd_decode_batch_device (K16a) on its own against
frames of libzstd (tests/golden/zstd_frames.npz), crafted, edge and malformed ones and the host
decoder, then ZarrImage.read_regions on Blosc-Zstd and zstd groups against the host route
(ZarrImage.get_tile) and numpy, then ZarrImage.render_tiles against the same pixels in a zlib group.
No tolerance anywhere: decoded bytes and ARGB words are compared for equality.  Every output slot of
the bare decoder is followed by sixteen canary bytes that must come back unchanged."""
import numpy as np
import pytest

import omr
from omr import _lib
from omr.context import make_qdef
from omr.synthetic import c2_channels
from blosc_streams import chunk_pixels
import zstd_streams as zs

pytestmark = pytest.mark.gpu

CANARY = 0xA5
ALL = ("zlib", "blosc", "blosc-zstd", "zstd")
TYPES = {"uint8": _lib.PIXELS_UINT8, "uint16": _lib.PIXELS_UINT16, "float32": _lib.PIXELS_FLOAT}


def decode_batch(ctx, frames, expected, mis=None, odd=False):
    """Frames through K16a in one call: [(status, bytes)], after checking every slot's canary.
    Frames and slots are packed byte to byte, so they begin at every alignment; with `mis` every
    frame begins `mis` bytes behind a dword boundary, with `odd` every slot at an odd offset."""
    import torch
    n = len(frames)
    src_off, pos, gaps = [], 0, []
    for s in frames:
        gaps.append(b"" if mis is None else b"\xEE" * ((mis - pos) % 4))
        pos += len(gaps[-1])
        src_off.append(pos)
        pos += len(s)
    dst_off, dpos = [], 0
    for e in expected:
        dpos += 1 if odd and dpos % 2 == 0 else 0
        dst_off.append(dpos)
        dpos += e + 16
    src = torch.from_numpy(np.frombuffer(b"".join(g + s for g, s in zip(gaps, frames)) + b"\0", dtype=np.uint8).copy()).cuda()
    assert src.data_ptr() % 4 == 0
    dst = torch.full((dpos,), CANARY, dtype=torch.uint8, device="cuda")
    offs = torch.tensor(src_off, dtype=torch.int64, device="cuda")
    lens = torch.tensor([len(s) for s in frames], dtype=torch.int32, device="cuda")
    exps = torch.tensor(expected, dtype=torch.int32, device="cuda")
    doff = torch.tensor(dst_off, dtype=torch.int64, device="cuda")
    stat = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    ctx.order_after_torch()
    _lib.check(_lib.lib.omr_zstd_decode_batch_device(ctx.h, src.data_ptr(), offs.data_ptr(), lens.data_ptr(),
                                                     exps.data_ptr(), n, dst.data_ptr(), doff.data_ptr(),
                                                     stat.data_ptr()), ctx.h)
    ctx.synchronize()
    out, st = dst.cpu().numpy(), stat.cpu().numpy()
    res = []
    for i in range(n):
        o, e = dst_off[i], expected[i]
        assert (out[o + e:o + e + 16] == CANARY).all(), f"canary behind frame {i} overwritten"
        res.append((int(st[i]), out[o:o + e].tobytes()))
    return res


def check_equal(ctx, datas, frames, mis=None, odd=False):
    res = decode_batch(ctx, frames, [len(d) for d in datas], mis, odd)
    for i, ((st, got), d) in enumerate(zip(res, datas)):
        assert st == _lib.OK, (i, st)
        assert got == d, f"frame {i} ({len(d)} bytes) differs"


GOOD = zs.all_good()
EDGE = zs.edge_frames()


@pytest.mark.parametrize("k", range(len(GOOD)), ids=[g[0] for g in GOOD])
def test_zstd_frame(ctx, k):
    name, data, frame = GOOD[k]
    assert omr.zstd_decode_host(frame, len(data)) == data
    check_equal(ctx, [data], [frame])


@pytest.mark.parametrize("mis", [0, 1, 2, 3])
def test_zstd_all_good_frames_at_each_source_alignment(ctx, mis):
    check_equal(ctx, [g[1] for g in GOOD], [g[2] for g in GOOD], mis, odd=True)


@pytest.mark.parametrize("k", range(len(EDGE)), ids=[e[0] for e in EDGE])
def test_zstd_edge_frame(ctx, k):
    name, data, frame = EDGE[k]
    assert omr.zstd_decode_host(frame, len(data)) == data
    check_equal(ctx, [data], [frame])


def test_zstd_edge_frames_in_one_launch(ctx):
    check_equal(ctx, [e[1] for e in EDGE] + [e[1] for e in EDGE[::-1]], [e[2] for e in EDGE] + [e[2] for e in EDGE[::-1]])


def test_zstd_300_mixed_frames(ctx):
    """300 frames of many sizes in one launch: more than one frame per workgroup is not needed to
    pass, but the grid stride, the reuse of the tables and of the literal buffer are run through
    with frames of every kind next to one another."""
    pool = [(d, f) for _, d, f in GOOD + EDGE if len(d) <= 50000]
    inputs = zs.inputs()
    for k in range(40):
        d = inputs["runs"][137 * k:137 * k + 50 + 211 * k]
        pool.append((d, omr.zstd_encode(d, checksum=bool(k & 1), single_segment=not k & 2)))
    picks = zs.rnd(300, 50).tolist()
    datas, frames = zip(*[pool[p % len(pool)] for p in picks])
    check_equal(ctx, list(datas), list(frames))


def test_zstd_malformed_between_good(ctx):
    """Inputs the decoder must survive (the set the host decoder refuses under the sanitizers in
    zstd-read-check, and every truncation of two small frames): each status equals the host's, the
    neighbours decode, and nothing is written behind any slot."""
    good = [zs.rbytes(3000, 60 + k, 9) for k in range(3)]
    gs = [omr.zstd_encode(g) for g in good]
    bad = list(zs.bad_frames())
    for name, data, frame in GOOD:
        if name in ("records@st19", "five_uniform@l19", "rle_literals_sequences"):
            bad += [(f"{name}[:{cut}]", frame[:cut], len(data)) for cut in zs.truncations(frame)]
            bad += [(f"{name} damaged {k}", f, len(data)) for k, f in enumerate(zs.damaged(frame, 40, 70))]
    frames, expected, bad_at = [], [], []
    for k, (name, s, e) in enumerate(bad):
        frames.append(gs[k % 3])
        expected.append(3000)
        bad_at.append(len(frames))
        frames.append(s)
        expected.append(e)
    frames.append(gs[len(bad) % 3])
    expected.append(3000)
    res = decode_batch(ctx, frames, expected)
    for i in range(len(frames)):
        if i not in bad_at:
            assert res[i] == (_lib.OK, good[(i // 2) % 3]), i
    for i, (name, s, e) in zip(bad_at, bad):
        try:
            want = (_lib.OK, omr.zstd_decode_host(s, e))
        except omr.OmrError as err:
            want = (err.status, None)
        assert res[i][0] == want[0], (name, res[i][0], want[0])
        if want[0] == _lib.OK:
            assert res[i][1] == want[1], name


def test_zstd_arguments(ctx):
    f = _lib.lib.omr_zstd_decode_batch_device
    assert f(ctx.h, None, None, None, None, 0, None, None, None) == _lib.OK
    assert f(ctx.h, None, None, None, None, 1, None, None, None) == _lib.INVALID_ARGUMENT
    assert f(ctx.h, None, None, None, None, -1, None, None, None) == _lib.INVALID_ARGUMENT
    assert f(None, None, None, None, None, 0, None, None, None) == _lib.INVALID_ARGUMENT


# ---- regions ------------------------------------------------------------------------------------

W, H = 200, 150
SHAPES = [(1, 1, [(0, 0), (199, 149), (64, 48)]), (37, 29, [(45, 33), (101, 77)]), (50, 40, [(150, 110)]),
          (200, 7, [(0, 0), (0, 143), (0, 45)])]
ROWS = 3
GROUPS = [("blosc-zstd", {"shuffle": 1, "split": None}), ("blosc-zstd", {"shuffle": 0, "split": None}),
          ("blosc-zstd", {"shuffle": 1, "split": False}), ("blosc-zstd", {"shuffle": 0, "split": False}),
          ("blosc-zstd", {"shuffle": 1, "typesize": 3, "blocksize": 2048, "split": False}), ("zstd", {})]


def write_group(path, a, kind, opts, **kw):
    if kind == "zstd":
        omr.write_zarr(path, a, chunk=(64, 48), compressor="zstd", **kw)
    else:
        omr.write_zarr(path, a, chunk=(64, 48), compressor="blosc", blosc=dict(opts, cname="zstd"), **kw)


@pytest.mark.parametrize("kind,opts", GROUPS, ids=[f"{g[0]}-{k}" for k, g in enumerate(GROUPS)])
@pytest.mark.parametrize("bo", ["<", ">"])
@pytest.mark.parametrize("name", list(TYPES))
def test_read_regions_equal_get_tile(ctx, tmp_path, name, bo, kind, opts):
    import torch
    a = chunk_pixels(name, np.random.default_rng(300 + len(name) + 7 * (bo == ">") + len(repr(opts))), (1, 2, 1, H, W))
    a[0, 1, 0, 96:144, 128:192] = 0                        # one chunk of zeros: left unwritten
    path = tmp_path / "r.zarr"
    write_group(path, a, kind, opts, byteorder=bo, skip_zero_chunks=True)
    assert not (path / "0" / "0/1/0/2/2").exists()
    with omr.ZarrImage(path, codecs=ALL) as img:
        assert img.pixel_type == TYPES[name] and img.info["compression"] == (3 if kind == "zstd" else 2)
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
        reqs = [(0, 1, 0, x, y) for (x, y) in ((100, 60), (110, 70), (100, 60), (120, 90), (0, 0))]
        got = img.read_regions(ctx, 0, reqs, 80, 60).cpu().numpy()
        for i, (z, c, t, x, y) in enumerate(reqs):
            assert got[i, :80 * 60 * bpp].tobytes() == a[0, c, 0, y:y + 60, x:x + 80].astype(img.dtype).tobytes()


def test_read_regions_level_1(ctx, tmp_path):
    rng = np.random.default_rng(310)
    a, lv1 = chunk_pixels("uint16", rng, (1, 2, 1, H, W)), chunk_pixels("uint16", rng, (1, 2, 1, 75, 100))
    for kind in ("blosc-zstd", "zstd"):
        write_group(tmp_path / kind, a, kind, {}, levels=[lv1], byteorder=">")
        with omr.ZarrImage(tmp_path / kind, codecs=(kind,)) as img:
            reqs = [(0, 0, 0, 0, 0), (0, 1, 0, 40, 15), (0, 1, 0, 60, 35)]
            got = img.read_regions(ctx, 1, reqs, 40, 40).cpu().numpy()
            for i, (z, c, t, x, y) in enumerate(reqs):
                assert got[i, :40 * 40 * 2].tobytes() == lv1[0, c, 0, y:y + 40, x:x + 40].astype(">u2").tobytes()
                assert got[i, :40 * 40 * 2].tobytes() == img.get_tile(1, z, c, t, x, y, 40, 40).tobytes()


def test_read_regions_golden_libzstd_chunks(ctx, tmp_path):
    """A group whose chunks are assembled from the fixture's libzstd level-5 frames."""
    a = zs.chunk_image()[None, None, None]
    omr.write_zarr(tmp_path / "g", a, chunk=(64, 48), compressor="blosc", blosc={"cname": "zstd", "codec": zs.golden_codec})
    with omr.ZarrImage(tmp_path / "g", codecs=("blosc-zstd",)) as img:
        got = img.read_regions(ctx, 0, [(0, 0, 0, 0, 0), (0, 0, 0, 30, 20)], 98, 76).cpu().numpy()
        for i, (x, y) in enumerate(((0, 0), (30, 20))):
            assert got[i, :98 * 76 * 2].tobytes() == a[0, 0, 0, y:y + 76, x:x + 98].tobytes()
            assert img.get_tile(0, 0, 0, 0, x, y, 98, 76).tobytes() == a[0, 0, 0, y:y + 76, x:x + 98].tobytes()


def test_read_regions_lz4_and_zstd_chunks_in_one_group(ctx, tmp_path):
    a = chunk_pixels("uint16", np.random.default_rng(311), (1, 1, 1, 96, 128))
    path = tmp_path / "m"
    omr.write_zarr(path, a, chunk=(64, 48), compressor="blosc", dimension_separator=".")
    for cy, cx in ((0, 1), (1, 0)):
        (path / "0" / f"0.0.0.{cy}.{cx}").write_bytes(
            omr.blosc_encode(a[0, 0, 0, cy * 48:(cy + 1) * 48, cx * 64:(cx + 1) * 64].tobytes(), 2, codec="zstd"))
    with omr.ZarrImage(path, codecs=("blosc", "blosc-zstd")) as img:
        ctx.enable_kernel_timing(True)
        try:
            ctx.kernel_timings()
            got = img.read_regions(ctx, 0, [(0, 0, 0, 0, 0)], 128, 96).cpu().numpy()
            assert sorted(k for _, k in ctx.kernel_timings()) == [33, 34, 35]
        finally:
            ctx.enable_kernel_timing(False)
        assert got[0, :128 * 96 * 2].tobytes() == a[0, 0, 0].tobytes()
    with omr.ZarrImage(path, codecs=("blosc",)) as img:       # the Zstd chunks are outside the open set
        with pytest.raises(omr.OmrError) as e:
            img.read_regions(ctx, 0, [(0, 0, 0, 0, 0)], 128, 96)
        assert e.value.status == _lib.INTERNAL and "zarr: corrupt blosc chunk" in str(e.value)
        got = img.read_regions(ctx, 0, [(0, 0, 0, 0, 0)], 64, 48).cpu().numpy()
        assert got[0, :64 * 48 * 2].tobytes() == a[0, 0, 0, :48, :64].tobytes()


def test_read_regions_corrupt_chunk(ctx, tmp_path):
    a = zs.chunk_image()[None, None, None]
    a = np.concatenate([a, a[:, :, :, ::-1]], axis=1)
    for kind, message in (("blosc-zstd", "zarr: corrupt blosc chunk"), ("zstd", "zarr: corrupt zstd chunk")):
        path = tmp_path / kind
        write_group(path, a, kind, {}, dimension_separator=".")
        chunk = path / "0" / "0.0.0.1.1"
        good = chunk.read_bytes()
        at = good.index(b"\x28\xb5\x2f\xfd")               # the container stays sound: a frame's block header changes
        bad = good[:at + 7] + bytes([good[at + 7] ^ 0x06]) + good[at + 8:]
        chunk.write_bytes(bad)
        with omr.ZarrImage(path, codecs=ALL) as img:
            with pytest.raises(omr.OmrError) as e:
                img.get_tile(0, 0, 0, 0, 64, 48, 64, 48)
            assert e.value.status == _lib.INTERNAL, kind
            with pytest.raises(omr.OmrError) as e:
                img.read_regions(ctx, 0, [(0, 0, 0, 0, 0), (0, 0, 0, 40, 30), (0, 1, 0, 0, 0)], 64, 48)
            assert e.value.status == _lib.INTERNAL, kind
            assert message in str(e.value), kind
            got = img.read_regions(ctx, 0, [(0, 1, 0, 40, 30)], 64, 48)    # the context goes on working
            assert got.cpu().numpy()[0].tobytes() == a[0, 1, 0, 30:78, 40:104].tobytes()


# ---- render -------------------------------------------------------------------------------------

REQS = [(0, 0, 0, 0), (0, 0, 64, 64), (0, 0, 136, 86), (0, 0, 17, 33)]


@pytest.mark.parametrize("kind", ["blosc-zstd", "zstd"])
def test_render_tiles_equal_zlib_group(ctx, tmp_path, kind):
    from omr.synthetic import microscopy_u16
    rng = np.random.default_rng(312)
    lv0 = np.stack([microscopy_u16(H, W, rng, blobs=6) for _ in range(4)])[None, :, None]
    write_group(tmp_path / "b.zarr", lv0, kind, {}, byteorder=">")
    omr.write_zarr(tmp_path / "z.zarr", lv0, chunk=(64, 48), byteorder=">", level=6)
    qdef, chans = make_qdef("rgb"), c2_channels(4)
    with omr.ZarrImage(tmp_path / "b.zarr", codecs=ALL) as img, omr.ZarrImage(tmp_path / "z.zarr") as ref:
        for fh, fv in ((False, False), (True, True)):
            got = img.render_tiles(ctx, qdef, chans, 0, REQS, 64, 64, flip_h=fh, flip_v=fv)
            assert np.array_equal(got, ref.render_tiles(ctx, qdef, chans, 0, REQS, 64, 64, flip_h=fh, flip_v=fv)), (fh, fv)
        assert got.any()


def test_kernel_timing_kinds(ctx, tmp_path):
    a = zs.chunk_image()[None, None, None]
    write_group(tmp_path / "b.zarr", a, "blosc-zstd", {})
    write_group(tmp_path / "s.zarr", a, "zstd", {})
    ctx.enable_kernel_timing(True)
    try:
        ctx.kernel_timings()
        with omr.ZarrImage(tmp_path / "b.zarr", codecs=ALL) as img:
            img.read_regions(ctx, 0, [(0, 0, 0, 10, 10)], 100, 80)
        assert sorted(k for _, k in ctx.kernel_timings()) == [34, 35]
        with omr.ZarrImage(tmp_path / "s.zarr", codecs=ALL) as img:
            img.read_regions(ctx, 0, [(0, 0, 0, 10, 10)], 100, 80)
        assert sorted(k for _, k in ctx.kernel_timings()) == [31, 35]
    finally:
        ctx.enable_kernel_timing(False)
