"""Raw pixel tiles as 8/16-bit greyscale PNG on the GPU (K12): omr_encode_png_gray_batch_device and
PixelBuffer.tiles_png.

Every file is checked four ways with PIL's and zlib's decoders plus numpy, no tolerance: each
chunk's CRC (zlib.crc32), the IHDR fields, the IDAT stream inflated by zlib (which checks the
Adler-32) into h rows of 1 + w * bps bytes with filter bytes 0..4, and PIL's decoded pixels against
the region (bit patterns for the signed types).  Every batch also runs in a context created with
OMR_PNG_GRAY_WAVE=0 (the workgroup filter): both routes must give the same bytes, and the kernel
timing kinds tell which route ran."""
import io
import os
import struct
import zlib

import numpy as np
import pytest

import omr
from omr import PixelBuffer, _lib, write_romio
from omr.synthetic import microscopy_u16

pytestmark = pytest.mark.gpu

U8, U16, I8, I16 = _lib.PIXELS_UINT8, _lib.PIXELS_UINT16, _lib.PIXELS_INT8, _lib.PIXELS_INT16
NP = {U8: "u1", U16: "u2", I8: "i1", I16: "i2"}
KIND_FILTER, KIND_GRAY_WAVE = 20, 27


@pytest.fixture(scope="module")
def ref_ctx():
    """A context that filters every grey batch with the workgroup kernel."""
    import torch  # noqa: F401
    old = os.environ.get("OMR_PNG_GRAY_WAVE")
    os.environ["OMR_PNG_GRAY_WAVE"] = "0"
    try:
        c = omr.Context(0)
    finally:
        if old is None:
            del os.environ["OMR_PNG_GRAY_WAVE"]
        else:
            os.environ["OMR_PNG_GRAY_WAVE"] = old
    yield c
    c.close()


def chunks(png):
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    i, out = 8, []
    while i < len(png):
        ln, = struct.unpack(">I", png[i:i + 4])
        typ, data = png[i + 4:i + 8], png[i + 8:i + 8 + ln]
        crc, = struct.unpack(">I", png[i + 8 + ln:i + 12 + ln])
        assert zlib.crc32(png[i + 4:i + 8 + ln]) == crc, typ
        out.append((typ, data))
        i += 12 + ln
    assert i == len(png)
    return out


def check_file(png, region, pt):
    """png holds the native-order [h][w] array `region` of pixel type pt."""
    h, w = region.shape
    bps = int(NP[pt][1])
    ch = chunks(png)
    assert [t for t, _ in ch if t != b"IDAT"] == [b"IHDR", b"IEND"]          # no PLTE / tRNS
    assert ch[0][0] == b"IHDR" and ch[-1] == (b"IEND", b"")
    assert struct.unpack(">IIBBBBB", ch[0][1]) == (w, h, 8 * bps, 0, 0, 0, 0)
    raw = zlib.decompress(b"".join(d for t, d in ch if t == b"IDAT"))
    rowlen = 1 + w * bps
    assert len(raw) == h * rowlen
    assert set(raw[::rowlen]) <= {0, 1, 2, 3, 4}
    from PIL import Image
    got = np.asarray(Image.open(io.BytesIO(png)))
    want = region.view("u" + NP[pt][1])                                       # the bit patterns
    assert got.shape == want.shape and np.array_equal(got.astype(want.dtype), want)


def stored_idat(png):
    z = b"".join(d for t, d in chunks(png) if t == b"IDAT")
    return (z[2] >> 1) & 3 == 0


def to_device(plane, big_endian):
    """A native-order 2-D array as device bytes in the asked byte order."""
    import torch
    a = plane.astype((">" if big_endian else "<") + plane.dtype.str[1:])
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda")


def run(c, tiles, pt, w, h, big_endian=True, cap=None):
    """tiles: [(device bytes, pitch_px, x, y)] -> ([(status, offset, file bytes)], [timing kinds])."""
    import torch
    n = len(tiles)
    if cap is None:
        cap = _lib.lib.omr_png_gray_batch_max_bytes(w, h, int(NP[pt][1]), n)
    out = torch.zeros(max(cap, 1), dtype=torch.uint8, device="cuda")
    offs = torch.full((max(n, 1),), -1, dtype=torch.int64, device="cuda")
    lens = torch.full((max(n, 1),), -1, dtype=torch.int32, device="cuda")
    stat = torch.full((max(n, 1),), -1, dtype=torch.int32, device="cuda")
    c.enable_kernel_timing(True)
    c.kernel_timings()
    try:
        c.encode_png_gray_batch_device(tiles, pt, w, h, out[:cap], offs, lens, stat, big_endian=big_endian)
        kinds = [k for _, k in c.kernel_timings()]
    finally:
        c.enable_kernel_timing(False)
    torch.cuda.synchronize()
    o, l, s, b = offs.cpu().numpy(), lens.cpu().numpy(), stat.cpu().numpy(), out.cpu().numpy()
    return [(int(s[i]), int(o[i]), b[int(o[i]):int(o[i]) + int(l[i])].tobytes()) for i in range(n)], kinds


def both(ctx, ref_ctx, planes, spec, pt, w, h, big_endian=True, wave=None):
    """Encode spec = [(plane index, x, y)] of the native-order `planes` on both routes; check every
    file, the routes' bytes against each other and (wave = True / False) the route taken."""
    dev = [to_device(p, big_endian) for p in planes]
    tiles = [(dev[k], planes[k].shape[1], x, y) for k, x, y in spec]
    res, kinds = run(ctx, tiles, pt, w, h, big_endian)
    ref, rkinds = run(ref_ctx, tiles, pt, w, h, big_endian)
    assert KIND_GRAY_WAVE not in rkinds and KIND_FILTER in rkinds
    if wave is not None:
        assert (KIND_GRAY_WAVE in kinds) == wave and (KIND_FILTER in kinds) == (not wave), kinds
    files = []
    for (st, off, png), (rst, _, rpng), (k, x, y) in zip(res, ref, spec):
        assert st == 0 and rst == 0 and off % 16 == 0
        check_file(png, planes[k][y:y + h, x:x + w], pt)
        assert png == rpng, "the wave and the workgroup filter disagree"
        files.append(png)
    return files


def noise(pt, h, w, seed):
    rng = np.random.default_rng(seed)
    info = np.iinfo(np.dtype(NP[pt]))
    return rng.integers(info.min, int(info.max) + 1, (h, w)).astype(NP[pt])


def image_like(pt, h, w, seed):
    """Smooth structure plus a little noise: every filter gets its rows."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    a = (xx * 37 + yy * 11 + (xx * yy) // 7) + rng.integers(0, 4, (h, w))
    a[h // 3:h // 2 + 1, w // 4:w // 2 + 1] = 12345
    return a.astype(np.int64).astype("u" + NP[pt][1]).view(NP[pt])


def wave_expected(pt, w, x, pitch):
    bps = int(NP[pt][1])
    return (w * bps) % 4 == 0 and w * bps <= 4096 and (x * bps) % 16 == 0 and (pitch * bps) % 16 == 0


# ---- sizes and ragged rows ----------------------------------------------------------------------
SIZES = [(1, 1), (1, 7), (3, 5), (17, 9), (255, 4), (257, 3), (1024, 16), (1032, 9), (2048, 9), (2056, 5), (4096, 3)]


@pytest.mark.parametrize("pt", [U8, U16])
@pytest.mark.parametrize("w,h", SIZES)
def test_sizes(ctx, ref_ctx, pt, w, h):
    planes = [image_like(pt, h, w, w + h), noise(pt, h, w, w)]
    both(ctx, ref_ctx, planes, [(0, 0, 0), (1, 0, 0)], pt, w, h, wave=wave_expected(pt, w, 0, w))


@pytest.mark.parametrize("pt", [I8, I16])
@pytest.mark.parametrize("w,h", [(1, 1), (17, 9), (257, 3), (1024, 16), (1032, 9)])
def test_sizes_signed(ctx, ref_ctx, pt, w, h):
    planes = [image_like(pt, h, w, 3 * w + h), noise(pt, h, w, w + 1)]
    assert w * h < 64 or planes[1].min() < 0
    files = both(ctx, ref_ctx, planes, [(0, 0, 0), (1, 0, 0)], pt, w, h, wave=wave_expected(pt, w, 0, w))
    # the file of a signed plane is the file of the unsigned plane with the same bits
    upt = U8 if pt == I8 else U16
    assert files == both(ctx, ref_ctx, [p.view(NP[upt]) for p in planes], [(0, 0, 0), (1, 0, 0)], upt, w, h)


def test_widest_wave_and_first_workgroup_width(ctx, ref_ctx):
    """uint16: 2048 pixels are 4096 row bytes, the widest wave form (M = 4); 2056 and 4096 pixels
    take the workgroup form; uint8 4096 is the widest wave form again."""
    both(ctx, ref_ctx, [image_like(U16, 9, 2048, 1)], [(0, 0, 0)], U16, 2048, 9, wave=True)
    both(ctx, ref_ctx, [image_like(U16, 5, 2056, 2)], [(0, 0, 0)], U16, 2056, 5, wave=False)
    both(ctx, ref_ctx, [image_like(U16, 3, 4096, 3)], [(0, 0, 0)], U16, 4096, 3, wave=False)
    both(ctx, ref_ctx, [image_like(U8, 3, 4096, 4)], [(0, 0, 0)], U8, 4096, 3, wave=True)


# ---- region placement ---------------------------------------------------------------------------
@pytest.mark.parametrize("pt", [U8, U16])
@pytest.mark.parametrize("h", [9, 8, 1])
def test_region_placement(ctx, ref_ctx, pt, h):
    """Nine rows cross a band boundary of the wave form (8 rows), 8 and 1 do not."""
    bps = int(NP[pt][1])
    w, ph = 64, 24
    x4 = 4 // bps                                        # x * bps == 4: a dword, not 16 bytes
    x16 = 16 // bps                                      # x * bps == 16
    aligned = image_like(pt, ph, 160, 7)                 # pitch * bps a multiple of 16
    ragged = image_like(pt, ph, 150 + 1, 8)              # 151 pixels: a pitch off 16 (and off 4) bytes
    dword = image_like(pt, ph, 150 if bps == 2 else 148, 9)   # pitch * bps a multiple of 4, not of 16
    tight = image_like(pt, ph, w, 10)                    # pitch == w
    for planes, x, wave in ((aligned, 3, False),         # x odd
                            (aligned, x4, False),        # x * bps at 4 but not 16
                            (aligned, x16, True),        # aligned x, aligned pitch
                            (aligned, 160 - w, True),    # the last columns
                            (ragged, x16, False),        # x * bps a multiple of 16, the pitch is not
                            (ragged, 3, False),
                            (dword, x4, False),          # dword rows, not 16 bytes
                            (tight, 0, True)):           # pitch == w
        assert wave == wave_expected(pt, w, x, planes.shape[1])
        for y in (0, 5, ph - h):                         # the first and the last rows of the plane
            both(ctx, ref_ctx, [planes], [(0, x, y)], pt, w, h, wave=wave)


# ---- byte order ---------------------------------------------------------------------------------
@pytest.mark.parametrize("pt,w,h,x", [(U16, 1024, 16, 0), (U16, 264, 9, 8), (U16, 37, 9, 3), (I16, 66, 5, 1),
                                      (U8, 64, 9, 16)])
def test_byte_order(ctx, ref_ctx, pt, w, h, x):
    plane = image_like(pt, h + 2, x + w + (8 if x else 0), 21)
    be = both(ctx, ref_ctx, [plane], [(0, x, 1)], pt, w, h, big_endian=True)
    le = both(ctx, ref_ctx, [plane], [(0, x, 1)], pt, w, h, big_endian=False)
    assert be == le


# ---- content ------------------------------------------------------------------------------------
def content_planes(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    rng = np.random.default_rng(33)
    two = rng.integers(0, 65536, (2, w))
    return {"zeros": np.zeros((h, w), np.uint16),
            "constant": np.full((h, w), 0xABCD, np.uint16),
            "hramp": (xx * 61).astype(np.uint16),
            "vramp": (yy * 523 + 7).astype(np.uint16),
            "rows2": two[yy[:, 0] % 2].astype(np.uint16),            # a row repeated every 2 rows
            "microscopy": microscopy_u16(h, w, np.random.default_rng(34)),
            "noise": noise(U16, h, w, 35)}


@pytest.mark.parametrize("w,h", [(256, 64), (250, 37)])           # the wave form / the workgroup form
def test_content(ctx, ref_ctx, w, h):
    planes = content_planes(h, w)
    names = list(planes)
    files = both(ctx, ref_ctx, [planes[k] for k in names], [(i, 0, 0) for i in range(len(names))], U16, w, h,
                 wave=(w == 256))
    size = dict(zip(names, map(len, files)))
    raw = w * h * 2
    assert size["noise"] <= _lib.lib.omr_png_gray_batch_max_bytes(w, h, 2, 1)
    assert stored_idat(files[names.index("noise")])
    for k in ("microscopy", "hramp", "vramp"):
        assert size[k] < raw, (k, size[k], raw)                   # not the stored path
        assert not stored_idat(files[names.index(k)])
    # zeros, and a constant or a ramp once filtered, are runs: a match of up to 32 bytes is two
    # codes of at most 15 bits, under an eighth of the bytes it covers; a sixth leaves room for
    # the rows' first samples and the block header
    for k in ("zeros", "constant", "hramp", "vramp"):
        assert size[k] < raw // 6, (k, size[k])
    # 8-bit: the same pictures' high bytes
    p8 = [(planes[k] >> 8).astype(np.uint8) for k in names]
    f8 = both(ctx, ref_ctx, p8, [(i, 0, 0) for i in range(len(names))], U8, w, h, wave=(w == 256))
    assert len(f8[names.index("microscopy")]) < w * h


# ---- batches ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 37])
def test_batches_mixed(ctx, ref_ctx, n):
    w, h = 72, 19
    planes = [image_like(U16, 40, 200, 50), noise(U16, 40, 200, 51), np.zeros((40, 200), np.uint16),
              microscopy_u16(40, 200, np.random.default_rng(52))]
    rng = np.random.default_rng(n)
    spec = [(int(rng.integers(0, 4)), int(rng.integers(0, 200 - w + 1)), int(rng.integers(0, 40 - h + 1)))
            for _ in range(n)]
    spec[0] = (spec[0][0], min(spec[0][1] | 1, 127), spec[0][2])  # one odd x: the whole batch off the wave form
    files = both(ctx, ref_ctx, planes, spec, U16, w, h, wave=False)
    # aligned offsets in every plane: the wave form over different planes and offsets in one call
    spec16 = [(k, x // 8 * 8, y) for k, x, y in spec]
    files16 = both(ctx, ref_ctx, planes, spec16, U16, w, h, wave=True)
    assert len(files) == len(files16) == n


def test_same_tile_twice_and_determinism(ctx, ref_ctx):
    plane = microscopy_u16(64, 256, np.random.default_rng(60))
    a = both(ctx, ref_ctx, [plane], [(0, 16, 3), (0, 16, 3), (0, 17, 3), (0, 17, 3)], U16, 128, 40)
    assert a[0] == a[1] and a[2] == a[3] and a[0] != a[2]
    b = both(ctx, ref_ctx, [plane], [(0, 16, 3), (0, 16, 3), (0, 17, 3), (0, 17, 3)], U16, 128, 40)
    assert a == b                                                 # two calls, identical bytes


def test_empty_batch(ctx):
    res, kinds = run(ctx, [], U16, 64, 64)
    assert res == [] and kinds == []
    assert _lib.lib.omr_encode_png_gray_batch_device(ctx.h, None, 0, U16, 1, 64, 64, None, 0, None, None,
                                                     None) == _lib.OK


@pytest.mark.parametrize("w", [64, 61])                           # the wave form / the workgroup form
def test_output_too_small(ctx, ref_ctx, w):
    h = 24
    planes = [image_like(U16, h, w, 70 + i) for i in range(4)]
    dev = [to_device(p, True) for p in planes]
    tiles = [(d, w, 0, 0) for d in dev]
    full, _ = run(ctx, tiles, U16, w, h)
    for k in (1, 3):
        cap = full[k][1]                                          # room for exactly the first k slots
        res, _ = run(ctx, tiles, U16, w, h, cap=cap)
        assert [r[0] for r in res] == [0] * k + [_lib.BUFFER_TOO_SMALL] * (4 - k)
        assert [r[2] for r in res] == [f[2] for f in full[:k]] + [b""] * (4 - k)
        rres, _ = run(ref_ctx, tiles, U16, w, h, cap=cap)
        assert rres == res


# ---- errors -------------------------------------------------------------------------------------
def test_errors_launch_nothing(ctx):
    import torch
    d = torch.zeros(4097 * 8 * 4, dtype=torch.uint8, device="cuda")
    out = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")

    def call(tiles, pt, w, h, n=None, launches=False):
        tab = (_lib.RawTile * max(len(tiles), 1))()
        for i, (p, pitch, x, y) in enumerate(tiles):
            tab[i].d_plane, tab[i].pitch_px, tab[i].x, tab[i].y = p, pitch, x, y
        import ctypes
        ctx.enable_kernel_timing(True)
        ctx.kernel_timings()
        try:
            st = _lib.lib.omr_encode_png_gray_batch_device(ctx.h, ctypes.addressof(tab), len(tiles) if n is None else n,
                                                           pt, 1, w, h, out.data_ptr(), out.numel(), None, None, None)
            kinds = ctx.kernel_timings()
        finally:
            ctx.enable_kernel_timing(False)
        assert (kinds != []) == launches                          # an error launches nothing
        return st

    p = d.data_ptr()
    INV = _lib.INVALID_ARGUMENT
    for pt in (_lib.PIXELS_FLOAT, _lib.PIXELS_INT32, _lib.PIXELS_UINT32, _lib.PIXELS_DOUBLE, -1, 8):
        assert call([(p, 16, 0, 0)], pt, 16, 4) == INV
    assert call([(p, 4097, 0, 0)], U8, 4097, 2) == INV
    assert call([(p, 16, 0, 0)], U8, 16, 4097) == INV
    assert call([(p, 16, 0, 0)], U8, 0, 4) == INV and call([(p, 16, 0, 0)], U8, 16, 0) == INV
    assert call([(p, 16, 0, 0)], U8, 16, 4, n=-1) == INV
    assert call([(p, 19, 4, 0)], U8, 16, 4) == INV                # pitch_px < x + width
    assert call([(p, 16, 0, 0), (p, 16, 1, 0)], U8, 16, 4) == INV
    assert call([(p + 1, 16, 0, 0)], U16, 16, 4) == INV           # a 16-bit plane at an odd address
    assert call([(None, 16, 0, 0)], U8, 16, 4) == INV
    assert call([(p, 16, -1, 0)], U8, 8, 4) == INV
    assert _lib.lib.omr_encode_png_gray_batch_device(ctx.h, None, 1, U8, 1, 16, 4, out.data_ptr(), out.numel(), None,
                                                     None, None) == INV     # a null table
    assert call([(p + 1, 16, 0, 0)], U8, 16, 4, launches=True) == _lib.OK     # bytes may sit anywhere


# ---- host-fed -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def romio_u16(tmp_path_factory):
    d = tmp_path_factory.mktemp("raw_png")
    rng = np.random.default_rng(80)
    px = np.stack([microscopy_u16(200, 300, rng) for _ in range(6)]).reshape(1, 3, 2, 200, 300)
    path = d / "pixels.romio"
    write_romio(path, px, U16)
    return d, path, px


@pytest.mark.parametrize("dma", [True, False])
def test_pixel_buffer_tiles_png(ctx, romio_u16, dma):
    _, path, px = romio_u16
    reqs = [(0, 0, 0, 0, 0), (1, 2, 0, 37, 11), (0, 1, 0, 200, 140), (1, 0, 0, 201, 140), (1, 1, 0, 199, 139)]
    _lib.check(_lib.lib.omr_ctx_set_pixel_buffer_dma(ctx.h, int(dma)), ctx.h)
    try:
        with PixelBuffer(path, 300, 200, 2, 3, 1, U16) as pb:
            with pytest.raises(omr.OmrError) as e:
                pb.tiles_png(ctx, reqs, 100, 60)
            assert e.value.statuses == [0, 0, 0, _lib.INVALID_ARGUMENT, 0]   # the tile past x fails alone
            files = e.value.files
            assert files[3] == b""
            good = [r for i, r in enumerate(reqs) if i != 3]
            assert pb.tiles_png(ctx, good, 100, 60) == [f for i, f in enumerate(files) if i != 3]
            for (z, c, t, x, y), f in zip(good, pb.tiles_png(ctx, good, 100, 60)):
                check_file(f, px[t, c, z, y:y + 60, x:x + 100], U16)
                assert np.array_equal(pb.get_tile(z, c, t, x, y, 100, 60).astype(np.uint16),
                                      px[t, c, z, y:y + 60, x:x + 100])
            assert pb.tiles_png(ctx, [], 100, 60) == []
            # the files of the device call on the same pixels
            import torch
            assert torch.cuda.is_available()
            dev = to_device(px[0, 2, 1], True)
            res, _ = run(ctx, [(dev, 300, 37, 11)], U16, 100, 60)
            assert res[0][2] == files[1]
    finally:
        _lib.check(_lib.lib.omr_ctx_set_pixel_buffer_dma(ctx.h, 1), ctx.h)


def test_pixel_buffer_tiles_png_level_view(ctx, romio_u16):
    d, path, px = romio_u16
    side = d / "pixels.pyr"
    with PixelBuffer(path, 300, 200, 2, 3, 1, U16) as pb:
        pb.build_pyramid(ctx, side, n_levels=3)
        pb.attach_pyramid(side)
        with pb.level(1) as view:
            assert (view.size_x, view.size_y) == (150, 100)
            reqs = [(0, 0, 0, 0, 0), (1, 2, 0, 50, 40), (0, 1, 0, 86, 51)]
            files = view.tiles_png(ctx, reqs, 64, 48)
            for (z, c, t, x, y), f in zip(reqs, files):
                check_file(f, view.get_tile(z, c, t, x, y, 64, 48).astype(np.uint16), U16)
            with pytest.raises(omr.OmrError) as e:
                view.tiles_png(ctx, [(0, 0, 0, 87, 0)], 64, 48)
            assert e.value.statuses == [_lib.INVALID_ARGUMENT]


def test_pixel_buffer_tiles_png_rejects_float(ctx, tmp_path):
    write_romio(tmp_path / "f.romio", np.zeros((1, 1, 1, 8, 8), np.float32), _lib.PIXELS_FLOAT)
    with PixelBuffer(tmp_path / "f.romio", 8, 8, 1, 1, 1, _lib.PIXELS_FLOAT) as pb:
        with pytest.raises(omr.OmrError) as e:
            pb.tiles_png(ctx, [(0, 0, 0, 0, 0)], 4, 4)
        assert e.value.status == _lib.INVALID_ARGUMENT
        assert len(pb.tile_tiff(0, 0, 0, 0, 0, 4, 4)) == _lib.lib.omr_tiff_raw_max_bytes(4, 4, _lib.PIXELS_FLOAT)


# ---- the existing encoders after a grey batch ---------------------------------------------------
def test_existing_encoders_unchanged_after_gray_batch(ctx):
    import torch
    rng = np.random.default_rng(90)
    yy, xx = np.mgrid[0:96, 0:128]
    argb = np.stack([((xx * 2 + i) << 16 | (yy * 2) << 8 | ((xx + yy) % 256)).astype(np.uint32) | 0xFF000000
                     for i in range(3)])
    argb ^= rng.integers(0, 3, argb.shape, dtype=np.uint32)
    masks = [(rng.integers(0, 256, (40 * 24 + 7) // 8, dtype=np.uint8).tobytes(), 40, 24, (255, 0, 0, 255), False, False),
             (rng.integers(0, 256, (33 * 9 + 7) // 8, dtype=np.uint8).tobytes(), 33, 9, (0, 255, 0, 128), True, False)]

    def rgb_and_masks(c):
        d = torch.from_numpy(argb.view(np.int32).copy()).to("cuda")
        cap = _lib.lib.omr_png_batch_max_bytes(128, 96, 3, 3)
        out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        offs = torch.zeros(3, dtype=torch.int64, device="cuda")
        lens = torch.zeros(3, dtype=torch.int32, device="cuda")
        c.encode_png_batch_device(d, 3, 128, 96, out, offs, lens, None)
        torch.cuda.synchronize()
        b, o, ln = out.cpu().numpy(), offs.cpu().numpy(), lens.cpu().numpy()
        return [b[o[i]:o[i] + ln[i]].tobytes() for i in range(3)], c.render_shape_mask_png_batch(masks)

    plane = microscopy_u16(96, 128, rng)
    run(ctx, [(to_device(plane, True), 128, 0, 0)] * 5, U16, 128, 96)         # a larger workspace first
    run(ctx, [(to_device(plane, True), 128, 1, 0)], U16, 100, 96)
    after = rgb_and_masks(ctx)
    with omr.Context(0) as fresh:
        assert after == rgb_and_masks(fresh)
    from PIL import Image
    for i, f in enumerate(after[0]):
        got = np.asarray(Image.open(io.BytesIO(f)))
        assert np.array_equal(got, np.stack([(argb[i] >> 16) & 255, (argb[i] >> 8) & 255, argb[i] & 255], -1))
    assert all(st == 0 and len(f) > 0 for st, f in after[1])
