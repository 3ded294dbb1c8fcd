"""Resolution pyramids on the GPU (K11): omr_pyramid_build_device bit for bit against the numpy
restatement (tests/test_pyramid_host.py::pyramid_ref) for every pixel type, byte order and rule at
the smallest sizes where each path of the kernel can go wrong; planes, strides and the per-pixel
form; determinism and launch counts; build_pyramid's sidecar byte for byte; and a tile request
with res > 0 end to end through the handler and the batcher."""
import ctypes
import io

import numpy as np
import pytest

import oracle_lib as O
from omr import Batcher, PixelBuffer, _lib, write_pyramid, write_romio
from omr._lib import lib
from omr.request import ImageRegionCtx, ImageRegionRequestHandler, create_rendering_def, update_settings
from test_pyramid_host import MEAN, NP_TYPES, SUB, max_levels, pyramid_ref

pytestmark = pytest.mark.gpu

# 2x2 one pixel out; 3x5 odd edges; 17x9 under one lane block, ragged; 64x64 exact blocks; 72x40
# whole chunks, partial block rows; 520x36 one wave row plus a ragged tail (crosses the 512-pixel
# wave width of 16-bit pixels); 1032x24 two wave rows; 250x130 width not a multiple of 8
SIZES = [(2, 2), (3, 5), (17, 9), (64, 64), (72, 40), (520, 36), (1032, 24), (250, 130)]
KIND_PYRAMID = 12


def make_plane(pt, w, h, seed):
    """Random pixels with the type's hard values sprinkled in."""
    dt = NP_TYPES[pt]
    rng = np.random.default_rng(seed)
    n = w * h
    if np.issubdtype(dt, np.integer):
        ii = np.iinfo(dt)
        a = rng.integers(ii.min, ii.max, n, dtype=dt, endpoint=True)
        special = np.array([ii.min, ii.max, ii.min + 1, ii.max - 1, 0, 1], dtype=dt)
    else:
        fi = np.finfo(dt)
        bits = {4: np.uint32, 8: np.uint64}[dt().itemsize]
        # random mantissas around 1 (sums that round), a few magnitudes, random bit patterns
        a = (1.0 + rng.random(n)) * rng.choice([1.0, -1.0, 2.0**-20, 2.0**30], n)
        a = a.astype(dt)
        wild = rng.integers(0, np.iinfo(bits).max, n, dtype=bits, endpoint=True).view(dt)
        a = np.where(rng.random(n) < 0.2, wild, a).astype(dt)
        special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, fi.tiny / 4, -fi.tiny / 8, fi.smallest_subnormal,
                            fi.max, -fi.max, 1.0, 1.0 + fi.eps, fi.eps / 2], dtype=dt)
    idx = rng.integers(0, n, min(n, max(4, n // 7)))
    a[idx] = special[rng.integers(0, len(special), len(idx))]
    if n >= 4:
        a[:4] = special[:4]            # the first box: min/max (NaN, +-inf) together
    return a.reshape(h, w)


def file_bytes(a, be):
    """The plane as the bytes the device sees (no arithmetic: NaN payloads survive)."""
    a = np.ascontiguousarray(a)
    raw = a.view(np.uint8).reshape(a.shape + (a.dtype.itemsize,)) if a.dtype.itemsize > 1 else a.view(np.uint8)[..., None]
    return np.ascontiguousarray(raw[..., ::-1] if be else raw).reshape(-1)


def from_bytes(raw, dt, be, shape):
    k = np.dtype(dt).itemsize
    b = np.asarray(raw, np.uint8).reshape(-1, k)
    return np.ascontiguousarray(b[:, ::-1] if be else b).reshape(-1).view(dt).reshape(shape)


def build(ctx, planes, pt, be, rule, n_levels, row_stride=0, width=None, height=None, ptrs=None, keep=None):
    """omr_pyramid_build_device on native numpy planes (or on given device addresses);
    returns [L1, ...] as native arrays [n_planes][h_k][w_k]."""
    import torch
    dt = NP_TYPES[pt]
    k = np.dtype(dt).itemsize
    if ptrs is None:
        height, width = planes[0].shape
        keep = [torch.from_numpy(file_bytes(p, be)).to("cuda") for p in planes]
        ptrs = [t.data_ptr() for t in keep]
    n = len(ptrs)
    outs = [torch.full((n * (width >> lv) * (height >> lv) * k + 16,), 0xA5, dtype=torch.uint8, device="cuda")
            for lv in range(1, n_levels)]
    ctx.pyramid_build_device(ptrs, pt, width, height, outs, n_levels, rule=rule, big_endian=be, row_stride=row_stride)
    ctx.synchronize()
    got = []
    for lv, o in zip(range(1, n_levels), outs):
        raw = o.cpu().numpy()
        assert np.all(raw[-16:] == 0xA5), "write past the level"
        got.append(from_bytes(raw[:-16], dt, be, (n, height >> lv, width >> lv)))
    return got


def same(got, exp, rule):
    if rule == MEAN and np.issubdtype(exp.dtype, np.floating):
        return np.array_equal(got, exp, equal_nan=True)
    return np.array_equal(got.view(np.uint8), np.ascontiguousarray(exp).view(np.uint8))   # bit for bit


def check(got, planes, rule, n_levels, what=""):
    exp = pyramid_ref(np.stack(planes), rule, n_levels)
    assert len(got) == n_levels - 1
    for lv in range(1, n_levels):
        assert got[lv - 1].shape == exp[lv].shape, (what, lv)
        if not same(got[lv - 1], exp[lv], rule):
            bad = np.argwhere(~((got[lv - 1] == exp[lv]) | ((got[lv - 1] != got[lv - 1]) & (exp[lv] != exp[lv]))))
            raise AssertionError(f"{what} level {lv}: {len(bad)} pixels differ, first at {bad[:4].tolist()}")


@pytest.mark.parametrize("be", [True, False], ids=["be", "le"])
@pytest.mark.parametrize("pt", sorted(NP_TYPES), ids=lambda p: NP_TYPES[p].__name__)
def test_build_device_exact(ctx, pt, be):
    for i, (w, h) in enumerate(SIZES):
        plane = make_plane(pt, w, h, 100 * pt + i)
        n_levels = max_levels(w, h)                     # the deepest valid pyramid
        for rule in (SUB, MEAN):
            got = build(ctx, [plane], pt, be, rule, n_levels)
            check(got, [plane], rule, n_levels, f"{w}x{h} rule {rule}")


@pytest.mark.parametrize("n", [1, 3, 32])
def test_distinct_planes(ctx, n):
    pt = _lib.PIXELS_UINT16
    planes = [make_plane(pt, 72, 40, 7 + p) for p in range(n)]
    for rule in (SUB, MEAN):
        check(build(ctx, planes, pt, True, rule, 5), planes, rule, 5, f"{n} planes")


@pytest.mark.parametrize("pt", [_lib.PIXELS_UINT8, _lib.PIXELS_INT16, _lib.PIXELS_FLOAT, _lib.PIXELS_DOUBLE],
                         ids=lambda p: NP_TYPES[p].__name__)
def test_strides_and_scalar_form(ctx, pt):
    """A region of a wider plane (row_stride_px > width) on and off the 16-byte grid: the vector
    and the per-pixel form give the same bytes, both equal to the restatement."""
    import torch
    k = np.dtype(NP_TYPES[pt]).itemsize
    wide_w, h, w = 176, 40, 128
    wide = make_plane(pt, wide_w, h, 41 + pt)
    dev = torch.from_numpy(file_bytes(wide, True)).to("cuda")
    shifted = torch.zeros(dev.numel() + 64, dtype=torch.uint8, device="cuda")   # the same plane one pixel off the grid
    shifted[k:k + dev.numel()] = dev
    results = []
    for x0, base in [(32, dev.data_ptr()), (1, dev.data_ptr()), (32, shifted.data_ptr() + k)]:
        region = np.ascontiguousarray(wide[:, x0:x0 + w])
        for rule in (SUB, MEAN):
            got = build(ctx, None, pt, True, rule, 6, row_stride=wide_w, width=w, height=h,
                        ptrs=[base + x0 * k], keep=[dev, shifted])
            check(got, [region], rule, 6, f"x0 {x0}")
            results.append(got)
    for a, b in zip(results[0:2], results[4:6]):          # aligned (vector) vs shifted base (per-pixel)
        for la, lb in zip(a, b):
            assert np.array_equal(la.view(np.uint8), lb.view(np.uint8))
    # a packed plane with an explicit stride equal to the width
    plane = make_plane(pt, 72, 40, 5)
    t = torch.from_numpy(file_bytes(plane, False)).to("cuda")
    check(build(ctx, None, pt, False, MEAN, 4, row_stride=72, width=72, height=40, ptrs=[t.data_ptr()], keep=[t]),
          [plane], MEAN, 4, "stride == width")


def kinds(ctx):
    return [k for _, k in ctx.kernel_timings()]


def test_deterministic_and_launch_counts(ctx):
    planes = [make_plane(_lib.PIXELS_FLOAT, 250, 130, 3 + p) for p in range(3)]
    a = build(ctx, planes, _lib.PIXELS_FLOAT, True, MEAN, 7)
    b = build(ctx, planes, _lib.PIXELS_FLOAT, True, MEAN, 7)
    for la, lb in zip(a, b):
        assert np.array_equal(la.view(np.uint8), lb.view(np.uint8))
    ctx.enable_kernel_timing(True)
    try:
        kinds(ctx)
        u16 = [make_plane(_lib.PIXELS_UINT16, 64, 64, 1)]
        assert build(ctx, u16, _lib.PIXELS_UINT16, True, MEAN, 1) == []
        assert kinds(ctx) == []                                      # n_levels == 1: no launch
        build(ctx, u16, _lib.PIXELS_UINT16, True, MEAN, 4)           # levels 1-3: one launch
        assert kinds(ctx) == [KIND_PYRAMID]
        build(ctx, u16, _lib.PIXELS_UINT16, True, SUB, 5)            # a fourth level across lanes: still one
        assert kinds(ctx) == [KIND_PYRAMID]
        build(ctx, u16, _lib.PIXELS_UINT16, True, MEAN, 6)           # 4 + 1
        assert kinds(ctx) == [KIND_PYRAMID] * 2
        build(ctx, u16, _lib.PIXELS_UINT16, True, MEAN, 7)           # 4 + 2
        assert kinds(ctx) == [KIND_PYRAMID] * 2
        f32 = [make_plane(_lib.PIXELS_FLOAT, 64, 64, 2)]
        build(ctx, f32, _lib.PIXELS_FLOAT, True, MEAN, 4)            # 32-bit pixels: 2 + 1 levels per launch
        assert kinds(ctx) == [KIND_PYRAMID]
        build(ctx, f32, _lib.PIXELS_FLOAT, True, MEAN, 5)            # 3 + 1
        assert kinds(ctx) == [KIND_PYRAMID] * 2
    finally:
        ctx.enable_kernel_timing(False)


def test_invalid_arguments_leave_the_context_usable(ctx):
    import torch
    pt = _lib.PIXELS_UINT16
    plane = make_plane(pt, 64, 48, 9)
    src = torch.from_numpy(file_bytes(plane, True)).to("cuda")
    out = [torch.zeros(64 * 48 * 2, dtype=torch.uint8, device="cuda") for _ in range(5)]
    P = (ctypes.c_void_p * 33)(*([src.data_ptr()] * 33))
    L = (ctypes.c_void_p * 16)(*([o.data_ptr() for o in out] + [out[0].data_ptr()] * 11))
    odd = (ctypes.c_void_p * 1)(src.data_ptr() + 1)
    nullp = (ctypes.c_void_p * 1)(None)
    nulll = (ctypes.c_void_p * 2)(out[0].data_ptr(), None)
    oddl = (ctypes.c_void_p * 2)(out[0].data_ptr(), out[1].data_ptr() + 1)

    def call(planes=P, n=1, ptype=pt, be=1, w=64, h=48, stride=0, rule=MEAN, n_levels=3, levels=L, c=ctx.h):
        return lib.omr_pyramid_build_device(c, planes, n, ptype, be, w, h, stride, rule, n_levels, levels)

    bad = [dict(planes=None), dict(levels=None), dict(planes=nullp), dict(levels=nulll), dict(ptype=8), dict(ptype=-1),
           dict(rule=2), dict(rule=-1), dict(n=0), dict(n=33), dict(n=-1), dict(n_levels=0), dict(n_levels=-2),
           dict(n_levels=7),                      # 1 + floor(log2(48)) = 6
           dict(n_levels=17, w=1 << 17, h=1 << 17), dict(stride=63), dict(stride=1), dict(stride=-5),
           dict(w=65536, h=32768),                # 2^31 pixels
           dict(w=0), dict(h=-1), dict(planes=odd), dict(levels=oddl)]
    for kw in bad:
        assert call(**kw) == _lib.INVALID_ARGUMENT, kw
        assert ctx.last_error()
    assert call(c=None) == _lib.INVALID_ARGUMENT
    assert call(n_levels=1, levels=None) == _lib.OK       # nothing to write
    # the context still works: a valid call right after
    check(build(ctx, [plane], pt, True, MEAN, 6), [plane], MEAN, 6, "after the invalid calls")
    ctx.synchronize()


# ---- build_pyramid on a ROMIO file -----------------------------------------------------------------
@pytest.mark.parametrize("dims,pt,n_levels", [((130, 70, 2, 3, 2), _lib.PIXELS_UINT16, 7),
                                              ((40, 40, 1, 2, 1), _lib.PIXELS_FLOAT, 4),
                                              ((33, 18, 5, 4, 2), _lib.PIXELS_UINT16, 3),     # 40 planes: two groups
                                              ((600, 300, 1, 1, 2), _lib.PIXELS_UINT8, 0)],   # default depth: 3 levels
                         ids=["u16", "f32", "40planes", "default"])
def test_build_pyramid_sidecar_byte_identical(ctx, tmp_path, dims, pt, n_levels):
    sx, sy, sz, sc, st = dims
    dt = NP_TYPES[pt]
    rng = np.random.default_rng(sx)
    if np.issubdtype(dt, np.integer):
        px = rng.integers(0, np.iinfo(dt).max, (st, sc, sz, sy, sx), dtype=dt, endpoint=True)
    else:
        px = ((rng.random((st, sc, sz, sy, sx)) - 0.5) * 1e4).astype(dt)           # no NaN: bytes compare
    write_romio(tmp_path / "pixels", px, pt)
    n_eff = n_levels if n_levels > 0 else 3
    with PixelBuffer(tmp_path / "pixels", sx, sy, sz, sc, st, pt) as pb:
        for rule in (SUB, MEAN):
            levels = pyramid_ref(px, rule, n_eff)
            write_pyramid(tmp_path / "expect", levels[1:], pt, rule=rule, size=(sx, sy))
            pb.build_pyramid(ctx, tmp_path / f"built{rule}", rule=rule, n_levels=n_levels)
            built = (tmp_path / f"built{rule}").read_bytes()
            assert built == (tmp_path / "expect").read_bytes(), f"rule {rule}"
            assert not (tmp_path / f"built{rule}.tmp").exists()
            pb.build_pyramid(ctx, tmp_path / "again", rule=rule, n_levels=n_levels)
            assert (tmp_path / "again").read_bytes() == built                     # building twice: the same file
        assert pb.getResolutionLevels() == 1                                      # building does not attach
        pb.attach_pyramid(tmp_path / f"built{MEAN}")
        assert pb.getResolutionLevels() == n_eff
        with pb.level(n_eff - 1) as v:
            lv = pyramid_ref(px, MEAN, n_eff)[-1]
            assert np.array_equal(v.get_tile(sz - 1, sc - 1, st - 1, 0, 0, v.size_x, v.size_y).astype(dt),
                                  lv[st - 1, sc - 1, sz - 1])


def test_build_pyramid_errors(ctx, tmp_path):
    px = np.arange(2 * 20 * 24, dtype=np.uint16).reshape(1, 2, 1, 20, 24)
    write_romio(tmp_path / "pixels", px, _lib.PIXELS_UINT16)
    with PixelBuffer(tmp_path / "pixels", 24, 20, 1, 2, 1, _lib.PIXELS_UINT16) as pb:
        for kw in (dict(rule=2), dict(n_levels=6), dict(n_levels=17)):
            with pytest.raises(_lib.OmrError) as e:
                pb.build_pyramid(ctx, tmp_path / "x", **kw)
            assert e.value.status == _lib.INVALID_ARGUMENT
        with pytest.raises(_lib.OmrError) as e:
            pb.build_pyramid(ctx, tmp_path / "no_such_dir" / "x", n_levels=3)
        assert e.value.status == _lib.INTERNAL and "No such file" in str(e.value)
        pb.build_pyramid(ctx, tmp_path / "ok", n_levels=3)                         # and the context still works
        pb.attach_pyramid(tmp_path / "ok")
        assert pb.getResolutionDescriptions() == [[24, 20], [12, 10], [6, 5]]


# ---- end to end: tile=res,x,y,w,h on a ROMIO buffer with a pyramid -----------------------------------
SX, SY, SZ, SC = 200, 136, 2, 3


@pytest.fixture(scope="module")
def image(tmp_path_factory, ctx):
    from omr.synthetic import microscopy_u16
    d = tmp_path_factory.mktemp("pyr_e2e")
    rng = np.random.default_rng(20261019)
    px = np.stack([np.stack([microscopy_u16(SY, SX, rng) for _ in range(SZ)]) for _ in range(SC)])[None]
    write_romio(d / "pixels", px, _lib.PIXELS_UINT16)
    with PixelBuffer(d / "pixels", SX, SY, SZ, SC, 1, _lib.PIXELS_UINT16) as pb:
        pb.build_pyramid(ctx, d / "pyramid", rule=MEAN, n_levels=3)
    return d, pyramid_ref(px, MEAN, 3)


def params(**kw):
    p = [("imageId", "1"), ("theZ", "1"), ("theT", "0"), ("m", "c"),
         ("c", "1|0:65535$FF0000,2|1755:51199$00FF00,3|3218:26623$0000FF"), ("format", "png")]
    return [(a, b) for a, b in p if a not in kw] + list(kw.items())


def oracle_region(irc, level, x, y, w, h):
    """The CPU restatement's render of level[:, z, y:y+h, x:x+w] with the request's settings and flips."""
    q, b = create_rendering_def(_lib.PIXELS_UINT16, SC)
    update_settings(irc, SC, q, b, None)
    planes = [np.ascontiguousarray(level[0, c, irc.z, y:y + h, x:x + w]).astype(">u2") for c in range(SC)]
    ptrs = (ctypes.c_void_p * SC)(*[p.ctypes.data for p in planes])
    out = np.zeros((h, w), np.uint32)
    assert O.lib.oracle_render_packed_int(ctypes.byref(q), b, SC, ptrs, 0, _lib.PIXELS_UINT16, 1, w, h,
                                          out.ctypes.data) == 0
    st, out = O.flip_int(out, w, h, irc.flipHorizontal, irc.flipVertical)
    assert st == 0
    return out


def rgb(argb):
    return np.stack([(argb >> 16) & 0xFF, (argb >> 8) & 0xFF, argb & 0xFF], -1).astype(np.uint8)


@pytest.mark.parametrize("kw,res,box", [
    (dict(tile="1,1,0,32,32"), 1, (32, 0, 32, 32)),                  # level 1 is 100 x 68
    # level 2 is 50 x 34; flipped horizontally the tile at x = 0 reads from x = 50 - 16 - 0
    (dict(tile="2,0,0,16,16", flip="h"), 2, (34, 0, 16, 16)),
    (dict(tile="2,3,2,16,16"), 2, (48, 32, 2, 2)),                   # the corner tile, cut to the level
    (dict(tile="0,1,1,64,64"), 0, (64, 64, 64, 64)),
])
def test_handler_serves_resolution_levels(ctx, image, kw, res, box):
    from PIL import Image
    d, levels = image
    irc = ImageRegionCtx(params(**kw))
    pb = PixelBuffer(d / "pixels", SX, SY, SZ, SC, 1, _lib.PIXELS_UINT16)
    pb.attach_pyramid(d / "pyramid")
    got = ImageRegionRequestHandler(ctx, irc).render_image_region(pb)
    exp = oracle_region(irc, levels[res], *box)
    img = Image.open(io.BytesIO(got))
    assert img.size == (box[2], box[3])
    np.testing.assert_array_equal(np.asarray(img.convert("RGB")), rgb(exp))


def test_handler_without_sidecar_unchanged(ctx, image):
    from PIL import Image
    d, levels = image
    irc = ImageRegionCtx(params(tile="0,1,1,64,64", flip="v"))
    pb = PixelBuffer(d / "pixels", SX, SY, SZ, SC, 1, _lib.PIXELS_UINT16)
    got = ImageRegionRequestHandler(ctx, irc).render_image_region(pb)
    exp = oracle_region(irc, levels[0], 64, SY - 64 - 64, 64, 64)
    np.testing.assert_array_equal(np.asarray(Image.open(io.BytesIO(got)).convert("RGB")), rgb(exp))


def test_batcher_job_on_a_level_view(ctx, image):
    from omr.synthetic import c2_channels
    d, levels = image
    ch = c2_channels(SC)
    qd = O.make_qdef("rgb")
    with PixelBuffer(d / "pixels", SX, SY, SZ, SC, 1, _lib.PIXELS_UINT16) as pb:
        pb.attach_pyramid(d / "pyramid")
        v = pb.level(1)
    # (the parent is closed: the view keeps the files open)
    reqs = [(i % SZ, 0, 4 * i, 2 * i) for i in range(16)]
    direct = ctx.render_pixel_buffer_tiles(qd, ch, v, reqs, 32, 32, flip_h=True)
    with Batcher(0, max_batch=16, max_wait_us=20000) as b:
        tickets = [b.submit(v, qd, ch, z, t, x, y, 32, 32, flip_h=True, fmt="argb") for (z, t, x, y) in reqs]
        outs = [b.wait(t) for t in tickets]
    v.close()
    for i, (z, t, x, y) in enumerate(reqs):
        got = np.frombuffer(outs[i], np.uint32).reshape(32, 32)
        np.testing.assert_array_equal(got, direct[i])
        planes = [np.ascontiguousarray(levels[1][0, c, z, y:y + 32, x:x + 32]).astype(">u2") for c in range(SC)]
        st, exp = O.render(ch, planes, _lib.PIXELS_UINT16, 32, 32, big_endian=True, flip_h=True)
        assert st == 0
        np.testing.assert_array_equal(got, exp)
