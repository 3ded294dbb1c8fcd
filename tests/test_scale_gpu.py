"""Scaled rendering on the device (K10): omr_scale_argb_device, the fused render + scale kernel,
its fallbacks, the OMR_SCALE_FUSED=0 route, sums above 2^32, statuses, the plan cache, thumbnail
JPEGs and Renderer.renderThumbnail.  Every comparison is exact (test_scale_host.scale_ref)."""
import ctypes

import numpy as np
import pytest

import oracle_lib as O
from k2_cases import context_with
from omr import _lib
from omr.context import make_qdef
from test_scale_host import scale_ref

pytestmark = pytest.mark.gpu

K_RENDER, K_FUSED, K_SCALE = 2, 10, 11          # omr_ctx_kernel_timings kinds
FLIPS = [(False, False), (True, False), (False, True), (True, True)]
PTS = {"u8": (_lib.PIXELS_UINT8, np.uint8), "i8": (_lib.PIXELS_INT8, np.int8),
       "u16": (_lib.PIXELS_UINT16, np.uint16), "i16": (_lib.PIXELS_INT16, np.int16)}
COLOURS = [(255, 0, 0, 255), (0, 255, 0, 200), (0, 0, 255, 255), (255, 255, 0, 128), (0, 255, 255, 255)]
LUT = np.concatenate([np.arange(256), 255 - np.arange(256), (np.arange(256) * 3) % 256]).astype(np.uint8)
SETTINGS = ["fast_int", "fast_frac", "codomain", "log", "reverse", "lut", "grey"]


@pytest.fixture(scope="module")
def unfused():
    with context_with(OMR_SCALE_FUSED="0") as c:
        yield c


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda")


def settings(kind, dtype, na, size_c=None):
    """(qdef, channel bindings) of one of SETTINGS: na active channels, an inactive binding in
    front of the second one when size_c leaves room (a channel's plane index then differs from
    its slot)."""
    info = np.iinfo(dtype)
    lo, hi = float(info.min), float(info.max)
    span = hi - lo
    chans = []
    for i in range(na):
        ws = lo + np.floor(span * (0.05 + 0.07 * i))
        we = hi - np.floor(span * (0.10 + 0.05 * i))
        if kind == "fast_frac":
            ws, we = ws + 0.5, we - 0.25
        c = {"active": True, "input_start": ws, "input_end": we, "global_min": lo, "global_max": hi,
             "rgba": COLOURS[i % len(COLOURS)]}
        if kind == "log" and i == 0:
            c.update(family=_lib.FAMILY_LOGARITHMIC, input_start=max(ws, 1.0))
        if kind == "reverse" and i == na - 1:
            c["reverse"] = True
        if kind == "lut" and i == 0:
            c["lut"] = LUT
        chans.append(c)
    if size_c is None:
        size_c = na + 1
    while len(chans) < size_c:
        chans.insert(1 if len(chans) > 1 else 0, {"active": False, "input_start": lo, "input_end": hi,
                                                  "global_min": lo, "global_max": hi, "rgba": (255, 255, 255, 255)})
    q = make_qdef("greyscale") if kind == "grey" else make_qdef("rgb", cd_start=10, cd_end=200) if kind == "codomain" \
        else make_qdef("rgb")
    return q, chans


def planes_for(rng, dtype, size_c, h, w, be):
    info = np.iinfo(dtype)
    out = []
    for _ in range(size_c):
        p = rng.integers(info.min, int(info.max) + 1, (h, w), dtype=np.int64).astype(dtype)
        p.flat[:2] = [info.min, info.max]
        out.append(p.astype(p.dtype.newbyteorder(">")) if be and p.dtype.itemsize > 1 else p)
    return out


def run_scaled(ctx, q, chans, images, pt, w, h, tw, th, be=False, flip=(False, False), strided=False, base_offset=0):
    """images: [n][size_c] numpy planes.  Returns (argb [n][th][tw], statuses, kernel kinds, the
    status of the synchronize that followed)."""
    import torch
    n, c = len(images), len(images[0])
    raw = np.stack([np.stack([np.ascontiguousarray(p).view(np.uint8).reshape(-1) for p in im]) for im in images])
    plane = raw.shape[2]
    buf = torch.zeros(raw.size + 64, dtype=torch.uint8, device="cuda")
    buf[base_offset:base_offset + raw.size] = torch.from_numpy(raw.reshape(-1).copy()).to("cuda")
    base = buf.data_ptr() + base_offset
    out = torch.zeros((n, th, tw), dtype=torch.int32, device="cuda")
    status = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    ctx.enable_kernel_timing(True)
    try:
        if strided:
            ctx.render_scaled_batch_strided_device(q, chans, base, c * plane, plane, n, pt, w, h, out, tw, th, status,
                                                   big_endian=be, flip_h=flip[0], flip_v=flip[1])
        else:
            table = torch.tensor([[base + (t * c + k) * plane for k in range(c)] for t in range(n)], dtype=torch.int64,
                                 device="cuda")
            ctx.render_scaled_batch_device(q, chans, table, n, pt, w, h, out, tw, th, status, big_endian=be,
                                           flip_h=flip[0], flip_v=flip[1])
        try:
            ctx.synchronize()
            sync = 0
        except _lib.OmrError as e:
            sync = e.status
        kinds = [k for _, k in ctx.kernel_timings()]
    finally:
        ctx.enable_kernel_timing(False)
    return out.cpu().numpy().view(np.uint32), list(status.cpu().numpy()), kinds, sync


def oracle_scaled(q, chans, images, pt, w, h, tw, th, be, flip):
    out = []
    for im in images:
        st, argb = O.render(chans, im, pt, w, h, big_endian=be, flip_h=flip[0], flip_v=flip[1], qdef=q)
        assert st == 0
        out.append(scale_ref(argb, tw, th))
    return np.stack(out)


def own_full_render(ctx, q, chans, image, pt, w, h, be, flip):
    import torch
    out = torch.empty((h, w), dtype=torch.int32, device="cuda")
    ctx.render_packed_int_device(q, chans, [dev(p) for p in image], pt, w, h, out, big_endian=be, flip_h=flip[0],
                                 flip_v=flip[1])
    ctx.synchronize()
    return out.cpu().numpy().view(np.uint32)


# ---- 1. omr_scale_argb_device ----------------------------------------------------------------------
ARGB_SHAPES = [(1, 1, 1, 1), (7, 5, 7, 5), (7, 5, 1, 1), (16, 16, 4, 4), (9, 13, 4, 6), (33, 17, 32, 16),
               (300, 200, 96, 64), (200, 131, 97, 61)]


def _scale_argb(ctx, src, tw, th, w=None):
    """src: uint32 [n][H][row stride]; w: the image width when the stride is larger."""
    import torch
    n, h, rs = src.shape
    row_stride = rs if w else 0
    w = w or rs
    d = torch.from_numpy(src.view(np.int32).copy()).to("cuda")
    out = torch.zeros((n, th, tw), dtype=torch.int32, device="cuda")
    ctx.enable_kernel_timing(True)
    try:
        ctx.scale_argb_device(d, n, w, h, out, tw, th, row_stride=row_stride)
        ctx.synchronize()
        kinds = [k for _, k in ctx.kernel_timings()]
    finally:
        ctx.enable_kernel_timing(False)
    assert kinds == [K_SCALE]
    return out.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("w,h,tw,th", ARGB_SHAPES)
def test_scale_argb_against_the_restatement(ctx, w, h, tw, th):
    rng = np.random.default_rng(w * 1000 + h)
    src = rng.integers(0, 2 ** 32, (1, h, w), dtype=np.uint64).astype(np.uint32)
    np.testing.assert_array_equal(_scale_argb(ctx, src, tw, th)[0], scale_ref(src[0], tw, th))


def test_scale_argb_half_rounds_up(ctx):
    assert _scale_argb(ctx, np.array([[[0, 1]]], np.uint32), 1, 1)[0, 0, 0] == 1


def test_scale_argb_row_stride_and_three_images(ctx):
    rng = np.random.default_rng(77)
    w, h, rs, tw, th = 50, 37, 64, 17, 11
    src = rng.integers(0, 2 ** 32, (3, h, rs), dtype=np.uint64).astype(np.uint32)
    got = _scale_argb(ctx, src, tw, th, w=w)
    for k in range(3):
        np.testing.assert_array_equal(got[k], scale_ref(src[k, :, :w], tw, th), err_msg=f"image {k}")


# ---- 2. the fused route against the CPU restatement -------------------------------------------------
_small = {}


def _small_case(name, be, na, kind):
    """64 x 48 -> 24 x 18 inputs and their reference, computed once."""
    key = (name, be, na, kind)
    if key not in _small:
        pt, dtype = PTS[name]
        q, chans = settings(kind, dtype, na)
        case = SETTINGS.index(kind) + 7 * na + 31 * be + 67 * list(PTS).index(name)
        images = [planes_for(np.random.default_rng(2000 + case), dtype, len(chans), 48, 64, be)]
        flip = FLIPS[case % 4]
        _small[key] = (q, chans, images, flip, oracle_scaled(q, chans, images, pt, 64, 48, 24, 18, be, flip))
    return _small[key]


@pytest.mark.parametrize("na", [1, 2, 4])
@pytest.mark.parametrize("be", [False, True], ids=["le", "be"])
@pytest.mark.parametrize("name", list(PTS))
def test_fused_every_type_and_setting(ctx, name, be, na):
    """64 x 48 -> 24 x 18 (8 chunks per row: 32 lane groups share each output row's 2.67 source
    rows) under every setting of SETTINGS, flips rotating."""
    pt, _ = PTS[name]
    for kind in SETTINGS:
        q, chans, images, flip, exp = _small_case(name, be, na, kind)
        got, st, kinds, sync = run_scaled(ctx, q, chans, images, pt, 64, 48, 24, 18, be, flip)
        assert kinds == [K_FUSED] and st == [0] and sync == 0, (kind, kinds, st)
        np.testing.assert_array_equal(got, exp, err_msg=kind)


_mid = {}


def _mid_case(name, kind):
    """256 x 256 -> 96 x 96 inputs and their reference (tests 2 and 4 share them)."""
    key = (name, kind)
    if key not in _mid:
        pt, dtype = PTS[name]
        case = SETTINGS.index(kind) + 7 * list(PTS).index(name)
        na, be = (1, 2, 4)[case % 3], case % 2 == 1
        q, chans = settings(kind, dtype, na)
        images = [planes_for(np.random.default_rng(3000 + case), dtype, len(chans), 256, 256, be)]
        flip = FLIPS[(case // 2) % 4]
        _mid[key] = (q, chans, images, be, flip, oracle_scaled(q, chans, images, pt, 256, 256, 96, 96, be, flip))
    return _mid[key]


@pytest.mark.parametrize("kind", SETTINGS)
@pytest.mark.parametrize("name", list(PTS))
def test_fused_256_to_96(ctx, name, kind):
    q, chans, images, be, flip, exp = _mid_case(name, kind)
    got, st, kinds, sync = run_scaled(ctx, q, chans, images, PTS[name][0], 256, 256, 96, 96, be, flip)
    assert kinds == [K_FUSED] and st == [0] and sync == 0
    np.testing.assert_array_equal(got, exp)


@pytest.mark.parametrize("flip", FLIPS)
def test_fused_every_flip(ctx, flip):
    q, chans = settings("fast_int", np.uint16, 3)
    images = [planes_for(np.random.default_rng(41), np.uint16, len(chans), 56, 72, True)]
    got, st, kinds, _ = run_scaled(ctx, q, chans, images, _lib.PIXELS_UINT16, 72, 56, 31, 23, True, flip)
    assert kinds == [K_FUSED]
    np.testing.assert_array_equal(got, oracle_scaled(q, chans, images, _lib.PIXELS_UINT16, 72, 56, 31, 23, True, flip))


def test_fused_c2_shape(ctx):
    """One 1024 x 1024 four-channel big-endian uint16 image -> 96 x 96 (the thumbnail of a C2 tile)."""
    from omr.synthetic import c2_channels, tile_u16
    planes = [p.astype(">u2") for p in tile_u16(7, 4, 1024, 1024)]
    chans = c2_channels(4)
    q = make_qdef("rgb")
    got, st, kinds, sync = run_scaled(ctx, q, chans, [planes], _lib.PIXELS_UINT16, 1024, 1024, 96, 96, True)
    assert kinds == [K_FUSED] and st == [0] and sync == 0
    np.testing.assert_array_equal(got, oracle_scaled(q, chans, [planes], _lib.PIXELS_UINT16, 1024, 1024, 96, 96, True,
                                                     (False, False)))


@pytest.mark.parametrize("strided,n", [(False, 3), (True, 2)], ids=["table-3", "strided-2"])
@pytest.mark.parametrize("name", ["u8", "i16"])
def test_fused_batches(ctx, name, strided, n):
    """Distinct images through the pointer table and the strided layout.  2560 wide: 320 chunks
    per row, the layout where a lane walks chunk columns t, t + 256 (a ragged second pass); 88
    wide at the identity size and down to one pixel."""
    pt, dtype = PTS[name]
    q, chans = settings("fast_frac", dtype, 2)
    rng = np.random.default_rng(55 + n)
    for w, h, tw, th in ((2560, 24, 103, 7), (88, 40, 88, 40), (88, 40, 1, 1)):
        images = [planes_for(rng, dtype, len(chans), h, w, False) for _ in range(n)]
        got, st, kinds, sync = run_scaled(ctx, q, chans, images, pt, w, h, tw, th, False, (True, False), strided)
        assert kinds == [K_FUSED] and st == [0] * n and sync == 0
        np.testing.assert_array_equal(got, oracle_scaled(q, chans, images, pt, w, h, tw, th, False, (True, False)),
                                      err_msg=f"{w}x{h} -> {tw}x{th}")


# ---- 3. the fallbacks -------------------------------------------------------------------------------
def _fallback(ctx, q, chans, image, pt, w, h, tw, th, be=False, flip=(False, True), expect=(K_RENDER, K_SCALE), **kw):
    got, st, kinds, sync = run_scaled(ctx, q, chans, [image], pt, w, h, tw, th, be, flip, **kw)
    assert kinds == list(expect), kinds
    assert st == [0] and sync == 0
    full = own_full_render(ctx, q, chans, image, pt, w, h, be, flip)
    np.testing.assert_array_equal(got[0], scale_ref(full, tw, th))


def _float_chans(n, lo=0.0, hi=60000.0):
    return [{"active": True, "input_start": lo + 1000.0 * i, "input_end": hi - 500.0 * i,
             "rgba": COLOURS[i % len(COLOURS)]} for i in range(n)]


def test_fallback_five_channels(ctx):
    q, chans = settings("fast_int", np.uint16, 5, size_c=5)
    _fallback(ctx, q, chans, planes_for(np.random.default_rng(60), np.uint16, 5, 48, 64, True), _lib.PIXELS_UINT16,
              64, 48, 24, 18, be=True)


@pytest.mark.parametrize("name", ["float32", "float64", "uint32"])
def test_fallback_wide_pixel_types(ctx, name):
    """float32 with monotone windows (K2's threshold mode), float64 and uint32 (evaluated)."""
    pt, dtype = {"float32": (_lib.PIXELS_FLOAT, np.float32), "float64": (_lib.PIXELS_DOUBLE, np.float64),
                 "uint32": (_lib.PIXELS_UINT32, np.uint32)}[name]
    rng = np.random.default_rng(61)
    image = [rng.uniform(-2000, 70000, (48, 64)).astype(dtype) if name != "uint32"
             else rng.integers(0, 70000, (48, 64)).astype(dtype) for _ in range(2)]
    chans = _float_chans(2)
    if name == "uint32":
        for c in chans:
            c["global_min"], c["global_max"] = 0.0, 4294967295.0
    _fallback(ctx, make_qdef("rgb"), chans, image, pt, 64, 48, 24, 18)


def test_fallback_width_63(ctx):
    q, chans = settings("fast_int", np.uint16, 2)
    _fallback(ctx, q, chans, planes_for(np.random.default_rng(62), np.uint16, len(chans), 48, 63, False),
              _lib.PIXELS_UINT16, 63, 48, 24, 18)


def test_fallback_plane_one_pixel_off_alignment(ctx):
    """The strided base one pixel past a 16-byte boundary; the same call on the boundary is fused."""
    q, chans = settings("fast_int", np.uint16, 2, size_c=2)
    image = planes_for(np.random.default_rng(63), np.uint16, 2, 48, 64, False)
    _fallback(ctx, q, chans, image, _lib.PIXELS_UINT16, 64, 48, 24, 18, strided=True, base_offset=2)
    _fallback(ctx, q, chans, image, _lib.PIXELS_UINT16, 64, 48, 24, 18, strided=True, base_offset=0, expect=(K_FUSED,))


def test_output_width_limit_both_sides(ctx):
    """The fused kernel's own condition: out_w <= 1024 (LDS accumulators, 11-bit weights)."""
    q, chans = settings("fast_int", np.uint16, 1, size_c=1)
    rng = np.random.default_rng(64)
    _fallback(ctx, q, chans, planes_for(rng, np.uint16, 1, 16, 2048, False), _lib.PIXELS_UINT16, 2048, 16, 1024, 8,
              expect=(K_FUSED,))
    _fallback(ctx, q, chans, planes_for(rng, np.uint16, 1, 16, 2064, False), _lib.PIXELS_UINT16, 2064, 16, 1032, 8)


# ---- 4. OMR_SCALE_FUSED=0 ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", SETTINGS)
@pytest.mark.parametrize("name", list(PTS))
def test_unfused_context_gives_identical_bytes(unfused, name, kind):
    q, chans, images, be, flip, exp = _mid_case(name, kind)
    got, st, kinds, sync = run_scaled(unfused, q, chans, images, PTS[name][0], 256, 256, 96, 96, be, flip)
    assert kinds == [K_RENDER, K_SCALE] and st == [0] and sync == 0
    np.testing.assert_array_equal(got, exp)


# ---- 5. sums above 2^32 -----------------------------------------------------------------------------
BIG_W, BIG_H, BIG_TW, BIG_TH = 4200, 4100, 96, 93        # 255 * 4200 * 4100 = 4.39e9 > 2^32


def test_above_2_32_all_ones(ctx):
    src = np.full((1, BIG_H, BIG_W), 0xFFFFFFFF, np.uint32)
    assert (_scale_argb(ctx, src, BIG_TW, BIG_TH) == 0xFFFFFFFF).all()


def test_above_2_32_random_argb(ctx):
    src = np.random.default_rng(80).integers(0, 2 ** 32, (1, BIG_H, BIG_W), dtype=np.uint64).astype(np.uint32)
    np.testing.assert_array_equal(_scale_argb(ctx, src, BIG_TW, BIG_TH)[0], scale_ref(src[0], BIG_TW, BIG_TH))


def test_above_2_32_fused_render(ctx):
    """One uint8 channel, bright enough that an output pixel's sum passes 2^32: the fused kernel's
    64-bit LDS accumulators."""
    rng = np.random.default_rng(81)
    plane = rng.integers(0, 256, (BIG_H, BIG_W)).astype(np.uint8)
    plane[: BIG_H // 2] |= 0xFC          # 252 * W * H > 2^32
    chans = [{"active": True, "input_start": 0.0, "input_end": 255.0, "global_min": 0.0, "global_max": 255.0,
              "rgba": (255, 255, 255, 255)}]
    _fallback(ctx, make_qdef("rgb"), chans, [plane], _lib.PIXELS_UINT8, BIG_W, BIG_H, BIG_TW, BIG_TH,
              flip=(True, True), expect=(K_FUSED,))


# ---- 6. statuses ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["u8", "i16"])
@pytest.mark.parametrize("route", ["fused", "unfused"])
def test_quantization_status_per_image(ctx, unfused, route, name):
    pt, dtype = PTS[name]
    c, kinds_exp = (ctx, [K_FUSED]) if route == "fused" else (unfused, [K_RENDER, K_SCALE])
    q, chans = settings("fast_int", dtype, 2, size_c=2)
    limit = float(np.iinfo(dtype).max - 20)
    chans[1]["global_max"] = limit
    rng = np.random.default_rng(90)
    images = [planes_for(rng, dtype, 2, 48, 64, False) for _ in range(3)]
    for im in images:
        im[1] = np.minimum(im[1], dtype(limit))
    images[1][1][29, 41] = dtype(limit + 1)
    got, st, kinds, sync = run_scaled(c, q, chans, images, pt, 64, 48, 24, 18)
    assert kinds == kinds_exp
    assert st == [0, _lib.QUANTIZATION, 0] and sync == _lib.QUANTIZATION
    exp = oracle_scaled(q, chans, [images[0], images[2]], pt, 64, 48, 24, 18, False, (False, False))
    np.testing.assert_array_equal(got[[0, 2]], exp)


@pytest.mark.parametrize("tw,th,n", [(65, 18, 1), (24, 49, 1), (24, 0, 1), (0, 18, 1), (24, 18, 0), (24, 18, -1)])
def test_invalid_arguments(ctx, tw, th, n):
    import torch
    q, chans = settings("fast_int", np.uint16, 1, size_c=1)
    data = torch.zeros(64 * 48 * 2, dtype=torch.uint8, device="cuda")
    out = torch.zeros(64 * 64, dtype=torch.int32, device="cuda")
    table = torch.tensor([data.data_ptr()], dtype=torch.int64, device="cuda")
    for call in (lambda: ctx.render_scaled_batch_device(q, chans, table, n, _lib.PIXELS_UINT16, 64, 48, out, tw, th),
                 lambda: ctx.render_scaled_batch_strided_device(q, chans, data, 64 * 48 * 2, 64 * 48 * 2, n,
                                                                _lib.PIXELS_UINT16, 64, 48, out, tw, th)):
        with pytest.raises(_lib.OmrError) as ei:
            call()
        assert ei.value.status == _lib.INVALID_ARGUMENT
    if n == 1:
        with pytest.raises(_lib.OmrError) as ei:
            ctx.scale_argb_device(out, 1, 64, 48, out, tw, th)
        assert ei.value.status == _lib.INVALID_ARGUMENT


# ---- 7. determinism and the plan cache --------------------------------------------------------------
def _cache_stats(c):
    h, m = ctypes.c_uint64(0), ctypes.c_uint64(0)
    _lib.check(_lib.lib.omr_debug_plan_cache_stats(c.h, ctypes.byref(h), ctypes.byref(m)), c.h)
    return h.value, m.value


def test_deterministic_and_shares_the_plan_cache_slot():
    import omr
    q, chans = settings("log", np.uint16, 3)
    images = [planes_for(np.random.default_rng(95), np.uint16, len(chans), 256, 256, True)]
    with omr.Context(0) as c:
        a, _, kinds, _ = run_scaled(c, q, chans, images, _lib.PIXELS_UINT16, 256, 256, 96, 96, True)
        assert kinds == [K_FUSED] and _cache_stats(c) == (0, 1)
        own_full_render(c, q, chans, images[0], _lib.PIXELS_UINT16, 256, 256, True, (False, False))
        assert _cache_stats(c) == (1, 1)                 # the plain render found the scaled render's slot
        b, _, _, _ = run_scaled(c, q, chans, images, _lib.PIXELS_UINT16, 256, 256, 96, 96, True)
        assert _cache_stats(c) == (2, 1)
        np.testing.assert_array_equal(a, b)


# ---- 8. thumbnail JPEGs -----------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["fused", "unfused"])
def test_thumbnail_jpeg_batch(ctx, unfused, route):
    import torch
    c = ctx if route == "fused" else unfused
    pt, w, h, tw, th, n = _lib.PIXELS_UINT16, 256, 192, 96, 72, 3
    q, chans = settings("fast_int", np.uint16, 3, size_c=3)
    rng = np.random.default_rng(99)
    # smooth planes (a JPEG of noise says little about the coder's run lengths)
    yy, xx = np.mgrid[0:h, 0:w]
    images = [[((np.sin(xx / (9.0 + k + 3 * t)) + np.cos(yy / (7.0 + 2 * k))) * 14000 + 30000 +
                rng.integers(0, 900, (h, w))).astype(np.uint16) for k in range(3)] for t in range(n)]
    small, st, kinds, _ = run_scaled(c, q, chans, images, pt, w, h, tw, th, flip=(False, True))
    exp = oracle_scaled(q, chans, images, pt, w, h, tw, th, False, (False, True))
    np.testing.assert_array_equal(small, exp)

    def files_of(call):
        d_out = torch.zeros(n * (tw * th * 4 + 4096), dtype=torch.uint8, device="cuda")
        offs = torch.zeros(n, dtype=torch.int64, device="cuda")
        lens = torch.zeros(n, dtype=torch.int32, device="cuda")
        stat = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        call(d_out, offs, lens, stat)
        c.synchronize()
        assert list(stat.cpu().numpy()) == [0] * n
        o, ln, b = offs.cpu().numpy(), lens.cpu().numpy(), d_out.cpu().numpy()
        return [b[int(o[i]):int(o[i]) + int(ln[i])].tobytes() for i in range(n)]

    keep = [[dev(p) for p in im] for im in images]
    table = torch.tensor([[p.data_ptr() for p in im] for im in keep], dtype=torch.int64, device="cuda")
    thumbs = files_of(lambda d, o, ln, s: c.render_thumbnail_jpeg_batch_device(
        q, chans, table, n, pt, w, h, tw, th, 0.9, d, o, ln, s, flip_v=True))
    d_small = torch.from_numpy(small.view(np.int32).copy()).to("cuda")
    encoded = files_of(lambda d, o, ln, s: c.encode_jpeg_batch_device(d_small, n, tw, th, 0.9, d, o, ln, s))
    assert thumbs == encoded
    assert thumbs == [O.encode_jpeg(exp[i], tw, th, 0.9) for i in range(n)]


# ---- 9. Renderer.renderThumbnail --------------------------------------------------------------------
def test_renderer_render_thumbnail(ctx):
    import omr
    w, h = 300, 200
    assert omr.thumbnail_size(w, h, 96) == (96, 64)
    rng = np.random.default_rng(101)
    planes = [rng.integers(0, 65536, (h, w)).astype(">u2") for _ in range(3)]
    r = omr.Renderer(ctx, _lib.PIXELS_UINT16, w, h, 3)
    r.setModel("rgb")
    for k, rgb in enumerate([(255, 0, 0), (0, 255, 0), (0, 0, 255)]):
        r.setChannelWindow(k, 500.0 + 100 * k, 50000.0 - 1000 * k)
        r.setRGBA(k, *rgb, 255)
    got = r.renderThumbnail(planes)
    assert got.shape == (64, 96)
    st, full = O.render(r.rdef.channels, planes, _lib.PIXELS_UINT16, w, h, big_endian=True, qdef=r.qdef())
    assert st == 0
    np.testing.assert_array_equal(got, scale_ref(full, 96, 64))
