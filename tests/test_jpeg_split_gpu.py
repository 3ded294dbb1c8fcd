"""The split JPEG entropy decode on the GPU (K18a k_jpeg_entropy_split, K18b k_jpeg_dc_sum, then
K17b / K17c unchanged), switched on by Context.set_jpeg_split: omr_jpeg_decode_batch_device,
TiffImage.read_regions and TiffImage.render_tiles give the bytes and statuses of the serial host
decoder on every stream of tests/golden/tiff_jpeg.npz and tests/golden/jpeg_split.npz, and a
context that never made the call (or cleared it) launches what it launched before.  No tolerance
anywhere, no Pillow; damage only ever yields a status."""
import numpy as np
import pytest

import jpeg_split_cases as sc
import omr
import tiff_jpeg_cases as jc
from omr import _lib
from omr.context import make_qdef
from test_tiff_codecs_gpu import REQS, read_checked, rgb_bindings

pytestmark = pytest.mark.gpu

K18A, K18B = 39, 40


class split_on:
    """The session's context with the split decode on; off again behind the block."""

    def __init__(self, ctx, min_bytes=1, bits=0):
        self.ctx, self.args = ctx, (min_bytes, bits)

    def __enter__(self):
        self.ctx.set_jpeg_split(*self.args)

    def __exit__(self, *exc):
        self.ctx.set_jpeg_split(0)


@pytest.fixture(scope="module")
def reference():
    return {s.id: sc.serial(s)[1] for s in sc.ALL}


def groups():
    """The streams that one batch call can take together: the same samples, colour and tables."""
    out = {}
    for s in sc.ALL:
        out.setdefault((s.n, s.ycc, s.tables), []).append(s)
    return list(out.values())


def batch(ctx, streams):
    s0 = streams[0]
    return omr.jpeg_decode_batch_device(ctx, [s.data for s in streams], [(s.w, s.h) for s in streams], s0.n, s0.ycc, s0.tables)


@pytest.mark.parametrize("bits", [32, 0], ids=["S32", "default"])
def test_batch_with_split_on_equals_host(ctx, reference, bits):
    with split_on(ctx, 1, bits):
        for s in sc.ALL:                                     # alone
            got, status = batch(ctx, [s])
            assert status == [_lib.OK] and got[0].tobytes() == reference[s.id], s.id
        ctx.enable_kernel_timing(True)
        try:
            for g in groups():                               # all that one call can hold together
                ctx.kernel_timings()
                got, status = batch(ctx, g)
                assert [k for _, k in ctx.kernel_timings()] == [K18A, K18B, 37, 38]      # no 36
                assert status == [_lib.OK] * len(g)
                for s, px in zip(g, got):
                    assert px.tobytes() == reference[s.id], s.id
        finally:
            ctx.enable_kernel_timing(False)
    assert sum(len(g) for g in groups()) == len(sc.ALL) and max(len(g) for g in groups()) >= 10


def interval_lengths(data):
    """The entropy-coded bytes of every restart interval of a stream."""
    first, end = sc.entropy_span(data)
    body, out, start, p = data[first:end], [], 0, 0
    while True:
        p = body.find(b"\xff", p)
        if p < 0:
            out.append(len(body) - start)
            return out
        if 0xD0 <= body[p + 1] <= 0xD7:
            out.append(p - start)
            start = p + 2
        p += 2


def test_threshold_between_interval_sizes_launches_both(ctx, reference):
    s = sc.split_stream("noise420_rst")
    lens = interval_lengths(s.data)
    assert len(lens) == 4 and min(lens) < max(lens) and min(lens) > 4096
    ctx.enable_kernel_timing(True)
    try:
        for threshold, kinds in ((max(lens), [36, K18A, K18B, 37, 38]), (max(lens) + 1, [36, 37, 38]), (min(lens), [K18A, K18B, 37, 38])):
            with split_on(ctx, threshold):
                ctx.kernel_timings()
                got, status = batch(ctx, [s, s])
                seen = [k for _, k in ctx.kernel_timings()]
            assert status == [_lib.OK] * 2 and got[0].tobytes() == reference[s.id] and got[1].tobytes() == reference[s.id]
            assert seen == kinds, (threshold, seen)
    finally:
        ctx.enable_kernel_timing(False)


def test_damaged_streams_between_good_ones(ctx, reference):
    s = sc.split_stream("noise422")
    first, end = sc.entropy_span(s.data)
    flipped = bytearray(s.data)
    flipped[(first + end) // 2] ^= 0x10
    cut = s.data[:(first + end) // 2] + b"\xff\xd9"          # the interval runs out of bits
    surplus = s.data[:end] + b"\0\0" + s.data[end:]
    streams = [s.data, jc.with_undefined_code(s.data), s.data, bytes(flipped), cut, s.data[:len(s.data) // 2], surplus, s.data]
    want = [sc.serial(s, d) for d in streams]
    assert [w[0] for w in want[:3]] == [_lib.OK, _lib.INTERNAL, _lib.OK] and want[4][0] == want[5][0] == _lib.INTERNAL
    assert want[6] == (_lib.OK, reference[s.id])
    for bits in (32, 0):
        with split_on(ctx, 1, bits):
            got, status = omr.jpeg_decode_batch_device(ctx, streams, [(s.w, s.h)] * len(streams), s.n, s.ycc, None)
        assert status == [w[0] for w in want], bits
        for g, w in zip(got, want):
            if w[0] == _lib.OK:
                assert g.tobytes() == w[1]


def test_set_jpeg_split_arguments(ctx):
    for bits in (16, 48, 4128, 31):
        with pytest.raises(omr.OmrError) as e:
            ctx.set_jpeg_split(1, bits)
        assert e.value.status == _lib.INVALID_ARGUMENT
    short = _lib.JpegSplitOptions(8, 1, 0)
    assert _lib.lib.omr_ctx_set_jpeg_split(ctx.h, _lib.ctypes.byref(short)) == _lib.INVALID_ARGUMENT
    assert _lib.lib.omr_ctx_set_jpeg_split(None, None) == _lib.INVALID_ARGUMENT
    for bits in (32, 4096, 0):
        ctx.set_jpeg_split(1, bits)
    ctx.set_jpeg_split(0)


@pytest.mark.parametrize("name", jc.NAMES)
def test_read_regions_with_split_on_equal_get_tile(ctx, tmp_path, name):
    px = jc.pixels(name)
    n, H, W = px.shape
    with omr.TiffImage(jc.write(tmp_path, name), 1, n, 1, accept=jc.ACCEPT) as img:
        for bits in (32, 0):
            with split_on(ctx, 1, bits):
                got = read_checked(ctx, img, 0, [(0, c, 0, 0, 0) for c in range(n)], W, H)
                part = read_checked(ctx, img, 0, [(0, n - 1, 0, 30, 10)], 37, 29)
            for c in range(n):
                assert got[c].tobytes() == img.get_tile(0, 0, c, 0, 0, 0, W, H).tobytes() == px[c].tobytes(), (bits, c)
            assert part[0].tobytes() == img.get_tile(0, 0, n - 1, 0, 30, 10, 37, 29).tobytes()


def test_kinds_without_the_setting_and_after_clearing_it(tmp_path):
    """A context that never makes the call, and one that made and cleared it, launch K17a."""
    name = "ycc422_tiles"
    px = jc.pixels(name)
    with omr.Context(0) as fresh, omr.TiffImage(jc.write(tmp_path, name), 1, 3, 1, accept=jc.ACCEPT) as img:
        fresh.enable_kernel_timing(True)
        for step in ("never", "on", "cleared"):
            if step == "on":
                fresh.set_jpeg_split(1)
            elif step == "cleared":
                assert _lib.lib.omr_ctx_set_jpeg_split(fresh.h, None) == _lib.OK
            fresh.kernel_timings()
            got = read_checked(fresh, img, 0, [(0, c, 0, 0, 0) for c in range(3)], 150, 70)
            kinds = [k for _, k in fresh.kernel_timings()]
            assert kinds == ([K18A, K18B, 37, 38, 31] if step == "on" else [36, 37, 38, 31]), (step, kinds)
            for c in range(3):
                assert got[c].tobytes() == px[c].tobytes(), (step, c)


def test_render_tiles_with_split_on_equals_off(ctx, tmp_path):
    qdef, chans = make_qdef("rgb"), rgb_bindings()
    with omr.TiffImage(jc.write(tmp_path, "ycc420_tiles_shared"), 1, 3, 1, accept=jc.ACCEPT) as img:
        ref = img.render_tiles(ctx, qdef, chans, 0, REQS, 64, 64)
        for bits in (32, 0):
            with split_on(ctx, 1, bits):
                got = img.render_tiles(ctx, qdef, chans, 0, REQS, 64, 64)
            assert np.array_equal(got, ref), bits
        assert len(np.unique(ref)) > 100                      # a picture, not a constant
