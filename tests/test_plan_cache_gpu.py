"""The context's device cache of staged render settings (plan cache): a request whose settings a
slot already holds launches no staging copy and no table build in front of K2.  Hits and misses
are read through omr_debug_plan_cache_stats; every result is diff 0 against the CPU restatement
(JPEG bytes: against a context created with OMR_PLAN_CACHE=0).  Run with OMR_PLAN_CACHE=0 in the
environment the results are checked alone."""
import ctypes
import os

import numpy as np
import pytest

import oracle_lib as O
from omr import _lib
from omr.synthetic import c2_channels, c5_channels, c5_planes

from k2_cases import I16, U16, channels, context_with, expected, render, tiles

pytestmark = pytest.mark.gpu

COUNTS = os.environ.get("OMR_PLAN_CACHE", "1") != "0"
Q = O.make_qdef("rgb")


def stats(ctx):
    h, m = ctypes.c_uint64(), ctypes.c_uint64()
    assert _lib.lib.omr_debug_plan_cache_stats(ctx.h, ctypes.byref(h), ctypes.byref(m)) == 0
    return h.value, m.value


def expect_counts(ctx, hits, misses):
    if COUNTS:
        assert stats(ctx) == (hits, misses)


def planes_of(pt, na, h=40, w=96, seed=7):
    dt = {_lib.PIXELS_UINT8: np.uint8, _lib.PIXELS_INT8: np.int8, U16: np.uint16, I16: np.int16}[pt]
    i = np.iinfo(dt)
    rng = np.random.default_rng(seed)
    return [rng.integers(i.min, int(i.max) + 1, (h, w)).astype(dt) for _ in range(na)]


def render_one(ctx, chans, planes, pt, qdef=Q, **kw):
    """One tile through the host API (small launch; the plane-pointer table is staged per call)
    and its restatement."""
    h, w = planes[0].shape
    got = ctx.render_packed_int(qdef, chans, planes, pt, w, h, **kw)
    st, exp = O.render(chans, planes, pt, w, h, qdef=qdef, **kw)
    assert st == 0
    np.testing.assert_array_equal(got, exp)


def test_same_settings_hit():
    chans, planes = c2_channels(4), planes_of(U16, 4)
    with context_with() as ctx:
        render_one(ctx, chans, planes, U16)
        expect_counts(ctx, 0, 1)
        render_one(ctx, chans, planes_of(U16, 4, seed=8), U16, flip_h=True)   # other pixels, same settings
        expect_counts(ctx, 1, 1)


def test_window_change_misses_and_back_hits():
    a, b = c2_channels(3), c2_channels(3)
    b[1]["input_end"] = 51198.0
    planes = planes_of(U16, 3)
    with context_with() as ctx:
        render_one(ctx, a, planes, U16)
        render_one(ctx, b, planes, U16)
        expect_counts(ctx, 0, 2)
        render_one(ctx, a, planes, U16)
        expect_counts(ctx, 1, 2)


@pytest.mark.parametrize("pts", [(_lib.PIXELS_UINT8, _lib.PIXELS_INT8), (U16, I16)], ids=["8", "16"])
def test_pixel_type_is_part_of_the_key(pts):
    chans = [{"active": True, "input_start": 10.0, "input_end": 100.0, "global_min": -32768.0,
              "global_max": 65535.0, "rgba": (255, 128, 0, 255)}]
    with context_with() as ctx:
        for i, pt in enumerate(pts):
            render_one(ctx, chans, planes_of(pt, 1), pt)
            expect_counts(ctx, 0, i + 1)


def test_eviction_round_robin():
    settings = []
    for k in range(3):
        c = c2_channels(2)
        c[0]["input_start"] = float(100 * (k + 1))
        settings.append(c)
    planes = planes_of(U16, 2)
    with context_with(OMR_PLAN_CACHE_SLOTS="2") as ctx:
        for rnd in range(2):
            for k, c in enumerate(settings):
                render_one(ctx, c, planes, U16)
                expect_counts(ctx, 0, 3 * rnd + k + 1)      # two slots, three settings: never a hit


def test_small_then_full_launch_share_a_slot():
    """One tile builds its contributions in LDS from the slot's plan; 64 tiles (the full launch)
    then read the table K1 left in the slot on the miss."""
    chans = channels(U16, [(1755, 51199), (100, 4000)])
    chans[0]["reverse"] = True
    host = tiles(U16, True, 64, 2)
    with context_with() as ctx:
        for i, n in enumerate((1, 64)):
            got = render(ctx, host[:n], U16, True, chans, 256, 256, fh=True)
            np.testing.assert_array_equal(got, expected(host[:n], U16, True, chans, 256, 256, fh=True))
            expect_counts(ctx, i, 1)


def test_float_threshold_tables_come_from_the_slot():
    rng = np.random.default_rng(5)
    planes = c5_planes(64, 64, rng)
    chans = c5_channels(planes)
    with context_with() as ctx:
        for i in range(2):
            render_one(ctx, chans, planes, _lib.PIXELS_FLOAT)
            expect_counts(ctx, i, 1)


def test_lut_colour_and_reverse():
    chans = c2_channels(2)
    chans[0]["lut"] = np.stack([np.arange(256), 255 - np.arange(256), np.arange(256) // 2], -1).astype(np.uint8)
    chans[1]["reverse"] = True
    planes = planes_of(U16, 2)
    with context_with() as ctx:
        for i in range(2):
            render_one(ctx, chans, planes, U16)
            expect_counts(ctx, i, 1)
        other = [dict(c) for c in chans]
        other[0]["lut"] = chans[0]["lut"][::-1].copy()      # the colour table is part of the key
        render_one(ctx, other, planes, U16)
        expect_counts(ctx, 1, 2)


def test_semantics_flag_is_part_of_the_key():
    chans = c2_channels(2)
    chans[0]["rgba"] = (10, 200, 90, 128)
    planes = planes_of(U16, 2)
    with context_with() as ctx:
        for i, flags in enumerate((0, _lib.SEM_ALPHA_SEPARATE, 0)):
            ctx.set_semantics(flags)
            with O.semantics(flags):
                render_one(ctx, chans, planes, U16)
        expect_counts(ctx, 1, 2)


def test_workspace_reallocation_keeps_the_slots():
    chans, planes = c2_channels(2), planes_of(U16, 2)
    with context_with() as ctx:
        render_one(ctx, chans, planes, U16)
        big = [np.random.default_rng(3).integers(0, 65536, (1024, 1024)).astype(np.uint16)]
        render_one(ctx, c2_channels(1), big, U16)            # 6 MiB of planes + output: the arena grows
        expect_counts(ctx, 0, 2)
        render_one(ctx, chans, planes, U16)
        expect_counts(ctx, 1, 2)


def test_stream_change_empties_the_cache():
    import torch
    chans, planes = c2_channels(2), planes_of(U16, 2)
    s2 = torch.cuda.Stream()
    with context_with() as ctx:
        render_one(ctx, chans, planes, U16)
        ctx.set_stream(s2.cuda_stream)
        render_one(ctx, chans, planes, U16)
        ctx.set_stream(None)
        render_one(ctx, chans, planes, U16)
        expect_counts(ctx, 0, 3)
        ctx.set_stream(None)                                  # no change: the cache stays
        render_one(ctx, chans, planes, U16)
        expect_counts(ctx, 1, 3)


def _jpeg_batch(ctx, host, chans, w, h, quality=0.9):
    import torch
    n, na = host.shape[:2]
    data = torch.from_numpy(np.ascontiguousarray(host).view(np.uint8).reshape(-1).copy()).to("cuda")
    d_out = torch.empty(n * (w * h * 4 + 4096), dtype=torch.uint8, device="cuda")
    offs = torch.empty(n, dtype=torch.int64, device="cuda")
    lens = torch.empty(n, dtype=torch.int32, device="cuda")
    stat = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    pb = h * w * 2
    ctx.render_jpeg_batch_strided_device(Q, chans, data, na * pb, pb, n, U16, w, h, quality, d_out, offs, lens, stat,
                                         big_endian=True)
    ctx.synchronize()
    o, ln, buf = offs.cpu().numpy(), lens.cpu().numpy(), d_out.cpu().numpy()
    assert (stat.cpu().numpy() == 0).all()
    return [buf[o[i]:o[i] + ln[i]].tobytes() for i in range(n)]


@pytest.mark.parametrize("plain_first", [True, False], ids=["render-then-jpeg", "jpeg-then-render"])
def test_fused_jpeg_shares_the_slot(plain_first):
    """A fused render -> JPEG and a plain render of one setting use one slot (the fused kernel's
    int16 bias moves kernel arguments, not the staged plan)."""
    w = h = 64
    chans = channels(U16, [(1755, 51199), (3218, 26623), (100, 4000)])
    host = tiles(U16, True, 2, 3, h=h, w=w)
    with context_with(OMR_PLAN_CACHE="0") as ref:
        want = _jpeg_batch(ref, host, chans, w, h)
    exp = expected(host, U16, True, chans, w, h)
    assert want == [O.encode_jpeg(exp[i], w, h, 0.9) for i in range(2)]
    with context_with() as ctx:
        for i, plain in enumerate((plain_first, not plain_first)):
            if plain:
                np.testing.assert_array_equal(render(ctx, host, U16, True, chans, w, h), exp)
            else:
                assert _jpeg_batch(ctx, host, chans, w, h) == want
            expect_counts(ctx, i, 1)


def test_byte_lut_evicted_between_uses():
    """Non-linear u16 settings read a 64 KiB byte LUT from the context's LUT cache; with a 64 KiB
    budget two settings evict each other's LUT, which is rebuilt (perhaps elsewhere) between two
    uses of a plan-cached setting.  The LUT's address is inside the plan bytes."""
    settings = []
    for k in range(2):
        c = c2_channels(2)
        c[0].update(family=_lib.FAMILY_LOGARITHMIC, input_start=float(50 + 400 * k))
        c[1].update(family=_lib.FAMILY_POLYNOMIAL, coefficient=2.0)
        settings.append(c)
    planes = planes_of(U16, 2)
    with context_with(OMR_LUT_CACHE_KB="64") as ctx:
        for rnd in range(3):
            for c in settings:
                render_one(ctx, c, planes, U16)
