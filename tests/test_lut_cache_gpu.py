"""The context's device cache of kModeLut16 byte LUTs (non-linear 16-bit families and noise
reduction, omr_render.hip device_quant_lut): every request is still bit-exact against the CPU
restatement when settings repeat (hits), when more settings pass through one context than the
cache holds (LRU eviction, kDevLutEntries = 64), and for LUT domains wider than the pixel type
(globalMin / globalMax beyond 0..65535: up to 2^24 entries, built once per setting).

A plan's own LUTs stay resident while it is prepared (omr_lut_policy.h): plans that need more
LUT bytes than the budget (OMR_LUT_CACHE_KB, read at context creation) overshoot it instead of
freeing a LUT an earlier channel of the same plan was given -- through K2, the fused render ->
JPEG kernel (F1) and the fused projection glue (K3R), which all read ChanParam::lut_addr -- and
eighteen LUTs of nearly 2^24 entries (288 MiB) in one plan against the 256 MiB default."""
import numpy as np
import pytest

import oracle_lib as O
from omr import _lib
from omr.renderer import f32
from omr.synthetic import c2_channels, tile_u16

pytestmark = pytest.mark.gpu


def _render(ctx, chans, planes, w, h):
    return ctx.render_packed_int(O.make_qdef("rgb"), chans, planes, _lib.PIXELS_UINT16, w, h)


def test_lut_cache_hits_and_eviction(ctx):
    h, w = 32, 48
    planes = tile_u16(21, 2, h, w, uniform=True)
    base = c2_channels(2)
    settings = []
    for i in range(80):                       # > kDevLutEntries distinct non-linear settings
        chans = [dict(c) for c in base]
        chans[0]["family"] = _lib.FAMILY_POLYNOMIAL
        chans[0]["coefficient"] = 0.5 + i / 40.0
        chans[1]["family"] = _lib.FAMILY_LOGARITHMIC if i % 2 else _lib.FAMILY_EXPONENTIAL
        chans[1]["coefficient"] = 0.25 + (i % 7) / 10.0
        chans[1]["input_start"], chans[1]["input_end"] = 1.0 + i, 3000.0 + 97 * i
        settings.append(chans)
    exp = []
    for chans in settings:
        st, e = O.render(chans, planes, _lib.PIXELS_UINT16, w, h)
        assert st == 0
        exp.append(e)
    for rep in range(2):                      # first pass fills and evicts; second re-builds / hits
        for i in (list(range(80)) if rep == 0 else [79, 78, 0, 1, 40, 79, 0]):
            np.testing.assert_array_equal(_render(ctx, settings[i], planes, w, h), exp[i], err_msg=f"setting {i}")


@pytest.mark.parametrize("gmin,gmax", [(-100000.0, 100000.0), (-5.0, 70000.0), (0.0, 65535.0)])
def test_lut_wide_domains(ctx, gmin, gmax):
    h, w = 24, 40
    planes = tile_u16(22, 2, h, w, uniform=True)
    chans = c2_channels(2)
    for c in chans:
        c["global_min"], c["global_max"] = gmin, gmax
    chans[0]["family"] = _lib.FAMILY_POLYNOMIAL
    chans[0]["coefficient"] = 1.7
    chans[1]["noise_reduction"] = True
    for _ in range(2):                        # miss, then hit
        st, exp = O.render(chans, planes, _lib.PIXELS_UINT16, w, h)
        assert st == 0
        np.testing.assert_array_equal(_render(ctx, chans, planes, w, h), exp)


# ---- plans whose LUTs pass the cache's byte budget -------------------------------------------
H, W = 24, 40
_FAMS = [_lib.FAMILY_POLYNOMIAL, _lib.FAMILY_LOGARITHMIC, _lib.FAMILY_EXPONENTIAL, _lib.FAMILY_LINEAR]


def _lut_plan(n, salt, cmax=64):
    """n kModeLut16 channels (polynomial, logarithmic, exponential, linear with noise reduction),
    each with a window and coefficient of its own -- so a LUT of its own, monotone (window start
    and coefficient above 0), and no LUT shared between plans of different salt.  Colour
    components in [4, 4 + cmax): small enough that the sum rarely saturates and a wrong LUT in
    any channel shows."""
    chans = []
    for i in range(n):
        fam = _FAMS[(i + salt) % 4]
        c = {"active": True, "input_start": f32(1.0 + 211 * i + 17 * salt),
             "input_end": f32(21000.0 + 2300 * i + 101 * salt), "global_min": 0.0, "global_max": 65535.0,
             "rgba": (4 + 37 * (i + salt) % cmax, 4 + 23 * (i + 2 * salt) % cmax, 4 + 51 * (i + 3) % cmax, 255)}
        if fam == _lib.FAMILY_LINEAR:
            c["noise_reduction"] = True
        else:
            c["family"] = fam
            c["coefficient"] = 0.3 + 0.005 * i if fam == _lib.FAMILY_EXPONENTIAL else 0.6 + 0.11 * i + 0.03 * salt
        chans.append(c)
    return chans


def _own_ctx(monkeypatch, kb, k3r=False):
    """A context of the test's own: the LUT budget (and OMR_K3R) are read at context creation."""
    import torch  # noqa: F401  (initialises the HIP runtime once)
    import omr
    if kb is None:
        monkeypatch.delenv("OMR_LUT_CACHE_KB", raising=False)
    else:
        monkeypatch.setenv("OMR_LUT_CACHE_KB", str(kb))
    if k3r:
        monkeypatch.setenv("OMR_K3R", "1")
    return omr.Context(0)


def test_plan_larger_than_the_budget(monkeypatch):
    """Six 64 KiB LUTs per plan against a 256 KiB budget: the fifth and sixth miss find only the
    plan's own entries to evict.  Twice (misses, then hits), then alternating with a second
    six-LUT plan, so each plan's entries are evicted between its calls."""
    planes = tile_u16(31, 6, H, W, uniform=True)
    plans = [_lut_plan(6, 0), _lut_plan(6, 5)]
    exp = []
    for chans in plans:
        st, e = O.render(chans, planes, _lib.PIXELS_UINT16, W, H)
        assert st == 0
        exp.append(e)
    assert not np.array_equal(exp[0], exp[1])
    c = _own_ctx(monkeypatch, 256)
    try:
        for call, which in enumerate((0, 0, 1, 0, 1, 0, 1, 0)):
            np.testing.assert_array_equal(_render(c, plans[which], planes, W, H), exp[which], err_msg=f"call {call}")
    finally:
        c.close()


@pytest.mark.parametrize("consumer", ["k2", "jpeg_24x40", "jpeg_f1_32x48", "k3r"])
def test_every_reader_of_lut_addr_with_a_plan_past_the_budget(monkeypatch, consumer):
    """Four LUTs per plan against 128 KiB (two LUTs), through each kernel that reads lut_addr:
    K2 (the 4-channel instantiation), the render -> JPEG batch (24x40 tiles take K2 + the batched
    encoder; F1 needs sides that are multiples of 16, so it runs at 32x48) and the fused
    projection glue K3R (OMR_K3R=1).  A second plan in between evicts the first one's LUTs."""
    from test_project_gpu import _glue
    from test_render_jpeg_gpu import _expect, _run
    plans = [_lut_plan(4, 1), _lut_plan(4, 6)]
    order = (0, 0, 1, 0)
    pt = _lib.PIXELS_UINT16
    c = _own_ctx(monkeypatch, 128, k3r=consumer == "k3r")
    try:
        if consumer == "k2":
            planes = tile_u16(32, 4, H, W, uniform=True)
            for which in order:
                st, exp = O.render(plans[which], planes, pt, W, H)
                assert st == 0
                np.testing.assert_array_equal(_render(c, plans[which], planes, W, H), exp)
        elif consumer.startswith("jpeg"):
            h, w = (32, 48) if consumer == "jpeg_f1_32x48" else (H, W)
            tiles = [tile_u16(40 + t, 4, h, w, uniform=True) for t in range(2)]
            for which in order:
                files, st = _run(c, plans[which], tiles, pt, w, h)
                assert (st == 0).all()
                assert files == _expect(plans[which], tiles, pt, w, h)
        else:
            rng = np.random.default_rng(34)
            stacks = [rng.integers(0, 65536, (5, H, W)).astype(np.uint16) for _ in range(4)]
            for which, alg in zip(order, (_lib.PROJECTION_MAX, _lib.PROJECTION_MEAN, _lib.PROJECTION_MAX,
                                          _lib.PROJECTION_MEAN)):
                _glue(c, plans[which], stacks, pt, W, H, 5, alg, 0, 4)
    finally:
        c.close()


def test_eighteen_wide_domain_luts_in_one_plan(monkeypatch):
    """Real size, default budget: 18 channels whose LUT domains are [-8388608 + i, 8388607] --
    2^24 - i entries each, 288 MiB against 256 MiB -- so the seventeenth miss finds nothing but
    the plan's own LUTs to evict.  In-range pixels render as with the 0..65535 domain."""
    n = 18
    planes = tile_u16(33, n, H, W, uniform=True)
    narrow = _lut_plan(n, 2, cmax=14)
    chans = [dict(c) for c in narrow]
    for i, c in enumerate(chans):
        c["global_min"], c["global_max"] = -8388608.0 + i, 8388607.0
    st, exp = O.render(chans, planes, _lib.PIXELS_UINT16, W, H)
    assert st == 0
    st, exp_narrow = O.render(narrow, planes, _lib.PIXELS_UINT16, W, H)
    assert st == 0
    np.testing.assert_array_equal(exp, exp_narrow)
    assert (exp.view(np.uint8).reshape(H, W, 4)[..., :3] == 255).mean() < 0.1      # a wrong LUT shows
    c = _own_ctx(monkeypatch, None)
    try:
        for rep in range(2):                     # misses with the overshoot, then hits
            np.testing.assert_array_equal(_render(c, chans, planes, W, H), exp, err_msg=f"pass {rep}")
    finally:
        c.close()
