"""Renders with 5..32 active channels against the CPU restatement, asserted equal.

Above four active channels K2 runs its runtime-channel-count form (k_render<..., NA = 0, ...>):
one chunk per lane, pixels loaded channel by channel, and the 10-bit packed accumulator fields
clamped after every add.  Float and 32-bit threshold channels get the half-size bucket table
(1,024 buckets) up to kMaxThreshActive = 8 channels and are demoted to per-pixel evaluation above.
Every K2 mode of that form is pinned here -- Table8, Fast16, Linear16, Mixed16, Thresh, Eval -- for
every pixel type and byte order, with inactive bindings interleaved (so a channel's plane index
differs from its slot), both vector forms (width 40 and 37), the four flips, sums that overflow
a colour component at some pixels only, every render entry point, the 32 / 33 channel limit and
the encoder and projection fallbacks at the 4 -> 5 boundary.

Exactness: 8/16-bit types and threshold channels quantize through host-built tables, so every
family is exact; float and 32-bit channels that are evaluated per pixel (window not monotone, or
more than 8 channels) use the linear family, which is exact in double.  Only the random sweep at
the end draws non-linear families for evaluated channels and keeps test_render_sweep's bar."""
import numpy as np
import pytest

import oracle_lib as O
from omr import _lib
from omr.context import make_qdef
from omr.renderer import f32
from test_render_sweep_gpu import TYPES, _config, _planes, _range

pytestmark = pytest.mark.gpu

H = 24
WIDTHS = (40, 37)                     # a multiple of the vector width, and an odd one (VEC = 1)
FLIPS = [(False, False), (True, False), (False, True), (True, True)]
NAS = [5, 8, 9, 16, 32]
PT_NAME = {_lib.PIXELS_UINT8: "u8", _lib.PIXELS_INT8: "i8", _lib.PIXELS_UINT16: "u16", _lib.PIXELS_INT16: "i16",
           _lib.PIXELS_UINT32: "u32", _lib.PIXELS_INT32: "i32", _lib.PIXELS_FLOAT: "f32"}
DTYPE = dict(TYPES)
LUT = np.concatenate([np.arange(256), 255 - np.arange(256), (np.arange(256) * 3) % 256]).astype(np.uint8)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to("cuda")


def _be(planes, be):
    return [p.astype(p.dtype.newbyteorder(">")) if be and p.dtype.itemsize > 1 else p for p in planes]


def _colour(i, na):
    """Components around 400 / na: sums reach 255 at some pixels, not everywhere."""
    base = max(6, 400 // na)
    return (base + 7 * i % 23, base + 11 * i % 19, base + 5 * i % 29, 255 if i % 4 else 160)


def _window(dtype, i, kind):
    lo, hi = _range(dtype)
    span = hi - lo
    a, b = lo + span * (0.05 + 0.04 * (i % 10)), hi - span * (0.03 + 0.05 * (i % 7))
    if kind == "inverted":
        return b, a
    if kind == "empty":
        return a, a
    if kind == "beyond":
        return lo - 0.3 * span, hi + 0.2 * span
    return a, b


def _chan(dtype, i, na, kind="ordinary", **kw):
    ws, we = _window(dtype, i, kind)
    c = {"active": True, "input_start": f32(ws), "input_end": f32(we), "rgba": _colour(i, na)}
    if dtype != np.float32:
        c["global_min"], c["global_max"] = _range(dtype)
    c.update(kw)
    return c


def _spread(active):
    """Bindings with an inactive one before every third active channel: size_c > n_active and
    K2Chan::index differs from the slot.  The inactive copy is white, so rendering it shows."""
    chans = []
    for i, c in enumerate(active):
        if i % 3 == 0:
            chans.append(dict(c, active=False, rgba=(255, 255, 255, 255)))
        chans.append(c)
    return chans


def _check(ctx, chans, planes, pt, w, be=False, flip=(False, False), qdef=None):
    q = qdef or make_qdef("rgb")
    src = _be(planes, be)
    st, exp = O.render(chans, src, pt, w, H, big_endian=be, flip_h=flip[0], flip_v=flip[1], qdef=q)
    assert st == 0
    got = ctx.render_packed_int(q, chans, src, pt, w, H, big_endian=be, flip_h=flip[0], flip_v=flip[1])
    np.testing.assert_array_equal(got, exp)
    return exp


# ---- every pixel type and channel count, linear windows of every kind --------------------------
@pytest.mark.parametrize("na", NAS)
@pytest.mark.parametrize("pt", [t for t, _ in TYPES], ids=lambda t: PT_NAME[t])
def test_linear_windows_every_type_and_count(ctx, pt, na):
    """Ordinary, inverted, empty and beyond-range linear windows.  8-bit: Table8.  16-bit:
    Linear16 (an inverted window is not Fast16).  Float / 32-bit: 5 and 8 channels mix threshold
    channels with evaluated ones (an inverted or empty window is not monotone); 9, 16 and 32 demote
    every threshold channel to evaluation."""
    dtype = DTYPE[pt]
    case = NAS.index(na) + 5 * [t for t, _ in TYPES].index(pt)
    kinds = ["ordinary", "inverted", "beyond", "empty", "ordinary"]
    active = [_chan(dtype, i, na, kinds[i % 5], reverse=i == 1, **({"lut": LUT} if i == 2 else {}))
              for i in range(na)]
    chans = _spread(active)
    rng = np.random.default_rng(900 + case)
    w = WIDTHS[case % 2]
    planes = _planes(rng, dtype, len(chans), H, w)
    _check(ctx, chans, planes, pt, w, be=case % 3 == 1, flip=FLIPS[case % 4])


# ---- the 16-bit kernel modes at NA = 0 ----------------------------------------------------------
@pytest.mark.parametrize("na", NAS)
@pytest.mark.parametrize("pt", [_lib.PIXELS_UINT16, _lib.PIXELS_INT16], ids=lambda t: PT_NAME[t])
@pytest.mark.parametrize("mode", ["fast16", "linear16", "mixed16"])
def test_16bit_modes(ctx, mode, pt, na):
    """Fast16: every channel linear with an increasing window and the default codomain.
    Linear16: the same under cd_start = 10, cd_end = 200.  Mixed16: linear channels next to
    polynomial, logarithmic, exponential and noise-reduction ones (byte LUTs of the context's
    cache).  One channel reversed, one with a .lut colour table."""
    dtype = DTYPE[pt]
    case = NAS.index(na) + 5 * (pt == _lib.PIXELS_INT16) + 10 * ["fast16", "linear16", "mixed16"].index(mode)
    active = [_chan(dtype, i, na, reverse=i == 1, **({"lut": LUT} if i == 3 else {})) for i in range(na)]
    if mode == "mixed16":
        for i, c in enumerate(active):
            if i % 5 == 1:
                c.update(family=_lib.FAMILY_POLYNOMIAL, coefficient=0.5 + 0.25 * (i % 4))
            elif i % 5 == 2:
                c.update(family=_lib.FAMILY_LOGARITHMIC)
            elif i % 5 == 3:
                c.update(family=_lib.FAMILY_EXPONENTIAL, coefficient=0.3)
            elif i % 5 == 4:
                c.update(noise_reduction=True)
    q = make_qdef("rgb", cd_start=10, cd_end=200) if mode == "linear16" else make_qdef("rgb")
    chans = _spread(active)
    rng = np.random.default_rng(1000 + case)
    w = WIDTHS[(case + na) % 2]
    planes = _planes(rng, dtype, len(chans), H, w)
    _check(ctx, chans, planes, pt, w, be=case % 2 == 0, flip=FLIPS[(case + 1) % 4], qdef=q)


# ---- float / 32-bit threshold channels at 5 and 8 (1,024 buckets per channel) -------------------
# windows a few hundred keys wide (about one threshold per key: buckets of one), narrower than
# 255 keys (several thresholds on one key), and spanning most of the type (most buckets empty)
THRESH_WINDOWS = {
    _lib.PIXELS_FLOAT: [(1.0, 1.0000358), (2.0, 2.000012), (1e-3, 3e38), (0.5, 60000.0), (100.0, 101.0),
                        (-300.0, 900.0), (3.0, 3.0e9), (1e-30, 1e-20)],
    _lib.PIXELS_UINT32: [(1000.0, 1300.0), (500.0, 600.0), (1e6, 4e9), (10.0, 70000.0), (2e9, 2.0000003e9),
                         (0.0, 4294967295.0), (7.0, 3.0e9), (123456.0, 123999.0)],
    _lib.PIXELS_INT32: [(-150.0, 150.0), (5.0, 60.0), (3.0, 2.0e9), (10.0, 70000.0), (-1e9, -9.99999e8),
                        (-2147483648.0, 2147483647.0), (-2e9, 2e9), (123456.0, 123999.0)],
}
# families for the windows that start above 0 (monotone: host-built thresholds, exact)
THRESH_FAMILIES = [None, (_lib.FAMILY_LOGARITHMIC, 1.0), (_lib.FAMILY_POLYNOMIAL, 0.5), (_lib.FAMILY_EXPONENTIAL, 0.2),
                   (_lib.FAMILY_POLYNOMIAL, 2.0), None, (_lib.FAMILY_LOGARITHMIC, 1.0), None]


def _thresh_chan(pt, i, na):
    ws, we = THRESH_WINDOWS[pt][i]
    c = {"active": True, "input_start": f32(ws), "input_end": f32(we), "rgba": _colour(i, na), "reverse": i == 4}
    if THRESH_FAMILIES[i] and ws > 0:
        c["family"], c["coefficient"] = THRESH_FAMILIES[i]
    if i == 5:
        c["noise_reduction"] = True
    return c


def _keys_to_values(keys, dtype):
    """Pixel values of K2's ordered 32-bit keys (host_key_value in omr_render.hip)."""
    k = np.asarray(keys, dtype=np.int64).astype(np.uint32)
    if dtype == np.float32:
        return np.where(k & 0x80000000, k & 0x7FFFFFFF, ~k).astype(np.uint32).view(np.float32)
    if dtype == np.int32:
        return (k ^ np.uint32(0x80000000)).view(np.int32)
    return k


def _code_edges(ch, pt, dtype):
    """The pixel values at which a monotone channel's code steps, from the restatement alone: for
    every code c the smallest key whose code is >= c (bisection over the type's whole key range,
    all 255 codes at once through one-row renders), with the keys just below and above it.  These
    are the values a threshold table, a bucket's one-threshold offset or the in-bucket search
    gets wrong by one when a compare or a count is off."""
    solo = dict(ch, active=True, reverse=False)
    solo.pop("lut", None)
    q = make_qdef("greyscale")

    def codes(keys):
        vals = np.ascontiguousarray(_keys_to_values(keys, dtype)).reshape(1, -1)
        st, e = O.render([solo], [vals], pt, vals.shape[1], 1, qdef=q)
        assert st == 0
        return (e[0] & 0xFF).astype(np.int64)

    klo, khi = (0x007FFFFF, 0xFF800000) if dtype == np.float32 else (0, 2 ** 32 - 1)    # float: -inf .. +inf
    c = np.arange(1, 256)
    lo, hi = np.full(255, klo, np.int64), np.full(255, khi, np.int64)
    reached = codes(hi) >= c
    while (lo < hi).any():
        open_ = lo < hi
        mid = (lo + hi) // 2
        ge = codes(mid) >= c
        hi = np.where(open_ & ge, mid, hi)
        lo = np.where(open_ & ~ge, mid + 1, lo)
    t = np.unique(lo[reached])
    keys = np.unique(np.clip(np.concatenate([t - 1, t, t + 1]), klo, khi))
    return _keys_to_values(keys, dtype)


def _window_plane(rng, dtype, ws, we, w, edges=None):
    """A third of the pixels uniform over the window and a tenth beyond each end, a third
    log-uniform over it (uniform when it starts at or below 0), a third random bit patterns (float:
    NaNs, infinities, denormals, negatives), plus the ends and the float specials; then up to
    half of the plane is given to `edges` (_code_edges: every code boundary and its neighbours)."""
    n = H * w
    ws, we = float(f32(ws)), float(f32(we))
    span = we - ws
    x = rng.uniform(ws - 0.1 * span, we + 0.1 * span, n)
    third = n // 3
    if ws > 0:
        x[third:2 * third] = np.exp(rng.uniform(np.log(ws), np.log(we), third))
    if dtype == np.float32:
        out = x.astype(np.float32)
        out[2 * third:] = rng.integers(0, 2 ** 32, n - 2 * third, dtype=np.uint64).astype(np.uint32).view(np.float32)
        out[:8] = [np.nan, np.inf, -np.inf, -0.0, 0.0, -1.5, ws, we]
    else:
        info = np.iinfo(dtype)
        out = np.clip(np.floor(x), info.min, info.max).astype(np.int64)
        out[2 * third:] = rng.integers(info.min, int(info.max) + 1, n - 2 * third, dtype=np.int64)
        out[:4] = [info.min, info.max, int(np.clip(ws, info.min, info.max)), int(np.clip(we, info.min, info.max))]
        out = out.astype(dtype)
    if edges is not None and len(edges):
        k = min(len(edges), n // 2)
        out[8:8 + k] = edges if len(edges) == k else rng.choice(edges, k, replace=False)
    return rng.permutation(out).reshape(H, w)


@pytest.mark.parametrize("na", [5, 8])
@pytest.mark.parametrize("pt", [_lib.PIXELS_UINT32, _lib.PIXELS_INT32, _lib.PIXELS_FLOAT], ids=lambda t: PT_NAME[t])
@pytest.mark.parametrize("be", [False, True])
def test_all_threshold_plans(ctx, be, pt, na):
    """kK2Thresh at NA = 0: every channel monotone.  Eight channels take 49,280 bytes of LDS."""
    dtype = DTYPE[pt]
    active = [_thresh_chan(pt, i, na) for i in range(na)]
    chans = _spread(active)
    case = na + 2 * be + [_lib.PIXELS_UINT32, _lib.PIXELS_INT32, _lib.PIXELS_FLOAT].index(pt)
    rng = np.random.default_rng(1100 + case)
    w = WIDTHS[case % 2]
    planes = [_window_plane(rng, dtype, c["input_start"], c["input_end"], w,
                            edges=_code_edges(c, pt, dtype) if c["active"] else None) for c in chans]
    _check(ctx, chans, planes, pt, w, be=be, flip=FLIPS[case % 4])


@pytest.mark.parametrize("pt", [_lib.PIXELS_UINT32, _lib.PIXELS_INT32, _lib.PIXELS_FLOAT], ids=lambda t: PT_NAME[t])
def test_seven_threshold_channels_and_one_evaluated(ctx, pt):
    """kK2Eval with threshold tables staged: seven monotone channels and one linear channel whose
    inverted window fails monotone_q, so it is evaluated per pixel (exactly: linear in double)."""
    dtype = DTYPE[pt]
    active = [_thresh_chan(pt, i, 8) for i in range(7)]
    ws, we = THRESH_WINDOWS[pt][3]
    active.insert(4, {"active": True, "input_start": f32(we), "input_end": f32(ws), "rgba": _colour(9, 8)})
    chans = _spread(active)
    rng = np.random.default_rng(1200 + pt)
    edges = [_code_edges(c, pt, dtype) if c["active"] and c["input_start"] < c["input_end"] else None for c in chans]
    for w, be, flip in ((40, False, FLIPS[1]), (37, True, FLIPS[2])):
        planes = [_window_plane(rng, dtype, *sorted((c["input_start"], c["input_end"])), w, edges=e)
                  for c, e in zip(chans, edges)]
        _check(ctx, chans, planes, pt, w, be=be, flip=flip)


# ---- saturation: the clamp after every add ------------------------------------------------------
def _component_sums(chans, planes, pt, w):
    """Per active channel, the restatement's render of that channel alone: [n][H][w][3] (r, g, b)."""
    out = []
    for k, c in enumerate(chans):
        if not c["active"]:
            continue
        solo = [dict(x, active=(j == k)) for j, x in enumerate(chans)]
        st, e = O.render(solo, planes, pt, w, H)
        assert st == 0
        out.append(np.stack([(e >> 16) & 255, (e >> 8) & 255, e & 255], -1).astype(np.int64))
    return np.stack(out)


@pytest.mark.parametrize("na", [5, 8, 32])
@pytest.mark.parametrize("pt", [_lib.PIXELS_UINT8, _lib.PIXELS_UINT16, _lib.PIXELS_FLOAT], ids=lambda t: PT_NAME[t])
def test_component_overflow_at_some_pixels(ctx, pt, na):
    """Colours and windows under which each colour component overflows at some pixels and not
    at others.  The first four channels alone never reach 255 (their colours sum below it), so
    every overflow happens on the clamp-per-add path.  At 32 channels, 28 of them read copies of
    one plane and switch on together where it is above their (step) windows: the running sum of a
    component passes 1,023 -- the capacity of a 10-bit accumulator field -- before the last add.
    The conditions are asserted on the restatement's output, not on the kernel's."""
    dtype = DTYPE[pt]
    lo, hi = (0.0, 65535.0) if dtype == np.float32 else _range(dtype)
    span = hi - lo
    w = WIDTHS[na % 2]
    rng = np.random.default_rng(1300 + na + pt)
    gl = {} if dtype == np.float32 else {"global_min": lo, "global_max": hi}

    def plane():
        if dtype == np.float32:
            return rng.uniform(lo, hi, (H, w)).astype(np.float32)
        return rng.integers(int(lo), int(hi) + 1, (H, w)).astype(dtype)

    active = [dict(gl, active=True, input_start=f32(lo + 0.02 * span * i), input_end=f32(hi - 0.03 * span * i),
                   rgba=(60 - i, 50 + i, 40 + 2 * i, 255)) for i in range(4)]
    planes = [plane() for _ in range(4)]
    if na == 32:
        shared = plane()
        for i in range(4, 32):         # steps between the 62nd and 76th percentile of the shared plane
            ws = lo + span * (0.62 + 0.005 * (i - 4))
            active.append(dict(gl, active=True, input_start=f32(ws), input_end=f32(ws + span * 0.004),
                               rgba=(200 - i, 150 + i, 180 + i % 5, 255)))
            planes.append(shared.copy())
    else:
        late = {5: (255, 240, 225), 8: (75, 70, 65)}[na]
        for i in range(4, na):
            active.append(dict(gl, active=True, input_start=f32(lo + 0.01 * span * i), input_end=f32(hi - 0.02 * span * i),
                               rgba=(late[0] - i, late[1] - 2 * i, late[2] + i, 255), reverse=i % 2 == 1))
            planes.append(plane())
    exp = _check(ctx, active, planes, pt, w, flip=FLIPS[na % 4])
    rgb = np.stack([(exp >> 16) & 255, (exp >> 8) & 255, exp & 255], -1)
    frac = (rgb == 255).any(-1).mean()
    assert 0.10 <= frac <= 0.90, f"{frac:.2f} of the pixels saturate"
    for k in range(3):
        assert 0 < (rgb[..., k] == 255).sum() < rgb[..., k].size, f"component {k}"
    solo = _component_sums(active, planes, pt, w)
    assert solo[:4].sum(0).max() < 255                       # the first four never reach 255 alone
    assert (solo.sum(0) > 255).any(-1).mean() >= 0.10         # the clamp is what holds 255
    if na == 32:
        assert (np.cumsum(solo, 0)[-2] > 1023).all(-1).any()  # past a 10-bit field before the last add


# ---- entry points -------------------------------------------------------------------------------
@pytest.mark.parametrize("pt,na,be", [(_lib.PIXELS_UINT16, 8, True), (_lib.PIXELS_INT16, 9, False),
                                      (_lib.PIXELS_UINT8, 16, False)], ids=["u16be-8", "i16-9", "u8-16"])
def test_entry_points_and_per_tile_status(ctx, pt, na, be):
    """Host planes, device planes, the pointer-table batch and the strided batch give the
    restatement's pixels; one pixel of one tile outside binding 6's [global_min, global_max] fails
    that tile only (OMR_QUANTIZATION in its status word, the others rendered)."""
    import torch
    dtype = DTYPE[pt]
    lo, hi = _range(dtype)
    w, n = 40, 3
    active = [_chan(dtype, i, na, reverse=i == 2, **({"lut": LUT} if i == 5 else {})) for i in range(na)]
    if pt != _lib.PIXELS_UINT8:
        active[1].update(family=_lib.FAMILY_POLYNOMIAL, coefficient=1.5)
    chans = _spread(active)
    assert chans[6]["active"]
    limit = hi - np.floor(0.1 * (hi - lo))
    chans[6]["global_max"] = limit
    rng = np.random.default_rng(1400 + na)
    tiles = [_planes(rng, dtype, len(chans), H, w) for _ in range(n)]
    for t in tiles:
        t[6] = np.minimum(t[6], dtype(limit))
    tiles[1][6][7, 11] = dtype(limit + 1)
    tiles = [_be(t, be) for t in tiles]
    q = make_qdef("rgb")
    flip = dict(flip_h=True, flip_v=na % 2 == 1)
    exp = []
    for i, t in enumerate(tiles):
        st, e = O.render(chans, t, pt, w, H, big_endian=be, **flip)
        assert st == (_lib.QUANTIZATION if i == 1 else 0)
        exp.append(e)
    dtiles = [[dev(p) for p in t] for t in tiles]
    for i in range(n):                                       # host planes, then device planes
        out = torch.empty((H, w), dtype=torch.int32, device="cuda")
        if i == 1:
            with pytest.raises(_lib.OmrError) as ei:
                ctx.render_packed_int(q, chans, tiles[i], pt, w, H, big_endian=be, **flip)
            assert ei.value.status == _lib.QUANTIZATION
            ctx.render_packed_int_device(q, chans, dtiles[i], pt, w, H, out, big_endian=be, **flip)
            with pytest.raises(_lib.OmrError) as ei:
                ctx.synchronize()
            assert ei.value.status == _lib.QUANTIZATION
            continue
        np.testing.assert_array_equal(ctx.render_packed_int(q, chans, tiles[i], pt, w, H, big_endian=be, **flip), exp[i])
        ctx.render_packed_int_device(q, chans, dtiles[i], pt, w, H, out, big_endian=be, **flip)
        ctx.synchronize()
        np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), exp[i])
    table = torch.tensor([[b.data_ptr() for b in t] for t in dtiles], dtype=torch.int64, device="cuda")
    raw = np.concatenate([np.ascontiguousarray(p).view(np.uint8).reshape(-1) for t in tiles for p in t])
    data = torch.from_numpy(raw).to("cuda")
    plane = H * w * np.dtype(dtype).itemsize
    for strided in (False, True):
        out = torch.zeros((n, H, w), dtype=torch.int32, device="cuda")
        status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        if strided:
            ctx.render_batch_strided_device(q, chans, data, len(chans) * plane, plane, n, pt, w, H, out, status,
                                            big_endian=be, **flip)
        else:
            ctx.render_batch_device(q, chans, table, n, pt, w, H, out, status, big_endian=be, **flip)
        with pytest.raises(_lib.OmrError) as ei:
            ctx.synchronize()
        assert ei.value.status == _lib.QUANTIZATION
        assert list(status.cpu().numpy()) == [0, _lib.QUANTIZATION, 0]
        got = out.cpu().numpy().view(np.uint32)
        for i in (0, 2):
            np.testing.assert_array_equal(got[i], exp[i], err_msg=f"strided {strided} tile {i}")


# ---- limits -------------------------------------------------------------------------------------
def test_thirty_two_succeed_thirty_three_refused(ctx):
    dtype, pt, w = np.uint16, _lib.PIXELS_UINT16, 37
    rng = np.random.default_rng(1500)
    chans = [_chan(dtype, i, 32) for i in range(33)]
    planes = _planes(rng, dtype, 33, H, w)
    _check(ctx, chans[:32], planes[:32], pt, w)
    with pytest.raises(_lib.OmrError) as ei:
        ctx.render_packed_int(make_qdef("rgb"), chans, planes, pt, w, H)
    assert ei.value.status == _lib.INVALID_ARGUMENT
    _check(ctx, chans[:32], planes[:32], pt, w, flip=FLIPS[3])       # the context is usable afterwards
    chans[17]["active"] = False                                      # 33 bindings, 32 active
    _check(ctx, chans, planes, pt, w)


@pytest.mark.parametrize("pt", [_lib.PIXELS_UINT16, _lib.PIXELS_FLOAT], ids=lambda t: PT_NAME[t])
def test_greyscale_renders_the_first_of_nine_active(ctx, pt):
    dtype, w = DTYPE[pt], 40
    rng = np.random.default_rng(1600)
    chans = _spread([_chan(dtype, i, 9) for i in range(9)])
    planes = _planes(rng, dtype, len(chans), H, w)
    q = make_qdef("greyscale")
    exp = _check(ctx, chans, planes, pt, w, qdef=q)
    first = [dict(c, active=c["active"] and k == 1) for k, c in enumerate(chans)]     # binding 0 is inactive
    st, alone = O.render(first, planes, pt, w, H, qdef=q)
    assert st == 0
    np.testing.assert_array_equal(exp, alone)


# ---- encoder and projection fallbacks at the 4 -> 5 boundary ------------------------------------
@pytest.mark.parametrize("pt", [_lib.PIXELS_UINT8, _lib.PIXELS_INT16], ids=lambda t: PT_NAME[t])
def test_render_jpeg_batch_five_channels(ctx, pt):
    """Five channels on 32x48 tiles (sides the fused F1 kernel takes at four): K2 NA = 0 + the
    batched encoder, files byte-identical to the restatement's render + JPEG."""
    from test_render_jpeg_gpu import _expect, _run
    dtype = DTYPE[pt]
    h, w = 32, 48
    rng = np.random.default_rng(1700 + pt)
    chans = [_chan(dtype, i, 5, reverse=i == 3) for i in range(5)]
    tiles = [_planes(rng, dtype, 5, h, w) for _ in range(2)]
    files, st = _run(ctx, chans, tiles, pt, w, h, flip=(True, False))
    assert (st == 0).all()
    assert files == _expect(chans, tiles, pt, w, h, flip=(True, False))


@pytest.mark.parametrize("na", [5, 8])
@pytest.mark.parametrize("alg", [_lib.PROJECTION_MAX, _lib.PROJECTION_MEAN], ids=["max", "mean"])
@pytest.mark.parametrize("k3r", [False, True], ids=["k3_k2", "k3r_set"])
def test_render_projected_five_and_eight_channels(ctx, monkeypatch, k3r, alg, na):
    """Projection glue above the fused K3R kernel's four channels (with OMR_K3R=1 too, where the
    request must fall back): K3 + K2 NA = 0."""
    import omr
    from test_project_gpu import _glue
    z, w = 5, 40
    rng = np.random.default_rng(1800 + na)
    stacks = [rng.integers(0, 65536, (z, H, w)).astype(np.uint16) for _ in range(na)]
    chans = [_chan(np.uint16, i, na, reverse=i == 0) for i in range(na)]
    chans[2].update(family=_lib.FAMILY_LOGARITHMIC)
    if k3r:
        monkeypatch.setenv("OMR_K3R", "1")
    c = omr.Context(0) if k3r else ctx
    try:
        _glue(c, chans, stacks, _lib.PIXELS_UINT16, w, H, z, alg, 0, z - 1, flip=(False, True))
    finally:
        if k3r:
            c.close()


# ---- the random sweep at 5..12 channels ---------------------------------------------------------
@pytest.mark.parametrize("seed", list(range(5000, 5028)))
def test_render_sweep_many_channels(ctx, seed):
    """test_render_sweep's settings and assertions with the channel count drawn from 5..12 (four
    seeds per pixel type)."""
    pt, dtype, chans, q, (fh, fv), rng = _config(seed, n_range=(5, 13))
    h, w = 24, WIDTHS[seed % 2]
    planes = _planes(rng, dtype, len(chans), h, w)
    st, exp = O.render(chans, planes, pt, w, h, qdef=q, flip_h=fh, flip_v=fv)
    try:
        got = ctx.render_packed_int(q, chans, planes, pt, w, h, flip_h=fh, flip_v=fv)
        gst = 0
    except _lib.OmrError as e:
        gst = e.status
    assert gst == st, f"status {gst} vs restatement {st}"
    if st:
        return
    linear = all(c.get("family", _lib.FAMILY_LINEAR) == _lib.FAMILY_LINEAR for c in chans if c["active"])
    if linear or _lib.BYTES_PER_PIXEL[pt] <= 2:
        np.testing.assert_array_equal(got, exp)
    else:
        g, e = got.view(np.uint8).astype(int), exp.view(np.uint8).astype(int)
        print(f"seed {seed}: max diff {np.abs(g - e).max()}, exact {np.mean(got == exp):.4f}")
        assert np.abs(g - e).max() <= 2 and np.mean(got == exp) > 0.98
