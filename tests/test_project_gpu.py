"""K3 Z-projection and the flip kernels on the GPU vs the CPU restatement.

Projection: ProjectionService.java:46-317 (bit-exact for every pixel type: integer sums are
exact, float sums keep the reference's z order in double).  Flips: the reference's index-oracle
tests (ImageRegionRequestHandlerTest.java:69-200, ShapeMaskRequestHandlerTest.java:84-215).
"""
import functools
import os

import numpy as np
import pytest

import oracle_lib as O
from omr import _lib, flip
from omr.synthetic import c2_channels, microscopy_u16

pytestmark = pytest.mark.gpu

TYPES = [(_lib.PIXELS_UINT8, np.uint8), (_lib.PIXELS_INT8, np.int8), (_lib.PIXELS_UINT16, np.uint16),
         (_lib.PIXELS_INT16, np.int16), (_lib.PIXELS_UINT32, np.uint32), (_lib.PIXELS_INT32, np.int32),
         (_lib.PIXELS_FLOAT, np.float32), (_lib.PIXELS_DOUBLE, np.float64)]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to("cuda")


def rand_stack(dtype, z, h, w, seed):
    rng = np.random.default_rng(seed)
    if np.issubdtype(dtype, np.floating):
        return (rng.normal(0, 1e4, (z, h, w))).astype(dtype)
    info = np.iinfo(dtype)
    return rng.integers(info.min, info.max, (z, h, w), endpoint=True, dtype=np.int64).astype(dtype)


@pytest.mark.parametrize("pt,dtype", TYPES)
@pytest.mark.parametrize("alg", [_lib.PROJECTION_MAX, _lib.PROJECTION_MEAN, _lib.PROJECTION_SUM])
def test_projection_bit_exact_all_types(ctx, pt, dtype, alg):
    z, h, w = 7, 9, 13                                     # ragged plane (117 px)
    stack = rand_stack(dtype, z, h, w, 100 + pt)
    for (start, end, step, bi, bo) in [(0, 6, 1, False, False), (1, 5, 2, True, True), (3, 3, 1, True, False),
                                       (0, 6, 3, False, True)]:
        src = stack.astype(stack.dtype.newbyteorder(">")) if bi else stack
        st, exp = O.project(src, pt, w, h, z, alg, start, end, step, be_in=bi, be_out=bo)
        assert st == 0
        got = ctx.project_stack(src, pt, w, h, z, alg, start, end, step, big_endian_in=bi, big_endian_out=bo)
        np.testing.assert_array_equal(got, exp, err_msg=f"{start},{end},{step},{bi},{bo}")


@pytest.mark.parametrize("pt,dtype", TYPES)
@pytest.mark.parametrize("alg", [_lib.PROJECTION_MAX, _lib.PROJECTION_MEAN, _lib.PROJECTION_SUM])
def test_projection_vector_path_all_types(ctx, pt, dtype, alg):
    """16-B vector K3 (plane = whole 16-B chunks): z split over 4 waves for max and integer
    sums, uneven quarters, unroll tails, start > end, stepping."""
    z, h, w = 37, 16, 24
    stack = rand_stack(dtype, z, h, w, 300 + pt)
    for (start, end, step, bi, bo) in [(0, 36, 1, False, False), (2, 30, 3, True, True), (5, 5, 1, True, False),
                                       (9, 4, 1, False, True), (0, 36, 7, True, True), (1, 34, 1, False, False)]:
        src = stack.astype(stack.dtype.newbyteorder(">")) if bi else stack
        st, exp = O.project(src, pt, w, h, z, alg, start, end, step, be_in=bi, be_out=bo)
        assert st == 0
        got = ctx.project_stack(src, pt, w, h, z, alg, start, end, step, big_endian_in=bi, big_endian_out=bo)
        np.testing.assert_array_equal(got, exp, err_msg=f"{start},{end},{step},{bi},{bo}")


def test_projection_device_api_and_validation(ctx):
    import torch
    z, h, w = 64, 128, 256
    stack = rand_stack(np.uint16, z, h, w, 5)
    d = dev(stack.astype(">u2"))
    out = torch.empty(h * w * 2, dtype=torch.uint8, device="cuda")
    ctx.project_stack_device(d, _lib.PIXELS_UINT16, w, h, z, _lib.PROJECTION_MEAN, 0, z - 1, out,
                             big_endian_in=True)
    ctx.synchronize()
    st, exp = O.project(stack.astype(">u2"), _lib.PIXELS_UINT16, w, h, z, _lib.PROJECTION_MEAN, 0, z - 1, be_in=True)
    np.testing.assert_array_equal(out.cpu().numpy(), exp)
    for start, end, step, alg in [(-1, 2, 1, 0), (0, z, 1, 0), (z, 0, 1, 0), (0, 3, 0, 0), (0, 3, 1, 9)]:
        with pytest.raises(_lib.OmrError) as ei:
            ctx.project_stack(stack, _lib.PIXELS_UINT16, w, h, z, alg, start, end, step)
        assert ei.value.status == _lib.INVALID_ARGUMENT


@pytest.mark.parametrize("alg", [_lib.PROJECTION_MAX, _lib.PROJECTION_MEAN, _lib.PROJECTION_SUM])
def test_project_stacks_device_one_launch(ctx, alg):
    """omr_project_stacks_device: three stacks in one launch (the glue's K3), each == the oracle."""
    import torch
    z, h, w = 20, 64, 96
    stacks = [rand_stack(np.uint16, z, h, w, 40 + c).astype(">u2") for c in range(3)]
    outs = [torch.empty(h * w * 2, dtype=torch.uint8, device="cuda") for _ in range(3)]
    ctx.project_stacks_device([dev(s) for s in stacks], _lib.PIXELS_UINT16, w, h, z, alg, 2, z - 3, outs,
                              big_endian_in=True)
    ctx.synchronize()
    for s, o in zip(stacks, outs):
        st, exp = O.project(s, _lib.PIXELS_UINT16, w, h, z, alg, 2, z - 3, be_in=True)
        assert st == 0
        np.testing.assert_array_equal(o.cpu().numpy(), exp)
    with pytest.raises(_lib.OmrError):
        ctx.project_stacks_device([dev(stacks[0])] * 33, _lib.PIXELS_UINT16, w, h, z, alg, 0, 1, outs * 11)


@pytest.mark.parametrize("alg", [_lib.PROJECTION_MAX, _lib.PROJECTION_MEAN])
def test_c3_projection_then_composite_full_size(ctx, alg):
    """BASELINE config C3: 3-channel uint16 512x512x64 Z-stack -> max/mean projection -> composite.
    Default bounds 0..63 (ImageRegionRequestHandler.java:511-516): mean skips the last plane."""
    import torch
    z, h, w = 64, 512, 512
    rng = np.random.default_rng(20261015 + 3)
    base = [microscopy_u16(h, w, rng) for _ in range(3)]
    stacks = [np.stack([np.clip(b.astype(np.int64) + rng.integers(-500, 500, (h, w)), 0, 65535).astype(np.uint16)
                        for _ in range(z)]) for b in base]
    be = [s.astype(">u2") for s in stacks]
    chans = c2_channels(3)
    projected = []
    for s in be:
        st, p = O.project(s, _lib.PIXELS_UINT16, w, h, z, alg, 0, z - 1, be_in=True, be_out=True)
        assert st == 0
        projected.append(p.view(">u2").reshape(h, w))
    st, exp = O.render(chans, projected, _lib.PIXELS_UINT16, w, h, big_endian=True)
    out = torch.empty((h, w), dtype=torch.int32, device="cuda")
    ctx.render_projected_device(O.make_qdef("rgb"), chans, [dev(s) for s in be], _lib.PIXELS_UINT16, w, h, z,
                                alg, 0, z - 1, out, big_endian=True)
    ctx.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), exp)


# ---- flips: ported index-oracle tests on the device kernels ------------------------------
@pytest.mark.parametrize("w,h", [(4, 4), (5, 5), (7, 4), (4, 7), (7, 1), (1, 7), (1, 1)])
def test_flip_argb_index_oracle(ctx, w, h):
    import torch
    src = torch.arange(w * h, dtype=torch.int32, device="cuda")
    for fh, fv in [(False, True), (True, False), (True, True)]:
        f = flip(ctx, src, w, h, fh, fv).cpu().numpy()
        for n in range(w * h):
            nc = w - 1 - n % w if fh else n % w
            nr = h - 1 - n // w if fv else n // w
            assert f[nr * w + nc] == n
    assert flip(ctx, src, w, h, False, False) is src           # no flip returns src


@pytest.mark.parametrize("w,h", [(4, 4), (5, 5), (7, 4), (4, 7), (7, 1), (1, 7), (1, 1)])
def test_flip_mask_index_oracle(ctx, w, h):
    import torch
    src = torch.arange(w * h, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    for fh, fv in [(False, True), (True, False), (True, True)]:
        ctx.flip_mask_device(src, dst, w, h, fh, fv)
        f = dst.cpu().numpy()
        for n in range(w * h):
            nc = w - 1 - n % w if fh else n % w
            nr = h - 1 - n // w if fv else n // w
            assert f[nr * w + nc] == n


def test_flip_errors(ctx):
    import torch
    with pytest.raises(ValueError):
        flip(ctx, None, 4, 4, True, True)                          # testFlipNullImage
    src = torch.ones(1, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):
        flip(ctx, src, 0, 4, True, True)                           # testFlipZeroXImage
    with pytest.raises(ValueError):
        flip(ctx, src, 4, 0, True, True)                           # testFlipZeroYImage
    with pytest.raises(_lib.OmrError):
        ctx.flip_argb_device(None, src, 4, 4, True, True)


# ---- projection glue: project every active channel + render (K3 + K2, or the fused K3R) ----
@pytest.fixture(scope="module")
def k3r_ctx():
    import os
    import omr
    os.environ["OMR_K3R"] = "1"                 # read at context creation
    try:
        c = omr.Context(0)
    finally:
        del os.environ["OMR_K3R"]
    yield c
    c.close()


@pytest.fixture(params=["k3_k2", "k3r"])
def glue_ctx(request, ctx, k3r_ctx):
    return ctx if request.param == "k3_k2" else k3r_ctx


def _glue(ctx, chans, stacks, pt, w, h, z, alg, start, end, stepping=1, be=False, flip=(False, False),
          model="rgb", qd_kw=None):
    import torch
    q = O.make_qdef(model, **(qd_kw or {}))
    out = torch.empty((h, w), dtype=torch.int32, device="cuda")
    devs = [dev(s) if s is not None else None for s in stacks]
    torch.cuda.synchronize()
    ctx.render_projected_device(q, chans, devs, pt, w, h, z, alg, start, end, out, stepping=stepping,
                                big_endian=be, flip_h=flip[0], flip_v=flip[1])
    ctx.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    planes = []
    for c, s in enumerate(stacks):
        if s is None or not chans[c].get("active", True):
            planes.append(None)
            continue
        st, p = O.project(s, pt, w, h, z, alg, start, end, stepping, be_in=be, be_out=be)
        assert st == 0
        planes.append(p)
    planes = [p if p is not None else np.zeros(w * h * np.dtype(stacks[0].dtype).itemsize, np.uint8) for p in planes]
    st, exp = O.render(chans, planes, pt, w, h, big_endian=be, flip_h=flip[0], flip_v=flip[1], qdef=q)
    assert st == 0
    np.testing.assert_array_equal(got, exp)


GLUE_TYPES = [(_lib.PIXELS_UINT16, np.uint16, (0.0, 65535.0)), (_lib.PIXELS_INT16, np.int16, (-32768.0, 32767.0)),
              (_lib.PIXELS_UINT8, np.uint8, (0.0, 255.0)), (_lib.PIXELS_INT8, np.int8, (-128.0, 127.0))]


@pytest.mark.parametrize("pt,dtype,rng_", GLUE_TYPES)
@pytest.mark.parametrize("alg", [_lib.PROJECTION_MAX, _lib.PROJECTION_MEAN, _lib.PROJECTION_SUM])
@pytest.mark.parametrize("be", [False, True])
def test_projection_glue_types_and_algorithms(glue_ctx, pt, dtype, rng_, alg, be):
    ctx = glue_ctx
    z, h, w = 13, 48, 64
    stacks = [rand_stack(dtype, z, h, w, 300 + c) for c in range(3)]
    if be:
        stacks = [s.astype(s.dtype.newbyteorder(">")) for s in stacks]
    lo, hi = rng_
    span = hi - lo
    chans = [{"input_start": lo + span * f0, "input_end": lo + span * f1, "global_min": lo, "global_max": hi,
              "rgba": col} for (f0, f1), col in zip([(0.0, 1.0), (0.1, 0.7), (0.3, 0.4)],
                                                    [(255, 0, 0, 255), (0, 255, 0, 255), (0, 0, 255, 255)])]
    _glue(ctx, chans, stacks, pt, w, h, z, alg, 1, z - 2, be=be, flip=(True, False))


@pytest.mark.parametrize("n_ch", [1, 2, 4])
@pytest.mark.parametrize("flip", [(False, False), (False, True), (True, True)])
def test_projection_glue_channels_flips_modes(glue_ctx, n_ch, flip):
    ctx = glue_ctx
    z, h, w = 64, 64, 128
    rng = np.random.default_rng(n_ch)
    stacks = [np.clip(microscopy_u16(h, w, rng).astype(np.int64) + rng.integers(-300, 300, (z, h, w)), 0,
                      65535).astype(np.uint16) for _ in range(n_ch)]
    chans = c2_channels(4)[:n_ch]
    lut = np.concatenate([np.arange(256), 255 - np.arange(256), np.arange(256) // 2]).astype(np.uint8)
    variants = [{}, {"reverse": True}, {"lut": lut}, {"family": _lib.FAMILY_LOGARITHMIC}]
    for c in range(n_ch):
        chans[c].update(variants[c])
    for alg, stepping in ((_lib.PROJECTION_MAX, 1), (_lib.PROJECTION_MEAN, 2), (_lib.PROJECTION_SUM, 3)):
        _glue(ctx, chans, stacks, _lib.PIXELS_UINT16, w, h, z, alg, 2, z - 1, stepping=stepping, flip=flip)
    _glue(ctx, chans, stacks, _lib.PIXELS_UINT16, w, h, z, _lib.PROJECTION_MEAN, 0, z - 1,
          qd_kw={"cd_start": 30, "cd_end": 220})


def test_projection_glue_unfused_cases(glue_ctx):
    ctx = glue_ctx
    """Odd width, five channels, 8-bit mean, float: the K3 + K2 path, same results."""
    rng = np.random.default_rng(9)
    z = 9
    s16 = [rng.integers(0, 65536, (z, 8, 33)).astype(np.uint16) for _ in range(5)]
    chans = c2_channels(4) + c2_channels(1)
    _glue(ctx, chans[:2], s16[:2], _lib.PIXELS_UINT16, 33, 8, z, _lib.PROJECTION_MEAN, 0, z - 1)
    s16 = [rng.integers(0, 65536, (z, 8, 32)).astype(np.uint16) for _ in range(5)]
    _glue(ctx, chans, s16, _lib.PIXELS_UINT16, 32, 8, z, _lib.PROJECTION_MAX, 0, z - 1)
    s8 = [rng.integers(0, 256, (z, 16, 32)).astype(np.uint8) for _ in range(2)]
    c8 = [{"input_start": 0.0, "input_end": 255.0, "global_min": 0.0, "global_max": 255.0, "rgba": (255, 9, 0, 255)},
          {"input_start": 20.0, "input_end": 90.0, "global_min": 0.0, "global_max": 255.0, "rgba": (0, 99, 255, 255)}]
    _glue(ctx, c8, s8, _lib.PIXELS_UINT8, 32, 16, z, _lib.PROJECTION_MEAN, 0, z - 1)
    sf = [rng.uniform(-10, 300, (z, 16, 32)).astype(np.float32) for _ in range(2)]
    cf = [{"input_start": 0.0, "input_end": 255.0, "rgba": (255, 0, 0, 255)},
          {"input_start": 5.0, "input_end": 200.0, "rgba": (0, 0, 255, 255)}]
    _glue(ctx, cf, sf, _lib.PIXELS_FLOAT, 32, 16, z, _lib.PROJECTION_MAX, 0, z - 1)


def test_projection_glue_quantization_error(glue_ctx):
    ctx = glue_ctx
    import torch
    z, h, w = 4, 16, 32
    stacks = [np.full((z, h, w), 100, np.uint16) for _ in range(2)]
    stacks[1][2, 3, 4] = 65000
    chans = c2_channels(2)
    for c in chans:
        c["global_max"] = 60000.0
    out = torch.empty((h, w), dtype=torch.int32, device="cuda")
    ctx.render_projected_device(O.make_qdef("rgb"), chans, [dev(s) for s in stacks], _lib.PIXELS_UINT16, w, h, z,
                                _lib.PROJECTION_MAX, 0, z - 1, out)
    with pytest.raises(_lib.OmrError) as e:
        ctx.synchronize()
    assert e.value.status == _lib.QUANTIZATION


@pytest.mark.parametrize("seed", list(range(int(os.environ.get("OMR_SWEEP_SEEDS", "40")))))
def test_projection_glue_sweep(glue_ctx, seed):
    """Random projection requests through the glue (K3 + K2, and K3R): type, byte order, active
    channels, windows (inverted / empty / fractional), reverse, .lut, codomain, algorithm,
    z range and stepping, flips — against the restatement's project + render."""
    rng = np.random.default_rng(7000 + seed)
    pt, dtype, (lo, hi) = GLUE_TYPES[seed % len(GLUE_TYPES)]
    n = int(rng.integers(1, 5))
    z, h, w = int(rng.integers(2, 20)), 16, 32 * int(rng.integers(1, 3))
    stacks = [rand_stack(dtype, z, h, w, 9000 + 10 * seed + c) for c in range(n)]
    be = bool(rng.integers(0, 2))
    if be:
        stacks = [s.astype(s.dtype.newbyteorder(">")) for s in stacks]
    chans = []
    for c in range(n):
        a, b = sorted(rng.uniform(lo, hi, 2))
        kind = rng.integers(0, 5)
        ws, we = (b, a) if kind == 0 else (a, a) if kind == 1 else (a + 0.5, b) if kind == 2 else (a, b)
        d = {"input_start": float(ws), "input_end": float(we), "global_min": lo, "global_max": hi,
             "rgba": tuple(int(v) for v in rng.integers(0, 256, 4)), "reverse": bool(rng.integers(0, 3) == 0)}
        if rng.integers(0, 5) == 0:
            d["lut"] = rng.integers(0, 256, 768).astype(np.uint8)
        chans.append(d)
    alg = int(rng.choice([_lib.PROJECTION_MAX, _lib.PROJECTION_MEAN, _lib.PROJECTION_SUM]))
    start = int(rng.integers(0, z))
    end = int(rng.integers(start, z))
    if alg != _lib.PROJECTION_MAX and end == start:
        end = min(z - 1, start + 1)
        if end == start:
            start = max(0, start - 1)
    qd_kw = {"cd_start": 20, "cd_end": 230} if rng.integers(0, 4) == 0 else None
    _glue(glue_ctx, chans, stacks, pt, w, h, z, alg, start, end, stepping=int(rng.integers(1, 4)), be=be,
          flip=(bool(rng.integers(0, 2)), bool(rng.integers(0, 2))), qd_kw=qd_kw)


# ---- numeric edges of K3 / K3R, by construction ------------------------------------------
# Every comparison below is with O.project (double accumulator in z order), bit for bit, the sign
# of zero included; a float NaN equals a NaN of any payload or sign (x86 and the GPU produce
# different default NaNs).  Outputs on the device carry 16 canary bytes behind them.
MAX, MEAN, SUM = _lib.PROJECTION_MAX, _lib.PROJECTION_MEAN, _lib.PROJECTION_SUM
ALGS = [MAX, MEAN, SUM]
ALG_IDS = ["max", "mean", "sum"]
CANARY = 0xA5


def _bits(a, dtype, be):
    dt = np.dtype(dtype)
    u = np.ascontiguousarray(a).view(np.uint8).reshape(-1).view(np.dtype(f"u{dt.itemsize}").newbyteorder(">" if be else "<"))
    return u.astype(np.uint64)


def assert_same(got, exp, dtype, be=False, what=""):
    """got == exp as bytes of `dtype` pixels (big-endian if be); NaN == NaN for float types."""
    g, e = _bits(got, dtype, be), _bits(exp, dtype, be)
    assert g.shape == e.shape, what
    bad = g != e
    dt = np.dtype(dtype)
    if dt.kind == "f":
        mag = np.uint64((1 << (8 * dt.itemsize - 1)) - 1)
        inf = np.uint64(0x7F800000 if dt.itemsize == 4 else 0x7FF0000000000000)
        bad &= ~(((g & mag) > inf) & ((e & mag) > inf))
    if bad.any():
        i = np.flatnonzero(bad)
        raise AssertionError(f"{what}: {i.size} pixels differ, first at {i[:6].tolist()}: got "
                             f"{[hex(int(v)) for v in g[i[:6]]]} expected {[hex(int(v)) for v in e[i[:6]]]}")


def with_canary(n_bytes, offset=0):
    """A device output of n_bytes at `offset` bytes into its allocation, 16 canary bytes behind it."""
    import torch
    buf = torch.full((offset + n_bytes + 16,), CANARY, dtype=torch.uint8, device="cuda")
    return buf, buf[offset:offset + n_bytes]


def canary_ok(buf, n_bytes, offset=0):
    b = buf.cpu().numpy()
    return bool((b[:offset] == CANARY).all() and (b[offset + n_bytes:] == CANARY).all())


def project_dev(ctx, d_stack, pt, dtype, w, h, z, alg, start, end, step=1, bi=False, bo=False):
    """omr_project_stack_device into a canaried output; the output bytes."""
    n = w * h * np.dtype(dtype).itemsize
    buf, out = with_canary(n)
    ctx.project_stack_device(d_stack, pt, w, h, z, alg, start, end, out, stepping=step, big_endian_in=bi,
                             big_endian_out=bo)
    ctx.synchronize()
    assert canary_ok(buf, n), "bytes behind the output were written"
    return out.cpu().numpy()


def check_dev(ctx, stack, d_stack, pt, dtype, w, h, z, alg, start, end, step=1, bi=False, bo=False, what=""):
    st, exp = O.project(stack, pt, w, h, z, alg, start, end, step, be_in=bi, be_out=bo)
    assert st == 0
    got = project_dev(ctx, d_stack, pt, dtype, w, h, z, alg, start, end, step, bi, bo)
    assert_same(got, exp, dtype, bo, f"{what} alg {alg} z {start}..{end} step {step} be {bi}/{bo}")
    return exp


# ---- A: large stepping ---------------------------------------------------------------------
INT_MAX = 2**31 - 1


@pytest.mark.parametrize("pt,dtype", TYPES)
@pytest.mark.parametrize("w,h", [(16, 24), (13, 9)], ids=["vector", "scalar"])
def test_projection_large_stepping(ctx, pt, dtype, w, h):
    """stepping >= size_z up to INT32_MAX from start 0: max is plane 0, mean and sum are plane 0
    when end > 0 and the empty projection otherwise.  The count of planes is taken in 64 bits
    (omr_projection_plane_count): no z is stepped past end, on the host or in a kernel."""
    z = 5
    stack = rand_stack(dtype, z, h, w, 500 + pt)
    d = dev(stack)
    for step in (z, INT_MAX - 1, INT_MAX):
        for end in (0, z - 1):
            for alg in ALGS:
                exp = check_dev(ctx, stack, d, pt, dtype, w, h, z, alg, 0, end, step, what=f"{w}x{h}")
                if alg == MAX or end > 0:           # one plane: max(0, v) / v / v
                    one = np.maximum(stack[0], 0) if alg == MAX else stack[0]
                    assert_same(exp, one, dtype, what="oracle, one plane")
                got = ctx.project_stack(stack, pt, w, h, z, alg, 0, end, step)
                assert_same(got, exp, dtype, what=f"host api {alg} {end} {step}")
    # start + stepping == INT32_MAX exactly is the last valid stepping for start 1
    check_dev(ctx, stack, d, pt, dtype, w, h, z, MAX, 1, 3, INT_MAX - 1)
    check_dev(ctx, stack, d, pt, dtype, w, h, z, SUM, 1, 3, INT_MAX - 1)


def test_projection_stepping_wrap_rejected(ctx, k3r_ctx):
    """start + stepping > INT32_MAX with a loop that runs (the reference's z wraps negative and its
    plane read throws): INVALID_ARGUMENT from every projection call, and the context goes on."""
    import torch
    z, h, w = 5, 24, 16
    stack = rand_stack(np.uint16, z, h, w, 77)
    d = dev(stack)
    chans = c2_channels(1)
    for c in (ctx, k3r_ctx):
        for alg, start, end, step in [(MAX, 1, 1, INT_MAX), (MAX, 1, 3, INT_MAX), (MEAN, 1, 2, INT_MAX),
                                      (SUM, 2, 4, INT_MAX - 1), (MAX, 4, 4, INT_MAX - 3)]:
            buf, out = with_canary(h * w * 2)
            argb = torch.full((h * w + 4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            calls = [lambda: c.project_stack(stack, _lib.PIXELS_UINT16, w, h, z, alg, start, end, step),
                     lambda: c.project_stack_device(d, _lib.PIXELS_UINT16, w, h, z, alg, start, end, out, stepping=step),
                     lambda: c.project_stacks_device([d, d], _lib.PIXELS_UINT16, w, h, z, alg, start, end, [out, out],
                                                     stepping=step),
                     lambda: c.render_projected_device(O.make_qdef("rgb"), chans, [d], _lib.PIXELS_UINT16, w, h, z, alg,
                                                       start, end, argb[:h * w], stepping=step)]
            for call in calls:
                with pytest.raises(_lib.OmrError) as ei:
                    call()
                assert ei.value.status == _lib.INVALID_ARGUMENT, (alg, start, end, step)
            st, _ = O.project(stack, _lib.PIXELS_UINT16, w, h, z, alg, start, end, step)
            assert st == _lib.INVALID_ARGUMENT
            c.synchronize()
            assert canary_ok(buf, 0) and bool((argb == 0x5A5A5A5A).all())      # nothing was launched
        # mean / sum over an empty range never step: valid
        check_dev(c, stack, d, _lib.PIXELS_UINT16, np.uint16, w, h, z, SUM, 1, 1, INT_MAX)
        # and the context still projects
        check_dev(c, stack, d, _lib.PIXELS_UINT16, np.uint16, w, h, z, MEAN, 0, z - 1, 1)
        _glue(c, chans, [stack], _lib.PIXELS_UINT16, w, h, z, MAX, 0, z - 1)


# ---- B1: float specials ------------------------------------------------------------------
B1_Z = 9
COL_A, COL_B = 13, 14                 # the order-sensitive columns


def special_stack(dtype, h, w, seed):
    """z = 9 float stack: pixel k of the first row group holds case k along z, the rest random bit
    patterns (NaNs of every payload, infinities, subnormals among them)."""
    dt = np.dtype(dtype)
    fi = np.finfo(dt)
    rng = np.random.default_rng(seed)
    n = h * w
    raw = rng.integers(0, 2**(8 * dt.itemsize), (B1_Z, n), dtype=np.uint64, endpoint=False)
    st = raw.astype(f"u{dt.itemsize}").view(dt).copy()
    fin = lambda: rng.normal(0, 1e4, B1_Z).astype(dt)
    big = dt.type(1e30 if dt.itemsize == 4 else 1e300)
    sub = dt.type(fi.smallest_subnormal)
    cols = []
    cols.append(np.full(B1_Z, np.nan))                                  # 0 all NaN
    for k in (0, 4, 8):                                                 # 1..3 NaN first / middle / last
        c = fin(); c[k] = np.nan; cols.append(c)
    c = fin(); c[3] = np.inf; cols.append(c)                            # 4 +inf among finite
    c = fin(); c[3] = -np.inf; cols.append(c)                           # 5 -inf among finite
    c = fin(); c[1] = np.inf; c[5] = -np.inf; cols.append(c)            # 6 +inf and -inf (inf - inf = NaN)
    cols.append(-np.abs(fin()) - 1)                                     # 7 all negative: max is +0
    cols.append(np.full(B1_Z, -0.0))                                    # 8 only -0.0: max +0, sum +0 (0 + -0)
    c = np.ones(B1_Z); c[1] = fi.max; c[3] = fi.max; cols.append(c)     # 9 max twice: the sum clamps
    cols.append(np.full(B1_Z, -fi.max))                                 # 10 -max: no lower clamp, f32 -> -inf
    cols.append(sub * np.arange(1, B1_Z + 1))                           # 11 subnormals only
    cols.append(np.full(B1_Z, 1 + fi.eps))                              # 12 sum needs rounding on narrowing
    cols.append(np.array([big, 1, -big, 1, big, 1, -big, 1, 1]))        # 13 in order the 1s after big are lost
    cols.append(np.array([2, 1, 3, big, 5, -big, 1, 1, 1]))             # 14 (1, 7, 2): 1 + big - big
    assert len(cols) == 15 and COL_B == 14 and n >= len(cols)
    for k, c in enumerate(cols):
        st[:, k] = np.asarray(c, dtype=np.float64).astype(dt)
    return st.reshape(B1_Z, h, w)


def _ordered(stack, pt, col, alg, start, end, step, reverse):
    """The oracle's value of pixel `col` over the planes the range reads, in z order or reversed."""
    sel = stack.reshape(stack.shape[0], -1)[start:end:step, col]
    n = len(sel)
    s = np.concatenate([sel[::-1] if reverse else sel, sel[:1]]).reshape(n + 1, 1, 1)
    st, out = O.project(np.ascontiguousarray(s), pt, 1, 1, n + 1, alg, 0, n)
    assert st == 0
    return out.tobytes()


@pytest.mark.parametrize("pt,dtype", [(_lib.PIXELS_FLOAT, np.float32), (_lib.PIXELS_DOUBLE, np.float64)],
                         ids=["f32", "f64"])
def test_float_order_columns_are_order_sensitive(pt, dtype):
    """The two columns lose their point if a z reordering gives the same sum: checked on the CPU."""
    stack = special_stack(dtype, 4, 32, 1)
    for col, rng_ in ((COL_A, (0, 8, 1)), (COL_B, (1, 7, 2))):
        for alg in (MEAN, SUM):
            fwd = _ordered(stack, pt, col, alg, *rng_, reverse=False)
            assert fwd != _ordered(stack, pt, col, alg, *rng_, reverse=True), (col, alg)
            st, full = O.project(stack, pt, 32, 4, B1_Z, alg, rng_[0], rng_[1], rng_[2])
            assert full.view(dtype)[col].tobytes() == fwd
    # a split of column A's 8 planes into consecutive quarters, added in z order, differs too
    a = stack.reshape(B1_Z, -1)[:8, COL_A].astype(np.float64)
    in_order = 0.0
    for v in a:
        in_order += v
    quarters = [a[0] + a[1], a[2] + a[3], a[4] + a[5], a[6] + a[7]]
    assert in_order == 1.0 and ((quarters[0] + quarters[1]) + quarters[2]) + quarters[3] != in_order


@pytest.mark.parametrize("pt,dtype", [(_lib.PIXELS_FLOAT, np.float32), (_lib.PIXELS_DOUBLE, np.float64)],
                         ids=["f32", "f64"])
@pytest.mark.parametrize("w,h", [(32, 4), (13, 3)], ids=["vector", "scalar"])
@pytest.mark.parametrize("alg", ALGS, ids=ALG_IDS)
def test_projection_float_specials(ctx, pt, dtype, w, h, alg):
    """NaN (max skips it, sums carry it), +-inf, inf - inf, all-negative and -0.0 columns (max starts
    from +0), the clamp at the type maximum with no lower clamp, subnormals, narrowing of a double
    sum, and two columns whose sum depends on the z order."""
    stack = special_stack(dtype, h, w, 10 * pt + w)
    fi = np.finfo(dtype)
    for bi in (False, True):
        src = stack.astype(stack.dtype.newbyteorder(">")) if bi else stack
        d = dev(src)
        for bo in (False, True):
            for start, end, step in [(0, B1_Z - 1, 1), (1, 7, 2), (4, 4, 1)]:
                exp = check_dev(ctx, src, d, pt, dtype, w, h, B1_Z, alg, start, end, step, bi, bo, what=f"{w}x{h}")
                e = exp.view(np.dtype(dtype).newbyteorder(">" if bo else "<")).astype(dtype)
                # the oracle itself shows the cases (so a change of the columns cannot empty them)
                if (start, end, step) == (0, B1_Z - 1, 1):
                    if alg == MAX:
                        assert e[0] == 0 and not np.signbit(e[0]) and not np.isnan(e[1:4]).any()
                        assert e[4] == np.inf and e[7] == 0 and e[8] == 0 and not np.signbit(e[8])
                        assert e[10] == 0 and e[9] == fi.max
                    else:
                        assert np.isnan(e[0:3]).all() and e[4] == fi.max and e[5] == -np.inf and np.isnan(e[6])
                        assert e[8] == 0 and not np.signbit(e[8]) and e[7] < 0 and 0 < e[11] < fi.tiny
                    if alg == SUM:
                        assert e[9] == fi.max and e[10] == -np.inf
                        assert not np.isnan(e[3])                        # NaN in the last plane: not summed
                elif start == end and alg == MEAN:
                    assert np.isnan(e).all()                             # 0 / 0
    got = ctx.project_stack(stack, pt, w, h, B1_Z, alg, 0, B1_Z - 1)
    assert_same(got, O.project(stack, pt, w, h, B1_Z, alg, 0, B1_Z - 1)[1], dtype, what="host api")


# ---- B2: the 32-bit accumulators of K3v at their limit -------------------------------------
def limit_stack(dtype, z, npx, seed):
    """Pixel 0 the type maximum in every plane, 1 the maximum but max-1 in one plane (the mean
    truncates to max-1), 2 the minimum in every plane (a signed sum wraps in the Java narrowing),
    3 minimum and maximum alternating, the rest random."""
    info = np.iinfo(dtype)
    st = rand_stack(dtype, z, 1, npx, seed).reshape(z, npx)
    st[:, 0] = info.max
    st[:, 1] = info.max
    st[1000, 1] = info.max - 1
    st[:, 2] = info.min
    st[0::2, 3] = info.min
    st[1::2, 3] = info.max
    return st


@pytest.mark.parametrize("pt,dtype", TYPES[:4], ids=["u8", "i8", "u16", "i16"])
def test_projection_acc32_plane_limit(ctx, pt, dtype):
    """65535 summed planes is the last count K3v sums in 32 bits (udiv_inv for the mean), 65536 the
    first it sums in 64: both sides of the switch, at the values that fill the accumulator.
    At 65536 planes a 32-bit sum would still fit (65536 x 65535 < 2^32, 65536 x -32768 = -2^31);
    65537 is where it first cannot (-32768 x 65537 < -2^31), so a limit moved up fails there."""
    z = 65538
    npx = 32 // np.dtype(dtype).itemsize                 # a 32-byte plane: two 16-byte chunks
    stack = limit_stack(dtype, z, npx, 600 + pt)
    info = np.iinfo(dtype)
    for be in ((False, True) if np.dtype(dtype).itemsize > 1 else (False,)):
        src = stack.astype(stack.dtype.newbyteorder(">")) if be else stack
        d = dev(src)
        for size_z, alg, end in [(65537, MEAN, 65535), (65537, SUM, 65535), (65537, MEAN, 65536), (65537, SUM, 65536),
                                 (65537, MAX, 65536), (65538, MEAN, 65537), (65538, SUM, 65537)]:
            exp = check_dev(ctx, src, d, pt, dtype, npx, 1, size_z, alg, 0, end, 1, be, be, what=f"{dtype.__name__}")
            e = exp.view(np.dtype(dtype).newbyteorder(">" if be else "<")).astype(np.int64)
            if alg == MEAN:
                assert (e[0], e[1], e[2]) == (info.max, info.max - 1, info.min)
            if alg == MAX:
                assert (e[0], e[1], e[2], e[3]) == (info.max, info.max, max(info.min, 0), info.max)


# ---- B3: the 32-bit sums of K3R at their limit ---------------------------------------------
def _full_window(lo, hi, rgba):
    return {"input_start": lo, "input_end": hi, "global_min": lo, "global_max": hi, "rgba": rgba}


@pytest.mark.parametrize("pt,dtype,rng_", GLUE_TYPES[:2], ids=["u16", "i16"])
@pytest.mark.parametrize("n_ch", [1, 2])
def test_projection_glue_plane_limit(glue_ctx, pt, dtype, rng_, n_ch):
    """K3R sums at most 32767 planes (|sum| < 2^31, the mean by fdiv); 32768 go through K3 + K2.
    Both counts, plus 32769 planes, where a 32-bit sum first cannot hold 65535 in every plane.
    A window over the top 256 values is rendered beside the full-range one: it shows max-1 from max."""
    w, h, z = 8, 2, 32770
    lo, hi = rng_
    stacks = [limit_stack(dtype, z, w * h, 700 + c).reshape(z, h, w) for c in range(n_ch)]
    cols = [(255, 0, 0, 255), (0, 255, 0, 255)]
    full = [_full_window(lo, hi, cols[c]) for c in range(n_ch)]
    top = [dict(_full_window(lo, hi, cols[c]), input_start=hi - 255.0) for c in range(n_ch)]
    for chans in (full, top):
        for size_z, end in ((32769, 32767), (32769, 32768), (32770, 32769)):
            for alg in (MEAN, SUM):
                _glue(glue_ctx, chans, stacks, pt, w, h, size_z, alg, 0, end)


@pytest.mark.parametrize("n_iter", range(1, 8))
def test_projection_glue_max_fewer_planes_than_parts(glue_ctx, n_iter):
    """Max over 1..7 planes: fewer than K3R's eight z parts, so some parts are empty."""
    w, h, z = 16, 32, 14
    stacks = [rand_stack(np.uint16, z, h, w, 800 + c) for c in range(4)]
    chans = c2_channels(4)
    _glue(glue_ctx, chans, stacks, _lib.PIXELS_UINT16, w, h, z, MAX, 1, n_iter)
    stacks = [rand_stack(np.int16, z, h, w, 810 + c) for c in range(4)]
    chans = [_full_window(-32768.0, 32767.0, c["rgba"]) for c in c2_channels(4)]
    _glue(glue_ctx, chans, stacks, _lib.PIXELS_INT16, w, h, z, MAX, 0, 2 * (n_iter - 1), stepping=2)


# ---- B4: the scalar kernel's grid-stride loop ----------------------------------------------
def _grid_threads():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count * 8 * 256


@functools.lru_cache(maxsize=1)
def _stride_stack(dtype, z, h, w, seed):                  # one stack for the three algorithms
    rng = np.random.default_rng(seed)
    if np.issubdtype(dtype, np.floating):
        return rng.normal(0, 1e4, (z, h, w)).astype(dtype)
    return rng.integers(0, 256, (z, h, w), dtype=dtype)


@pytest.mark.parametrize("alg", ALGS, ids=ALG_IDS)
def test_projection_scalar_grid_stride_f64(ctx, alg):
    """k_project's grid is capped at cu_count * 8 blocks of 256 lanes, a lane per 16-byte chunk: an
    odd s x s float64 plane (two pixels a chunk, the last one ragged) with more chunks than that
    makes lanes take a second trip."""
    threads = _grid_threads()
    s = 1
    while -(-s * s // 2) <= threads:
        s += 2
    assert s % 2 == 1 and -(-s * s // 2) > threads and -(-(s - 2) * (s - 2) // 2) <= threads
    assert (s * s * 8) % 16 != 0                                  # not the vector path
    z = 3
    stack = _stride_stack(np.float64, z, s, s, 900)
    check_dev(ctx, stack, dev(stack), _lib.PIXELS_DOUBLE, np.float64, s, s, z, alg, 0, z - 1, what=f"{s}x{s}")


@pytest.mark.parametrize("alg", ALGS, ids=ALG_IDS)
def test_projection_scalar_grid_stride_u8(ctx, alg):
    """The same for uint8 (16 pixels a chunk): rows of 4097 pixels, the fewest rows that leave the
    plane one pixel past a whole number of chunks with more chunks than the grid has lanes."""
    threads = _grid_threads()
    w, h = 4097, 1
    while -(-w * h // 16) <= threads:
        h += 16                                                   # w * h = 1 (mod 16)
    assert (w * h) % 16 == 1 and -(-w * h // 16) > threads and -(-w * (h - 16) // 16) <= threads
    z = 3
    stack = _stride_stack(np.uint8, z, h, w, 901)
    check_dev(ctx, stack, dev(stack), _lib.PIXELS_UINT8, np.uint8, w, h, z, alg, 0, z - 1, what=f"{w}x{h}")


# ---- B5: misaligned pointers fall back to the scalar kernel; 32 stacks a launch ------------------
def _stacks_dev(ctx, stacks, d_stacks, out_offsets, w, h, z, alg, start, end):
    n = w * h * 2
    outs = [with_canary(n, off) for off in out_offsets]
    ctx.project_stacks_device(d_stacks, _lib.PIXELS_UINT16, w, h, z, alg, start, end, [o for _, o in outs])
    ctx.synchronize()
    for i, (s, (buf, o), off) in enumerate(zip(stacks, outs, out_offsets)):
        st, exp = O.project(s, _lib.PIXELS_UINT16, w, h, z, alg, start, end)
        assert st == 0
        assert_same(o.cpu().numpy(), exp, np.uint16, what=f"stack {i} alg {alg}")
        assert canary_ok(buf, n, off), f"stack {i}: bytes around the output were written"


@pytest.mark.parametrize("alg", ALGS, ids=ALG_IDS)
def test_project_stacks_device_misaligned(ctx, alg):
    """A plane of whole 16-byte chunks, but one stack or one output 4 bytes off a 16-byte address:
    the launch takes the scalar kernel for all three stacks."""
    import torch
    z, h, w = 6, 16, 24
    stacks = [rand_stack(np.uint16, z, h, w, 950 + c) for c in range(3)]
    d = [dev(s) for s in stacks]
    big = torch.zeros(stacks[1].nbytes + 64, dtype=torch.uint8, device="cuda")
    off = big[4:4 + stacks[1].nbytes]
    off.copy_(d[1])
    assert off.data_ptr() % 16 == 4 and d[0].data_ptr() % 16 == 0
    _stacks_dev(ctx, stacks, [d[0], off, d[2]], [0, 0, 0], w, h, z, alg, 0, z - 1)
    _stacks_dev(ctx, stacks, d, [0, 0, 4], w, h, z, alg, 1, z - 1)
    _stacks_dev(ctx, stacks, d, [0, 0, 0], w, h, z, alg, 0, z - 1)          # and the aligned launch itself


@pytest.mark.parametrize("alg", ALGS, ids=ALG_IDS)
def test_project_stacks_device_32_stacks(ctx, alg):
    """kMaxStacks distinct stacks in one launch (grid y = 32), each its own oracle result."""
    z, h, w = 3, 16, 24
    stacks = [rand_stack(np.uint16, z, h, w, 1000 + c) for c in range(32)]
    _stacks_dev(ctx, stacks, [dev(s) for s in stacks], [0] * 32, w, h, z, alg, 0, z - 1)


# ---- B6: empty ranges on the scalar path -----------------------------------------------------
@pytest.mark.parametrize("pt,dtype", TYPES)
@pytest.mark.parametrize("alg", ALGS, ids=ALG_IDS)
def test_projection_scalar_empty_ranges(ctx, pt, dtype, alg):
    """start > end and start == end on the ragged 13x9 plane: max of one plane or of none (+0),
    sum 0, mean 0 / 0 (NaN, 0 after an integer narrowing)."""
    z, h, w = 10, 9, 13
    stack = rand_stack(dtype, z, h, w, 1100 + pt)
    d = dev(stack)
    for start, end, step in [(9, 4, 1), (9, 4, 3), (5, 5, 1), (0, 0, 2)]:
        exp = check_dev(ctx, stack, d, pt, dtype, w, h, z, alg, start, end, step, what="13x9")
        if alg == SUM or (alg == MAX and start > end):
            assert not exp.any()

