"""Helpers of the K2 plan-cache tests: contexts created under an environment, 16-bit tiles
holding every value, a strided batch render and its CPU restatement."""
import contextlib
import os

import numpy as np

import oracle_lib as O
from omr import _lib
from omr.synthetic import C2_COLORS

U16, I16 = _lib.PIXELS_UINT16, _lib.PIXELS_INT16
NP = {U16: np.uint16, I16: np.int16}


@contextlib.contextmanager
def context_with(**env):
    """A context created under the given environment (the library reads its switches at
    omr_ctx_create)."""
    import omr
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        c = omr.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    try:
        yield c
    finally:
        c.close()


def channels(pt, windows):
    lo, hi = (0.0, 65535.0) if pt == U16 else (-32768.0, 32767.0)
    return [{"active": True, "input_start": float(ws), "input_end": float(we), "global_min": lo, "global_max": hi,
             "rgba": C2_COLORS[i % 4]} for i, (ws, we) in enumerate(windows)]


_base = {}


def tiles(pt, be, n, na, h=256, w=256, row_stride=None):
    """[n][na][h][row_stride] pixels; every 16-bit value once per 65,536 pixels of a channel
    (a rolled copy of one permutation per channel: no two tiles or channels alike)."""
    rs = row_stride or w
    if "perm" not in _base:
        _base["perm"] = np.random.default_rng(16).permutation(65536).astype(np.uint16)
    perm = _base["perm"]
    out = np.empty((n, na, h, rs), np.uint16)
    for t in range(n):
        for c in range(na):
            out[t, c] = np.resize(np.roll(perm, 977 * t + 131 * c + 1), h * rs).reshape(h, rs)
    out = out.view(NP[pt])
    return out.astype(out.dtype.newbyteorder(">")) if be else out


def render(ctx, host, pt, be, chans, w, h, fh=False, fv=False):
    import torch
    n, na, _, rs = host.shape
    data = torch.from_numpy(np.ascontiguousarray(host).view(np.uint8).reshape(-1).copy()).to("cuda")
    out = torch.empty((n, h, w), dtype=torch.int32, device="cuda")
    pb = host.shape[2] * rs * 2
    ctx.render_batch_strided_device(O.make_qdef("rgb"), chans, data, na * pb, pb, n, pt, w, h, out, big_endian=be,
                                    flip_h=fh, flip_v=fv, row_stride=rs)
    ctx.synchronize()
    return out.cpu().numpy().view(np.uint32)


def expected(host, pt, be, chans, w, h, fh=False, fv=False):
    n, na, _, rs = host.shape
    if rs == w:
        planes = [[np.ascontiguousarray(host[t, c]) for c in range(na)] for t in range(n)]
        _, exp = O.render_tiles_mt(chans, planes, n, pt, w, h, big_endian=be, flip_h=fh, flip_v=fv, n_threads=8)
        return exp
    exp = np.empty((n, h, w), np.uint32)
    for t in range(n):
        st, exp[t] = O.render(chans, [np.ascontiguousarray(host[t, c]) for c in range(na)], pt, w, h, big_endian=be,
                              flip_h=fh, flip_v=fv, row_stride=rs)
        assert st == 0
    return exp
