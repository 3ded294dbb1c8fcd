"""JPEG 2000 codestreams alone, reversible (K19) and irreversible (K20: the 9/7 transform with scalar
quantisation and the irreversible colour transform), through the calls that take flags:
omr_j2k_decode_host_ex, omr_j2k_decode_batch_device_ex and omr_j2k_stream_forms_ex.  With
irreversible=False they are omr.j2k_decode_host, omr.j2k_decode_batch_device and
omr.j2k_stream_forms: a 9/7 stream is refused by name."""
import ctypes

import numpy as np

from . import _lib
from ._lib import lib
from .tiffimage import _decode_batch_device, _decode_host_frame


def _flags(irreversible):
    return _lib.J2K_ALLOW_IRREVERSIBLE if irreversible else 0


def decode_host(stream, width, height, samples=1, bits=8, irreversible=True):
    """The host decoder (get_tile's): [height][width] or [height][width][3], uint8 or uint16, or
    OmrError (INVALID_ARGUMENT: a form out of scope, named in the message; INTERNAL: damage)."""
    return _decode_host_frame(
        lambda tab, ntab, src, nsrc, out, why, nwhy: lib.omr_j2k_decode_host_ex(
            src, nsrc, int(width), int(height), int(samples), int(bits), _flags(irreversible), out, why, nwhy),
        stream, width, height, samples, dtype=np.uint16 if bits == 16 else np.uint8)


def decode_batch_device(ctx, streams, sizes, samples=1, bits=8, irreversible=True):
    """streams[i] with a frame of sizes[i] = (width, height), decoded on ctx's GPU, reversible and
    irreversible ones side by side.  Returns ([arrays, [h][w] or [h][w][3], uint8 or uint16],
    [status per stream]); the bytes are the host decoder's."""
    return _decode_batch_device(
        ctx, streams, sizes, samples, bits // 8, "<u2" if bits == 16 else "u1",
        lambda blob, offs, lens, ws, hs, n, out, doffs, status: lib.omr_j2k_decode_batch_device_ex(
            ctx.h, blob, offs, lens, ws, hs, n, int(samples), int(bits), _flags(irreversible), out, doffs,
            status))


def stream_forms(stream):
    """(names of _lib.J2K_FORM_NAMES, names of _lib.J2K_LOSSY_FORM_NAMES) a good codestream uses;
    the second set is empty for a reversible stream."""
    src = np.frombuffer(bytes(stream), dtype=np.uint8)
    bits, lossy = ctypes.c_uint64(0), ctypes.c_uint32(0)
    _lib.check(lib.omr_j2k_stream_forms_ex(src.ctypes.data if src.size else None, src.size, _lib.J2K_ALLOW_IRREVERSIBLE,
                                           ctypes.byref(bits), ctypes.byref(lossy)))
    return ({n for k, n in enumerate(_lib.J2K_FORM_NAMES) if bits.value >> k & 1},
            {n for k, n in enumerate(_lib.J2K_LOSSY_FORM_NAMES) if lossy.value >> k & 1})
