#!/usr/bin/env python3
"""Writes tests/golden/zstd_frames.npz: Zstandard frames of a real encoder for the K16 tests.

libzstd (libzstd.so.1 through ctypes; the fixture in the repository was written with 1.4.8)
compresses the inputs of tests/zstd_streams.py with ZSTD_compress at levels 1, 5 and 19,
ZSTD_compress2 with the checksum flag, and ZSTD_compressStream2 with a flush in the middle (a
windowed frame without a content size).  omr.zstd_frame_forms tells which forms each frame uses;
per form the smallest frame that adds it is kept (and ALWAYS), and the run fails when a required form
(zstd_streams.REQUIRED_FORMS) is missing.  The fixture stores the frames kept ("frame/<input>@<how>"),
the SHA-256 of every input used ("sha/<input>"), and for the group test the level-5 frame of every
stream of zstd_streams.chunk_image's Blosc chunks ("chunk/<SHA-256 of the stream's bytes>").

    python tools/make_zstd_golden.py            # needs the built library and libzstd.so.1
"""
import ctypes
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "omero-ms-image-region_amd"), os.path.join(REPO, "tests")]

import omr  # noqa: E402
import zstd_streams as zs  # noqa: E402

Z = ctypes.CDLL("libzstd.so.1")
Z.ZSTD_compressBound.restype = ctypes.c_size_t
Z.ZSTD_compressBound.argtypes = [ctypes.c_size_t]
Z.ZSTD_isError.argtypes = [ctypes.c_size_t]
Z.ZSTD_compress.restype = ctypes.c_size_t
Z.ZSTD_compress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int]
Z.ZSTD_createCCtx.restype = ctypes.c_void_p
Z.ZSTD_freeCCtx.argtypes = [ctypes.c_void_p]
Z.ZSTD_CCtx_setParameter.restype = ctypes.c_size_t
Z.ZSTD_CCtx_setParameter.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
Z.ZSTD_compress2.restype = ctypes.c_size_t
Z.ZSTD_compress2.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]
Z.ZSTD_versionString.restype = ctypes.c_char_p
C_LEVEL, C_CHECKSUM = 100, 201                 # ZSTD_c_compressionLevel, ZSTD_c_checksumFlag
E_CONTINUE, E_FLUSH, E_END = 0, 1, 2


class Buf(ctypes.Structure):                   # ZSTD_inBuffer and ZSTD_outBuffer have the same layout
    _fields_ = [("p", ctypes.c_void_p), ("size", ctypes.c_size_t), ("pos", ctypes.c_size_t)]


Z.ZSTD_compressStream2.restype = ctypes.c_size_t
Z.ZSTD_compressStream2.argtypes = [ctypes.c_void_p, ctypes.POINTER(Buf), ctypes.POINTER(Buf), ctypes.c_int]


def check(n):
    assert not Z.ZSTD_isError(n), "libzstd failed"
    return n


def compress(data, level):
    cap = Z.ZSTD_compressBound(len(data))
    out = ctypes.create_string_buffer(cap)
    n = check(Z.ZSTD_compress(out, cap, data, len(data), level))
    return out.raw[:n]


def compress_checksum(data, level):
    c = Z.ZSTD_createCCtx()
    check(Z.ZSTD_CCtx_setParameter(c, C_LEVEL, level))
    check(Z.ZSTD_CCtx_setParameter(c, C_CHECKSUM, 1))
    cap = Z.ZSTD_compressBound(len(data))
    out = ctypes.create_string_buffer(cap)
    n = check(Z.ZSTD_compress2(c, out, cap, data, len(data)))
    Z.ZSTD_freeCCtx(c)
    return out.raw[:n]


def compress_stream(data, level):
    """Streamed with a flush in the middle: a windowed frame without a content size."""
    c = Z.ZSTD_createCCtx()
    check(Z.ZSTD_CCtx_setParameter(c, C_LEVEL, level))
    cap = Z.ZSTD_compressBound(len(data)) + 1024
    out = ctypes.create_string_buffer(cap)
    src = ctypes.create_string_buffer(data, max(len(data), 1))
    ob = Buf(ctypes.addressof(out), cap, 0)
    half = len(data) // 2
    for end, op in ((half, E_FLUSH), (len(data), E_END)):
        ib = Buf(ctypes.addressof(src), end, 0 if end == half else half)
        while True:
            left = check(Z.ZSTD_compressStream2(c, ctypes.byref(ob), ctypes.byref(ib), op))
            if left == 0 and ib.pos == ib.size:
                break
    Z.ZSTD_freeCCtx(c)
    return out.raw[:ob.pos]


ALWAYS = ("image_small_shuffled@l5",)            # kept whatever it adds: what a shuffled chunk of pixels looks like


def main():
    print("libzstd", Z.ZSTD_versionString().decode())
    data = zs.inputs()
    cands = []
    for name, d in data.items():
        for how, fn in (("l1", lambda b: compress(b, 1)), ("l5", lambda b: compress(b, 5)), ("l19", lambda b: compress(b, 19)),
                        ("ck5", lambda b: compress_checksum(b, 5)), ("st1", lambda b: compress_stream(b, 1)),
                        ("st19", lambda b: compress_stream(b, 19))):
            f = fn(d)
            assert omr.zstd_decode_host(f, len(d)) == d, (name, how)
            cands.append((len(f), f"{name}@{how}", f, omr.zstd_frame_forms(f)))
    cands.sort(key=lambda c: (c[0], c[1]))
    kept, have = [], set()
    for size, key, f, forms in cands:                       # smallest first: a frame is kept when it adds a form
        if forms - have or key in ALWAYS:
            kept.append((key, f))
            have |= forms
    missing = zs.REQUIRED_FORMS - have
    assert not missing, f"no frame uses {sorted(missing)}"
    arrays = {}
    for key, f in kept:
        arrays["frame/" + key] = np.frombuffer(f, dtype=np.uint8)
        src = key.split("@")[0]
        arrays["sha/" + src] = np.array(zs.sha(data[src]))
    for part in zs.chunk_parts():
        arrays["chunk/" + zs.sha(part)] = np.frombuffer(compress(part, 5), dtype=np.uint8)
    np.savez(zs.GOLDEN, **arrays)
    total = sum(len(f) for _, f in kept)
    print(f"{len(kept)} frames, {total} bytes; forms {sorted(have)}")
    for key, f in kept:
        print(f"  {key}: {len(f)} bytes")
    print(zs.GOLDEN, os.path.getsize(zs.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
