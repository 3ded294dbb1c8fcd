"""Makes tests/golden/lz4_blocks.npz: (data, stream) pairs from a real LZ4 encoder, the system's
liblz4 through ctypes (LZ4_compress_default and LZ4_compress_HC), which pin the inner codec of the
Blosc reader (K15) to something other than the project's own encoder.  Run once where liblz4.so.1 is
installed; the tests only read the file.

    python tools/make_lz4_golden.py
"""
import ctypes
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden", "lz4_blocks.npz")


def shuffled_halves():
    """The high-byte and low-byte halves of one shuffled 64 x 48 uint16 chunk: blobs on a noisy
    floor, so the high bytes compress and the low bytes hardly do."""
    rng = np.random.default_rng(152)
    yy, xx = np.mgrid[0:48, 0:64]
    a = 200 + rng.integers(0, 60, (48, 64))
    for cx, cy, s, amp in ((20, 15, 6.0, 3000), (45, 30, 9.0, 1800)):
        a = a + amp * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s * s))
    b = a.astype("<u2").tobytes()
    return b[1::2], b[0::2]


def cases():
    rng = np.random.default_rng(151)
    few = rng.integers(0, 5, 8000, dtype=np.uint8).tobytes()
    ramp = (np.arange(8000) // 5).astype(np.uint8).tobytes()
    high, low = shuffled_halves()
    return [("one_byte", b"\x2a", 0), ("abc", b"abc", 0),
            ("noise_3000", rng.integers(0, 256, 3000, dtype=np.uint8).tobytes(), 0),
            ("equal_70000", b"\x3c" * 70000, 0),
            ("few_8000", few, 0), ("few_8000_hc", few, 9),
            ("ramp_8000", ramp, 0), ("ramp_8000_hc", ramp, 9),
            ("chunk_high_bytes", high, 0), ("chunk_low_bytes", low, 0)]


def main():
    lz = ctypes.CDLL("liblz4.so.1")
    out = {}
    names = []
    for name, data, hc in cases():
        cap = lz.LZ4_compressBound(len(data))
        buf = ctypes.create_string_buffer(cap)
        n = lz.LZ4_compress_HC(data, buf, len(data), cap, hc) if hc else lz.LZ4_compress_default(data, buf, len(data), cap)
        assert n > 0, name
        back = ctypes.create_string_buffer(len(data) + 1)
        assert lz.LZ4_decompress_safe(buf.raw[:n], back, n, len(data)) == len(data) and back.raw[:len(data)] == data
        out[name + "__data"] = np.frombuffer(data, dtype=np.uint8)
        out[name + "__stream"] = np.frombuffer(buf.raw[:n], dtype=np.uint8)
        names.append(name)
        print(f"{name}: {len(data)} -> {n} bytes")
    out["names"] = np.array(names)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
