"""The zlib streams of the K14 tests (test_zarr_read_host.py, test_zarr_read_gpu.py): good ones made
with the stdlib zlib, bad ones written bit by bit.  Made once and shared; nothing here needs a GPU."""
import functools
import zlib

import numpy as np


def deflate(data, level=-1, strategy=zlib.Z_DEFAULT_STRATEGY):
    co = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
    return co.compress(bytes(data)) + co.flush()


@functools.lru_cache(maxsize=None)
def good_streams():
    """[(name, data, stream)]: every block type and the cases the batch emitter can get wrong."""
    rng = np.random.default_rng(14)
    noise = rng.integers(0, 256, 70000, dtype=np.uint8).tobytes()
    few = rng.integers(0, 9, 5000, dtype=np.uint8).tobytes()
    half = rng.integers(0, 256, 32000, dtype=np.uint8).tobytes()
    out = [("one byte", b"\x07", deflate(b"\x07")),                       # a fixed-Huffman block
           ("equal bytes, RLE", b"\x3c" * 5000, deflate(b"\x3c" * 5000, 6, zlib.Z_RLE)),   # distance 1, length 258
           ("noise, level 0", noise, deflate(noise, 0)),                  # two stored blocks
           ("noise, level 6", noise, deflate(noise, 6)),                  # zlib falls back to stored blocks
           ("few values, fixed", few, deflate(few, 6, zlib.Z_FIXED)),
           ("few values, dynamic", few, deflate(few, 6)),
           ("few values, Huffman only", few, deflate(few, 6, zlib.Z_HUFFMAN_ONLY)),
           ("far matches", half + half, deflate(half + half, 9))]         # matches at distance 32000
    assert len(out[2][2]) > 70000 and len(out[3][2]) > 70000
    assert out[4][2][2] & 6 == 2 and out[5][2][2] & 6 == 4                # BTYPE 1 and 2
    assert len(out[7][2]) < 34000, "the second half is not matched"
    co = zlib.compressobj(6)
    pieces, stream = [], b""
    for k, flush in enumerate((zlib.Z_SYNC_FLUSH, zlib.Z_FULL_FLUSH, zlib.Z_SYNC_FLUSH, zlib.Z_SYNC_FLUSH,
                               zlib.Z_FULL_FLUSH)):
        part = (few[k * 700:k * 700 + 650] + bytes([k]) * (3 + 5 * k)) if k != 3 else b""
        pieces.append(part)
        stream += co.compress(part) + co.flush(flush)
    tail = noise[:333]
    stream += co.compress(tail) + co.flush()
    out.append(("flushed pieces", b"".join(pieces) + tail, stream))       # block ends at odd bits, empty stored blocks
    for name, data, s in out:
        assert zlib.decompress(s) == data, name
    return out


@functools.lru_cache(maxsize=None)
def mixed_streams():
    """About 300 streams for one call: [(data, stream)]."""
    rng = np.random.default_rng(15)
    sizes = [1 + (i * i * 37) % 4000 for i in range(296)] + [65536, 100000, 131072, 1]
    out = []
    for i, n in enumerate(sizes):
        kind = i % 3
        if kind == 0:
            d = rng.integers(0, 256, n, dtype=np.uint8)
        elif kind == 1:
            d = rng.integers(0, 4, n, dtype=np.uint8)
        else:
            d = (np.arange(n) // (1 + i % 7)).astype(np.uint8)
        out.append((d.tobytes(), deflate(d.tobytes(), (0, 1, 6, 9)[(i // 3) % 4])))
    return out


class BitWriter:
    """Deflate's bit order: fields LSB first, Huffman codes MSB first."""

    def __init__(self, head=b"\x78\x01"):
        self.out = bytearray(head)
        self.acc = self.n = 0

    def put(self, value, nbits):
        self.acc |= (value & ((1 << nbits) - 1)) << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8
        return self

    def code(self, code, nbits):
        for k in range(nbits - 1, -1, -1):
            self.put((code >> k) & 1, 1)
        return self

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)
        return self

    def raw(self, data):
        assert self.n == 0
        self.out += bytes(data)
        return self

    def done(self, pad=8):
        self.align()
        return bytes(self.out) + b"\0" * pad


def fixed_literal(w, v):
    return w.code(0x30 + v, 8) if v < 144 else w.code(0x190 + v - 144, 9)


def fixed_symbol(w, sym):          # 256 .. 287
    return w.code(sym - 256, 7) if sym < 280 else w.code(0xC0 + sym - 280, 8)


@functools.lru_cache(maxsize=None)
def bad_streams():
    """[(name, stream, expected)]: each must give OMR_INTERNAL, on the host and on the device."""
    rng = np.random.default_rng(16)
    data = rng.integers(0, 9, 5000, dtype=np.uint8).tobytes()
    good = deflate(data, 6)
    adler = zlib.adler32(b"hello").to_bytes(4, "big")
    out = [("empty stream", b"", 10)]
    cm7 = 0x7700 + (31 - 0x7700 % 31) % 31
    assert cm7 % 31 == 0 and not cm7 & 0x20
    out.append(("CM != 8", cm7.to_bytes(2, "big") + good[2:], 5000))
    out.append(("bad FCHECK", good[:1] + bytes([good[1] ^ 1]) + good[2:], 5000))
    assert 0x7820 % 31 == 0
    out.append(("FDICT set", b"\x78\x20" + b"\0\0\0\1" + good[2:], 5000))
    out.append(("block type 3", BitWriter().put(1, 1).put(3, 2).done(), 64))
    out.append(("stored LEN != ~NLEN", BitWriter().put(1, 1).put(0, 2).align().put(5, 16).put((~5 & 0xFFFF) ^ 1, 16)
                .raw(b"hello").raw(adler).done(0), 5))
    out.append(("HLIT = 287", BitWriter().put(1, 1).put(2, 2).put(30, 5).put(0, 5).put(0, 4).done(64), 64))
    w = BitWriter().put(1, 1).put(2, 2).put(0, 5).put(0, 5).put(0, 4)
    for _ in range(4):
        w.put(1, 3)                                      # 16, 17, 18 and 0: four codes of one bit
    out.append(("over-subscribed code lengths", w.done(64), 64))
    w = BitWriter().put(1, 1).put(2, 2).put(0, 5).put(0, 5).put(0, 4)
    for v in (1, 0, 0, 1):                               # 16 -> code 1, 0 -> code 0
        w.put(v, 3)
    w.code(1, 1).put(0, 2)                               # repeat the previous length: there is none
    out.append(("repeat code 16 first", w.done(64), 64))
    w = BitWriter().put(1, 1).put(2, 2).put(0, 5).put(0, 5).put(1, 4)
    for v in (0, 0, 0, 1, 1):                            # 0 -> code 0, 8 -> code 1
        w.put(v, 3)
    for _ in range(256):
        w.code(1, 1)                                     # 256 literals of 8 bits: a complete code
    w.code(0, 1).code(0, 1)                              # end-of-block and the one distance code: unused
    for v in b"hello":
        w.code(v, 8)
    out.append(("no end-of-block code", w.done(64), 5))
    w = BitWriter().put(1, 1).put(1, 2)
    fixed_symbol(fixed_literal(w, 0x61), 286)
    out.append(("litlen symbol 286", w.done(64), 64))
    w = BitWriter().put(1, 1).put(1, 2)
    fixed_symbol(fixed_literal(w, 0x61), 257).code(30, 5)
    out.append(("distance symbol 30", w.done(64), 64))
    w = BitWriter().put(1, 1).put(1, 2)
    fixed_symbol(fixed_literal(w, 0x61), 257).code(1, 5)  # length 3 at distance 2 after one byte
    fixed_symbol(w, 256)
    out.append(("distance before the start", w.done(64), 4))
    out.append(("cut in half", good[:len(good) // 2], 5000))
    out.append(("more than expected", good, 4999))
    out.append(("fewer than expected", good, 5001))
    co = zlib.compressobj(6)
    out.append(("final block missing", co.compress(data) + co.flush(zlib.Z_SYNC_FLUSH), 5000))
    out.append(("flipped Adler-32 byte", good[:-1] + bytes([good[-1] ^ 0xFF]), 5000))
    for name, s, e in out:
        try:
            ok = len(zlib.decompress(s)) == e
        except zlib.error:
            ok = False
        assert not ok, name
    return out
