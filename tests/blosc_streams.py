"""The LZ4 blocks and Blosc chunks of the K15 tests (test_blosc_read_host.py, test_blosc_read_gpu.py):
golden streams of a real encoder (tests/golden/lz4_blocks.npz, made by tools/make_lz4_golden.py with
the system's liblz4), streams of the product's own encoders, and crafted ones written sequence by
sequence.  Made once and shared; nothing here needs a GPU."""
import functools
import os

import numpy as np

import omr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lz4_blocks.npz")


def _length(nibble_max, v):
    """The extension bytes of a length whose nibble holds min(v, 15)."""
    if v < nibble_max:
        return b""
    v -= nibble_max
    return b"\xff" * (v // 255) + bytes([v % 255])


def lz4_sequences(seqs):
    """An LZ4 block from [(literals, offset, match_len), ...]; match_len 0 (offset ignored) writes
    the literals alone, as the last sequence of a block is."""
    out = bytearray()
    for lits, offset, mlen in seqs:
        ml = mlen - 4 if mlen else 0
        assert mlen == 0 or mlen >= 4
        out.append(min(len(lits), 15) << 4 | min(ml, 15))
        out += _length(15, len(lits)) + bytes(lits)
        if mlen:
            out += int(offset).to_bytes(2, "little") + _length(15, ml)
    return bytes(out)


def lz4_decode_py(stream, expected):
    """The rule of omr_lz4_decode_host in plain Python: the data, or ValueError."""
    s, out, ip = bytes(stream), bytearray(), 0

    def ext(v):
        nonlocal ip
        if v == 15:
            while True:
                if ip >= len(s):
                    raise ValueError("extension past the input")
                b = s[ip]
                ip += 1
                v += b
                if b != 255:
                    break
        return v

    while True:
        if ip >= len(s):
            raise ValueError("input ends after a match")
        token = s[ip]
        ip += 1
        lit = ext(token >> 4)
        if lit > len(s) - ip or lit > expected - len(out):
            raise ValueError("literals")
        out += s[ip:ip + lit]
        ip += lit
        if ip == len(s):
            if len(out) != expected:
                raise ValueError("size")
            return bytes(out)
        if len(s) - ip < 2:
            raise ValueError("offset cut")
        off = s[ip] | s[ip + 1] << 8
        ip += 2
        if off == 0 or off > len(out):
            raise ValueError("offset")
        n = ext(token & 15) + 4
        if n > expected - len(out):
            raise ValueError("match past expected")
        for _ in range(n):
            out.append(out[-off])


@functools.lru_cache(maxsize=None)
def golden_streams():
    """[(name, data, stream)] of liblz4 1.9.3, default and HC."""
    z = np.load(GOLDEN)
    return [(str(n), z[str(n) + "__data"].tobytes(), z[str(n) + "__stream"].tobytes()) for n in z["names"]]


@functools.lru_cache(maxsize=None)
def crafted_streams():
    """[(name, data, stream)]: the length and offset edges, written by hand."""
    rng = np.random.default_rng(153)
    noise = rng.integers(0, 256, 70000, dtype=np.uint8).tobytes()
    out = []
    for n in (15, 15 + 255, 15 + 255 + 255):              # the last one: extension bytes 255, 255, 0
        out.append((f"literal run of {n}", lz4_sequences([(noise[:n], 0, 0)])))
    assert out[2][1][:4] == b"\xf0\xff\xff\x00"
    for n in (19, 19 + 255):
        out.append((f"match of {n}", lz4_sequences([(noise[:40], 33, n), (b"tail!", 0, 0)])))
    for off, n in ((1, 77), (3, 100), (7, 131), (3, 1001), (7, 4099), (1, 260), (2, 67), (5, 333)):
        out.append((f"offset {off}, match of {n}", lz4_sequences([(noise[100:100 + off + 2], off, n), (b"end", 0, 0)])))
    out.append(("offset 65535", lz4_sequences([(noise[:65535], 65535, 40), (noise[:7], 65535, 300), (b"12345", 0, 0)])))
    out.append(("match ends at expected", lz4_sequences([(b"abcdefgh", 8, 20), (b"", 0, 0)])))
    assert out[-1][1][-1] == 0
    # more than 64 sequences, matches that read the literals and matches of their own round
    seqs = []
    for k in range(150):
        seqs.append((noise[k * 5:k * 5 + 1 + k % 4], 1 + (k * 7) % (3 + k), 4 + k % 9))
    out.append(("150 short sequences", lz4_sequences(seqs + [(b"", 0, 0)])))
    seqs = [(noise[:20], 20, 30)] + [(b"", 3 + k, 40) for k in range(70)]
    out.append(("a chain of dependent matches", lz4_sequences(seqs + [(b"x", 0, 0)])))
    seqs = [(noise[:300], 300, 100), (noise[300:330], 17, 64), (noise[330:331], 430, 33), (noise[400:700], 1, 5)]
    out.append(("long and short mixed", lz4_sequences(seqs + [(noise[:17], 0, 0)])))
    res = []
    for name, s in out:
        # the size is what the sequences say: decode with a generous limit first
        total = len(lz4_decode_py_unbounded(s))
        res.append((name, lz4_decode_py(s, total), s))
    return res


def lz4_decode_py_unbounded(stream):
    for cap in (1 << 12, 1 << 17, 1 << 22):
        try:
            return _decode_upto(stream, cap)
        except OverflowError:
            continue
    raise AssertionError("crafted stream too large")


def _decode_upto(stream, cap):
    s, out, ip = bytes(stream), bytearray(), 0
    while True:
        token = s[ip]
        ip += 1
        lit = token >> 4
        if lit == 15:
            while True:
                b = s[ip]
                ip += 1
                lit += b
                if b != 255:
                    break
        out += s[ip:ip + lit]
        ip += lit
        if ip == len(s):
            return bytes(out)
        off = s[ip] | s[ip + 1] << 8
        ip += 2
        n = token & 15
        if n == 15:
            while True:
                b = s[ip]
                ip += 1
                n += b
                if b != 255:
                    break
        for _ in range(n + 4):
            out.append(out[-off])
        if len(out) > cap:
            raise OverflowError


@functools.lru_cache(maxsize=None)
def mixed_streams():
    """About 300 streams of the product's encoder for one call: [(data, stream)] (the size list of
    zarr_streams.mixed_streams)."""
    rng = np.random.default_rng(154)
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
        out.append((d.tobytes(), omr.lz4_encode(d.tobytes())))
    return out


@functools.lru_cache(maxsize=None)
def bad_streams():
    """[(name, stream, expected)]: each must give OMR_INTERNAL, on the host and on the device."""
    rng = np.random.default_rng(155)
    few = rng.integers(0, 5, 5000, dtype=np.uint8).tobytes()
    good = omr.lz4_encode(few)
    assert lz4_decode_py(good, 5000) == few and len(good) < 4500
    out = [("empty", b"", 10),
           ("offset 0", lz4_sequences([(b"abcd", 0, 8), (b"z", 0, 0)]), 13),
           ("offset one beyond the bytes produced", lz4_sequences([(b"abcd", 5, 8), (b"z", 0, 0)]), 13),
           ("literals past the input", b"\x50abc", 5),
           ("literals past expected", lz4_sequences([(b"0123456789", 0, 0)]), 5),
           ("match past expected", lz4_sequences([(b"abcd", 4, 20), (b"", 0, 0)]), 10),
           ("cut after the offset", lz4_sequences([(b"abcd", 4, 19)])[:-1], 23),
           ("cut inside a literal length extension", b"\xf0\xff", 600),
           ("cut inside a match length extension", lz4_sequences([(b"abcd", 4, 19 + 255 + 3)])[:-1], 4 + 19 + 255 + 3),
           ("ends after a match", lz4_sequences([(b"abcd", 4, 8)]), 12),
           ("one byte short of expected", good, 5001),
           ("one byte over expected", good, 4999),
           ("cut in half", good[:len(good) // 2], 5000)]
    for name, s, e in out:
        try:
            lz4_decode_py(s, e)
        except ValueError:
            continue
        raise AssertionError(name + " decodes")
    return out


def chunk_pixels(name, rng, shape):
    """Pixels whose high bytes compress and whose low bytes hardly do, as microscopy planes are."""
    if name.startswith("float"):
        a = np.round(rng.standard_normal(shape) * 50)
    else:
        a = rng.integers(0, 120, shape) + np.arange(shape[-1])[None, None, None, None, :] // 8
    return a.astype(name)


def layout_image(path):
    """One image whose chunks take every path of the container: [(what, plane, chunk file)].  Planes
    are channels of a 64 x 48 image with one chunk each (uint16: 6,144 bytes)."""
    rng = np.random.default_rng(162)
    a = chunk_pixels("uint16", rng, (1, 6, 1, 48, 64))
    a[0, 3] = rng.integers(0, 65536, (1, 48, 64))          # noise: written memcpyed
    a[0, 5] = 0                                            # left unwritten
    omr.write_zarr(path, a, chunk=(64, 48), compressor="blosc", dimension_separator=".", skip_zero_chunks=True)
    raw = [a[0, c, 0].astype("<u2").tobytes() for c in range(6)]
    files = [path / "0" / f"0.{c}.0.0.0" for c in range(6)]
    files[0].write_bytes(omr.blosc_encode(raw[0], 2, 1, 2048))            # three whole blocks
    files[1].write_bytes(omr.blosc_encode(raw[1], 2, 1, 4096))            # a whole block and a leftover, not split
    files[2].write_bytes(omr.blosc_encode(raw[2], 2, 0, 512))             # twelve blocks of two splits, not shuffled
    files[3].write_bytes(omr.blosc_encode(raw[3], 2, 1, 0, memcpy=True))
    # files[4]: the writer's own chunk; its low-byte split does not compress
    c4 = files[4].read_bytes()
    at = int.from_bytes(c4[16:20], "little")
    low = int.from_bytes(c4[at:at + 4], "little")          # "<u2" shuffled: the low bytes come first
    high = int.from_bytes(c4[at + 4 + low:at + 8 + low], "little")
    assert high < 3072 and low == 3072, "the low-byte split is stored raw"
    assert not files[5].exists()
    c1 = files[1].read_bytes()
    n1 = int.from_bytes(c1[20:24], "little")
    assert int.from_bytes(c1[16:20], "little") == 24 and n1 + 4 + int.from_bytes(c1[n1:n1 + 4], "little") == len(c1)
    return a, files
