"""The LZ4 blocks and Blosc chunks of the K15 tests (test_blosc_read_host.py, test_blosc_read_gpu.py):
golden streams of a real encoder (tests/golden/lz4_blocks.npz, made by tools/make_lz4_golden.py with
the system's liblz4), streams of the product's own encoders, and crafted ones written sequence by
sequence: the length and offset edges, the edges of K15a's emit stage (edge_streams) and a seeded
sweep (random_lz4_streams), each checked by lz4_decode_py where it is made.  Made once and shared;
nothing here needs a GPU."""
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
    res += edge_streams() + [random_lz4_streams(seed) for seed in range(16)]
    assert len({r[0] for r in res}) == len(res)
    return res


class Lz4Script:
    """Sequences and the data they stand for: the test chooses the sequences, the data is their
    replay.  A round is 64 sequences, as the device decoder collects them; `first` is where the
    round's first match is stored, `pos` where the last sequence's literals are, `ip` the stream's
    length so far."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.out = bytearray()
        self.seqs = []
        self.first = self.pos = self.ip = 0

    def seq(self, nlit, mlen, dist=None, start=None):
        """nlit new literals, then a match of mlen bytes `dist` back, or from output byte `start`."""
        self.pos = len(self.out)
        lits = self.rng.integers(0, 256, nlit, dtype=np.uint8).tobytes()
        self.out += lits
        mpos = len(self.out)
        if len(self.seqs) % 64 == 0:
            self.first = mpos
        if dist is None:
            dist = mpos - start
        assert 1 <= dist <= min(mpos, 65535) and mlen >= 4, (nlit, mlen, dist, mpos)
        for _ in range(mlen):
            self.out.append(self.out[-dist])
        self.seqs.append((lits, dist, mlen))
        self.ip += 1 + len(_length(15, nlit)) + nlit + 2 + len(_length(15, mlen - 4))
        return self

    def to_round(self, k):
        """Short sequences until the next one is sequence k of its round."""
        while len(self.seqs) % 64 != k:
            self.seq(1, 4, 1 + len(self.seqs) % 3)
        return self

    def end(self, nlit=0):
        lits = self.rng.integers(0, 256, nlit, dtype=np.uint8).tobytes()
        data, stream = bytes(self.out + lits), lz4_sequences(self.seqs + [(lits, 0, 0)])
        assert len(stream) == self.ip + 1 + len(_length(15, nlit)) + nlit
        assert lz4_decode_py(stream, len(data)) == data
        return data, stream


@functools.lru_cache(maxsize=None)
def edge_streams():
    """[(name, data, stream)]: the periods, thresholds, alignments and round borders of K15a's emit
    stage, each stream the replay of its own sequences."""
    out = []

    def add(name, s, tail=0):
        data, stream = s.end(tail)
        out.append((name, data, stream))

    # overlapped matches with real periods: 2 dist + 1 bytes, and long ones whose lanes step their phase
    # through four and more turns, free (the source is the sequence's own literals) and not, stored
    # at each of the four alignments
    for dist in (8, 9, 31, 63, 64, 65, 100, 127, 128, 129, 255, 256, 257, 300):
        s = Lz4Script(300 + dist)
        for a in range(4):
            for nlit, mlen in ((dist, 2 * dist + 1), (1, 1100 + 3 * a + dist % 7), (dist, 1150 + dist % 5)):
                s.seq(nlit + (a - len(s.out) - nlit) % 4, mlen, dist)
                assert (len(s.out) - mlen) % 4 == a
        add(f"period {dist}, short and long", s, dist % 4)

    s = Lz4Script(320)
    for mlen in (4, 5, 32, 33, 64, 65, 257):
        for dist in (mlen - 1, mlen, mlen + 1):
            s.seq(dist + 2, mlen, dist)                    # free: it reads its own sequence's literals
            s.seq(0, mlen, dist)                           # not free: it reads the match before it
            s.seq(1, mlen, dist)
    add("distance at, below and above the match length", s, 1)

    # the sizes at which a lane hands a copy to the wave: literal runs of 16 and 17, matches of 32 and 33
    s = Lz4Script(321).seq(40, 8, 40)
    for n in (16, 17):
        s.seq(n, 4, 3).seq(n, 32, 1).seq(n, 33, n)
    s.seq(270, 6, 270).seq(15, 7, 285)                     # extension bytes 255, 0 and 0
    for mlen in (32, 33):
        s.seq(mlen + 3, mlen, mlen + 3)                    # free, from its own literals
        s.seq(0, mlen, start=s.first - mlen)               # free, it ends where the round's first match begins
        s.seq(2, mlen, mlen + 1)                           # not free, from the match before it
        s.seq(0, mlen, 5)                                  # not free and overlapped
    add("copies of 16, 17, 32 and 33 bytes", s, 17)

    # wave_copy: every head, tail and source shift.  Literal runs stored at da and read at sa (mod 4): a
    # spacer sequence of a literals and a match of m bytes moves the two positions apart
    for n in range(17, 30):
        s = Lz4Script(330 + n).seq(8, 4, 8)
        for da in range(4):
            for sa in range(4):
                a, m = [(a, m) for a in range(4) for m in range(4, 8)
                        if (len(s.out) + a + m) % 4 == da and (s.ip + 3 + a + 2) % 4 == sa][0]
                s.seq(a, m, 1 + (da + sa) % 5)
                assert len(s.out) % 4 == da and (s.ip + 2) % 4 == sa
                s.seq(n, 4, 2)
        add(f"literal runs of {n} at every alignment", s, n)
    for mlen in range(33, 46):
        s = Lz4Script(350 + mlen).seq(64, 4, 64)
        for da in range(4):
            for sa in range(4):
                a = (da - len(s.out)) % 4
                mpos = len(s.out) + a
                s.seq(a, mlen, mlen + (mpos - sa - mlen) % 4)
                assert mpos % 4 == da and (mpos - s.seqs[-1][1]) % 4 == sa and s.seqs[-1][1] >= mlen
        add(f"matches of {mlen} at every alignment", s, 2)

    # the round's border: the closing sequence as the 63rd, 64th and 1st of a round, with literals and bare
    for total in (63, 64, 65, 128, 129):
        for tail in (0, 5):
            s = Lz4Script(370 + total)
            for k in range(total - 1):
                s.seq(k % 3 + 4 * (k == 0), 4 + k % 20, 1 + k % 4)
            assert len(s.seqs) + 1 == total
            add(f"{total} sequences, {tail} closing literals", s, tail)

    # the rule of the free match at its edges, for a match a lane copies and one the wave copies
    s = Lz4Script(380)

    def scene():
        return s.to_round(0).seq(40, 8, 40).seq(6, 4, 2)

    for mlen in (8, 40):
        for e in (0, 1):                                   # the source ends at the round's first match, and a byte above
            scene().seq(5, mlen, start=s.first + e - mlen)
        for e in (0, 1):                                   # it starts at its own literals, and a byte below
            scene()
            s.seq(mlen + 2, mlen, start=len(s.out) - e)
        scene()                                            # wholly in the literals of an earlier sequence
        p = len(s.out)
        s.seq(mlen + 4, 4, 1).seq(1, mlen, start=p + 1)
        scene()                                            # across a free match that a lane copied
        p = len(s.out)
        s.seq(6, 8, 6).seq(3, mlen, start=p + 2)
        scene().seq(3, 12, 5)                              # X, not free; then sources about its two ends
        x1 = len(s.out)
        x0 = x1 - 12
        s.seq(mlen, mlen, start=x1 - 1)                    # X's last byte and the literals above it
        s.seq(4, 4, start=x0 - 4).seq(4, mlen, start=x0 - 3).seq(5, mlen, start=x1 - 12)
        s.seq(3, mlen, start=x0 - 3 - 8)
    add("free and dependent matches at the rule's edges", s, 3)

    # the 256-byte window over the stream: tokens, offsets and the extension bytes of both lengths at every
    # phase of the stream, so that each falls on both sides of a reload at each source alignment
    for phase in range(33):                                # the pattern below repeats every 33 bytes
        s = Lz4Script(400 + phase).seq(8 + phase, 4, 8)
        for k in range(120):                               # no long literal run: the windows follow one another
            if k % 5 == 2:
                s.seq(0, 4 + 15 + 255 + 3, 1 + k % 7)      # extension bytes 255, 3
            elif k % 5 == 4:
                s.seq(15 + k % 3, 5, 6)                    # one extension byte
            else:
                s.seq(0, 4 + k % 11, 1 + k % 9)
        assert s.ip > 700
        add(f"window reloads, phase {phase}", s, phase % 3)
    return out


def lz4_census(stream):
    """What a good LZ4 block holds, by a plain parse of its own (nothing of the product): a dict of
      sequences   their number, the closing one included
      closing     (the closing sequence's index in its round of 64, its literals)
      matches     [(mlen, dist, mpos, free, start - pos, send - first)] with `free` by K15a's rule
                  (send <= first or start >= pos; first: where the round's first match is stored)
      sources     per match, what its source [start, send) touches of its own round, a set of
                  "earlier rounds", "literals" (of an earlier sequence), "own literals", "free lane
                  match" (free, of at most 32 bytes), "free wave match", "dependent match", and for
                  a dependent match it crosses into from below or leaves at the top, "dependent
                  match, its first byte" and "dependent match, its last byte"
      literals    {(run length, store position mod 4, position in the stream mod 4)}
      reloads     {mis: kinds of byte ("token", "lit ext", "offset 0", "offset 1", "match ext") on
                  which a 256-byte window over the stream's dwords, `mis` bytes behind a dword
                  boundary, is loaded anew}."""
    s, ip, out = bytes(stream), 0, 0
    reads, matches, literals, n, first = [], [], set(), 0, 0
    sources, spans, round_start = [], [], 0

    def ext(v, kind):
        nonlocal ip
        if v == 15:
            while True:
                reads.append((ip, kind))
                v += s[ip]
                ip += 1
                if s[ip - 1] != 255:
                    break
        return v

    while True:
        reads.append((ip, "token"))
        token = s[ip]
        ip += 1
        lit = ext(token >> 4, "lit ext")
        literals.add((lit, out % 4, ip % 4))
        if n % 64 == 0:
            spans, round_start = [], out
        pos, out, ip = out, out + lit, ip + lit
        n += 1
        if ip == len(s):
            break
        reads += [(ip, "offset 0"), (ip + 1, "offset 1")]
        dist = s[ip] | s[ip + 1] << 8
        ip += 2
        mlen = ext(token & 15, "match ext") + 4
        if n % 64 == 1:
            first = out
        start = out - dist
        send = start + min(mlen, dist)
        free = send <= first or start >= pos
        matches.append((mlen, dist, out, free, start - pos, send - first))
        seen = {"earlier rounds"} if start < round_start else set()
        for lo, hi, what in spans + [(pos, out, "own literals")]:
            if start < hi and lo < send and lo < hi:
                seen.add(what)
                if what == "dependent match":
                    seen |= {what + ", its first byte"} if start < lo else set()
                    seen |= {what + ", its last byte"} if hi < send else set()
        sources.append(seen)
        spans += [(pos, out, "literals"), (out, out + mlen, "dependent match" if not free else
                                           "free lane match" if mlen <= 32 else "free wave match")]
        out += mlen
    reloads = {}
    for mis in range(4):
        lo, kinds = None, set()
        for at, kind in reads:
            k = (mis + at) >> 2
            if lo is None or k < lo or k - lo >= 64:
                if lo is not None:
                    kinds.add(kind)
                lo = k
        reloads[mis] = kinds
    return {"sequences": n, "closing": ((n - 1) % 64, lit), "matches": matches, "sources": sources, "literals": literals,
            "reloads": reloads}


def random_lz4_streams(seed):
    """(name, data, stream): 100 .. 400 random sequences; offsets lean to 1 .. 70, to sources that
    begin about the round's first match, and to the largest there is."""
    s = Lz4Script(2000 + seed)
    rng = s.rng
    n = int(rng.integers(100, 401))
    s.seq(int(rng.integers(1, 80)), 4, 1)
    for _ in range(n - 2):
        nlit = int(rng.choice([0, 1, 15, 16, 17, int(rng.integers(0, 8)), int(rng.integers(0, 8)), int(rng.integers(0, 40))]))
        if rng.random() < 0.04:
            nlit = 270
        mlen = int(rng.choice([4, 19, 32, 33, 64, 65, int(rng.integers(4, 12)), int(rng.integers(4, 12)), int(rng.integers(4, 80))]))
        if rng.random() < 0.04:
            mlen = 274
        mpos = len(s.out) + nlit
        first = mpos if len(s.seqs) % 64 == 0 else s.first
        how, have = rng.random(), min(mpos, 65535)
        if how < 0.4:
            dist = int(rng.integers(1, 71))
        elif how < 0.7:
            dist = mpos - first - int(rng.integers(-mlen - 2, 40))
        elif how < 0.85:
            dist = have - int(rng.integers(0, 3))
        else:
            dist = int(rng.integers(1, have + 1))
        s.seq(nlit, mlen, max(1, min(dist, have)))
    data, stream = s.end(int(rng.choice([0, 1, 16, 17, 300])))
    assert len(s.seqs) + 1 == n
    return f"sweep {seed}", data, stream


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
