"""The zlib streams of the K14 tests (test_zarr_read_host.py, test_zarr_read_gpu.py): good ones made
with the stdlib zlib, bad ones written bit by bit, and the forms of RFC 1951 that the stdlib
compressor never writes (rare_streams, random_deflate_streams), written by a small Deflate writer
from tokens and code lengths the tests choose.  Every good stream is checked against
zlib.decompress where it is made, every bad one is one zlib.decompress refuses; deflate_census
counts what a stream holds.  Nothing here needs a GPU, and nothing of the product takes part."""
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


# ---- a Deflate writer: the tokens and the code lengths are given, nothing is searched or optimised ----

ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)          # RFC 1951 3.2.7
LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]               # length symbols 257 .. 285
LBASE = [3 + k for k in range(8)] + [3 + ((4 + (i & 3)) << ((i - 4) >> 2)) for i in range(8, 28)] + [258]
DEXT = [0] * 4 + [(s - 2) >> 1 for s in range(4, 30)]                               # distance symbols 0 .. 29
DBASE = [1, 2, 3, 4] + [1 + ((2 + (s & 1)) << ((s - 2) >> 1)) for s in range(4, 30)]
assert LBASE[8:12] == [11, 13, 15, 17] and LBASE[27] == 227 and DBASE[4:8] == [5, 7, 9, 13] and DBASE[29] == 24577
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DL = [5] * 32


def length_symbol(n):
    """(symbol, extra bits, their value) of a match length; 258 is symbol 285, never 284 + 31."""
    i = 28 if n == 258 else max(k for k in range(28) if LBASE[k] <= n)
    assert 0 <= n - LBASE[i] < 1 << LEXT[i] or n == 258
    return 257 + i, LEXT[i], n - LBASE[i]


def distance_symbol(d):
    s = max(k for k in range(30) if DBASE[k] <= d)
    assert 0 <= d - DBASE[s] < 1 << DEXT[s]
    return s, DEXT[s], d - DBASE[s]


def leaf_lengths(n, maxlen, deep=1.0, rng=None):
    """The lengths of a complete code of n >= 2 codes, by splitting leaves: from one leaf, a leaf
    below maxlen becomes two that are one longer, n - 1 times.  `deep` is the share of the splits
    that take the deepest leaf there is (1.0: the chain 1, 2, 3, ..., so maxlen is reached as soon
    as n allows); the others take a leaf drawn from rng."""
    assert 2 <= n <= 1 << maxlen
    leaves = [0]
    while len(leaves) < n:
        can = [k for k, l in enumerate(leaves) if l < maxlen]      # never empty below 2^maxlen leaves
        if rng is None or rng.random() < deep:
            k = max(can, key=lambda q: leaves[q])
        else:
            k = can[int(rng.integers(0, len(can)))]
        leaves[k] += 1
        leaves.append(leaves[k])
    assert sum(1 << (15 - l) for l in leaves) == 1 << 15, "not complete"
    return sorted(leaves)


def assign(symbols, lengths, size):
    """`size` code lengths: symbols[k] takes lengths[k], the others none."""
    assert len(symbols) == len(lengths) == len(set(symbols))
    out = [0] * size
    for s, l in zip(symbols, lengths):
        out[s] = l
    return out


def canonical(lens):
    """[(code, length)] by symbol, the canonical code of RFC 1951 3.2.2 (length 0: None)."""
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = []
    for l in lens:
        out.append((nxt[l], l) if l else None)
        nxt[l] += 1 if l else 0
    return out


def pack_lengths(seq, use=(16, 17, 18), prev=None):
    """A code length sequence as items (symbol, extra value) with the repeat symbols in `use`, run
    by run; `prev` is the length before seq[0] when the run may go on from it."""
    items, k = [], 0
    while k < len(seq):
        v, n = seq[k], 1
        while k + n < len(seq) and seq[k + n] == v:
            n += 1
        k += n
        while n:
            if v == 0 and n >= 11 and 18 in use:
                r = min(n, 138)
                items.append((18, r - 11))
            elif v == 0 and n >= 3 and 17 in use:
                r = min(n, 10)
                items.append((17, r - 3))
            elif v and prev == v and n >= 3 and 16 in use:
                r = min(n, 6)
                items.append((16, r - 3))
            else:
                r = 1
                items.append((v, 0))
            prev = v
            n -= r
    return items


def unpack_lengths(items):
    out = []
    for sym, extra in items:
        if sym < 16:
            out.append(sym)
        elif sym == 16:
            out += [out[-1]] * (3 + extra)
        else:
            out += [0] * ((3 if sym == 17 else 11) + extra)
    return out


def write_tokens(w, tokens, ll, dl, eob=True):
    """Tokens under the codes of the lengths ll and dl: b (a literal), (length, distance),
    ("sym", s) (a bare literal/length symbol) or ("raw", value, nbits)."""
    lc, dc = canonical(ll), canonical(dl)
    for t in tokens:
        if isinstance(t, int):
            w.code(*lc[t])
        elif t[0] == "sym":
            w.code(*lc[t[1]])
        elif t[0] == "raw":
            w.put(t[1], t[2])
        else:
            s, nb, v = length_symbol(t[0])
            w.code(*lc[s]).put(v, nb)
            s, nb, v = distance_symbol(t[1])
            w.code(*dc[s]).put(v, nb)
    if eob:
        w.code(*lc[256])
    return w


def write_dynamic(w, tokens, ll, dl, items=None, cl=None, hclen=None, check=True, eob=True):
    """A dynamic block's header and tokens.  ll and dl are the code lengths (HLIT = len(ll), HDIST =
    len(dl)); `items` is their packing (default: pack_lengths of each, as zlib packs), `cl` the 19
    lengths of the code-length code (default: a chain over the symbols the items use) and `hclen`
    how many of them are sent (default: as few as the format allows).  check=False writes what a
    decoder must refuse."""
    if items is None:
        items = pack_lengths(ll) + pack_lengths(dl)
    if cl is None:
        used = sorted({s for s, _ in items})
        cl = assign(used, leaf_lengths(len(used), 7) if len(used) > 1 else [1], 19)
    if hclen is None:
        hclen = max(4, 1 + max(k for k in range(19) if cl[ORDER[k]]))
    if check:
        assert unpack_lengths(items) == list(ll) + list(dl), "the items are not the lengths"
        assert 257 <= len(ll) <= 286 and 1 <= len(dl) <= 30 and ll[256]
        assert all(cl[s] for s, _ in items) and not any(cl[ORDER[k]] for k in range(hclen, 19))
    w.put(len(ll) - 257, 5).put(len(dl) - 1, 5).put(hclen - 4, 4)
    for k in range(hclen):
        w.put(cl[ORDER[k]], 3)
    cc = canonical(cl)
    for sym, extra in items:
        w.code(*cc[sym]).put(extra, {16: 2, 17: 3, 18: 7}.get(sym, 0))
    return write_tokens(w, tokens, ll, dl, eob)


def codes_for(tokens, rng=None, maxlen=15, deep=1.0, spare=0):
    """Code lengths (ll, dl) that cover the tokens: complete codes by leaf_lengths over the symbols
    used and `spare` unused ones, the lengths dealt to the symbols in an order drawn from rng."""
    ls, ds = {256}, set()
    for t in tokens:
        if isinstance(t, int):
            ls.add(t)
        elif t[0] == "sym":
            ls.add(t[1])
        elif t[0] != "raw":
            ls.add(length_symbol(t[0])[0])
            ds.add(distance_symbol(t[1])[0])

    def deal(used, size, least):
        used = sorted(used)
        free = [s for s in range(size) if s not in used]
        if rng is not None:
            free = [free[k] for k in rng.permutation(len(free))]
        used += free[:max(spare, least - len(used))]
        if rng is not None:
            used = [used[k] for k in rng.permutation(len(used))]
        lens = assign(used, leaf_lengths(len(used), max(maxlen, (len(used) - 1).bit_length()), deep, rng), size)
        while len(lens) > 1 and lens[-1] == 0:
            lens.pop()
        return lens

    ll = deal(ls, 286, 2)
    ll += [0] * (257 - len(ll))
    dl = deal(ds, 30, 2) if ds else [0]
    return ll, dl


def deflate_blocks(blocks, head=b"\x78\x01", data=None, phases=None, finish=True):
    """A zlib stream of [("stored", bytes) | ("fixed", tokens) | ("dynamic", tokens, options of
    write_dynamic)], the last one final, and the Adler-32 of `data`.  The bit phase at which each
    stored block's header ends is appended to `phases`.  finish=False: the BitWriter as it stands
    behind the last block."""
    w = BitWriter(head)
    for k, b in enumerate(blocks):
        w.put(int(k == len(blocks) - 1), 1)
        if b[0] == "stored":
            w.put(0, 2)
            if phases is not None:
                phases.append(w.n)
            w.align().put(len(b[1]), 16).put(len(b[1]) ^ 0xFFFF, 16).raw(b[1])
        elif b[0] == "fixed":
            write_tokens(w.put(1, 2), b[1], FIXED_LL, FIXED_DL)
        else:
            opts = dict(b[2]) if len(b) > 2 else {}
            if "ll" not in opts:
                opts["ll"], opts["dl"] = codes_for(b[1])
            write_dynamic(w.put(2, 2), b[1], opts.pop("ll"), opts.pop("dl"), **opts)
    if not finish:
        return w
    return w.align().raw(zlib.adler32(data).to_bytes(4, "big")).done(0)


class Script:
    """Blocks of tokens and the data they stand for: the test chooses the tokens, the data is their
    replay.  A batch is 64 symbols of one Huffman block, as the device decoder collects them."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.out = bytearray()
        self.blocks = []
        self.tok = self.at = None

    def begin(self, kind, **opts):
        self.tok, self.at = [], []
        self.blocks.append((kind, self.tok, opts))
        return self

    def lit(self, n=1, values=256):
        for _ in range(n):
            self.byte(int(self.rng.integers(0, values)))
        return self

    def byte(self, b):
        self.at.append(len(self.out))
        self.tok.append(b)
        self.out.append(b)
        return self

    def match(self, length, dist):
        assert 3 <= length <= 258 and 1 <= dist <= min(len(self.out), 32768), (length, dist, len(self.out))
        self.at.append(len(self.out))
        self.tok.append((length, dist))
        for _ in range(length):
            self.out.append(self.out[-dist])
        return self

    def stored(self, n):
        data = self.rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        self.blocks.append(("stored", data))
        self.out += data
        self.tok = self.at = None
        return self

    def batch_start(self):
        """The output position at which the batch of the next token begins."""
        k = len(self.tok) // 64 * 64
        return self.at[k] if k < len(self.tok) else len(self.out)

    def to_batch(self, k, values=256):
        """Literals until the next token is symbol k of its batch."""
        while len(self.tok) % 64 != k:
            self.lit(1, values)
        return self

    def source_end(self, length, end):
        """A match of `length` (not overlapping) whose source ends `end` bytes above its batch's
        first byte."""
        dist = len(self.out) + length - self.batch_start() - end
        assert dist >= length
        return self.match(length, dist)

    def stream(self, **kw):
        data = bytes(self.out)
        s = deflate_blocks(self.blocks, data=data, **kw)
        assert zlib.decompress(s) == data
        return data, s


def closed(w, data):
    """The stream of a writer that stands behind its final block, with the Adler-32 of `data`."""
    return w.align().raw(zlib.adler32(data).to_bytes(4, "big")).done(0)


def _add(out, name, script, **kw):
    data, s = script.stream(**kw)
    out.append((name, data, s))


# the pairs at 2 .. 14 and four codes of 15 bits: 30 codes, from the chain 1, 2, ..., 15, 15 by splitting each single leaf
PAIRS_30 = [l for l in range(2, 15) for _ in (0, 1)] + [15] * 4


@functools.lru_cache(maxsize=None)
def rare_streams():
    """[(name, data, stream)]: what RFC 1951 allows and the stdlib compressor never writes."""
    out = []

    # the chain 1, 2, ..., 14, 15, 15 over fifteen literals and the end-of-block code (at 15 bits); no
    # distance code; HCLEN = 19 and a code-length code of all nineteen symbols, down to 7 bits
    s = Script(200).begin("dynamic")
    vals = [int(v) for v in s.rng.permutation(256)[:15]]
    for k in range(300):
        s.byte(vals[k % 15] if k < 30 else vals[int(s.rng.integers(0, 15))])
    ll = assign(vals + [256], leaf_lengths(16, 15), 257)
    items = pack_lengths(ll) + pack_lengths([0])
    rare = [c for c in range(19) if c not in {c for c, _ in items}]
    used = sorted({c for c, _ in items}, key=lambda c: sum(1 for q, _ in items if q == c))
    cl = assign(rare + used, leaf_lengths(19, 7), 19)        # the symbols the header uses most get the longest codes
    s.blocks[0][2].update(ll=ll, dl=[0], items=items, cl=cl, hclen=19)
    _add(out, "litlen chain 1..15, HCLEN 19", s)

    # 286 literal/length codes, most of them of 15 bits, all decoded; the distance code of PAIRS_30 with
    # all 30 symbols; every length and distance symbol with its extra bits all zeros and all ones;
    # length 258 at distance 32768 from the first byte of the output; 15 + 5 + 15 + 13 bits back to back
    s = Script(201).stored(32768).begin("dynamic")
    s.match(258, 32768)
    lengths = [LBASE[i] + e for i in range(29) for e in sorted({0, (1 << LEXT[i]) - 1})]
    lengths[lengths.index(258)] = 257                        # 284 with 31 is not valid: 258 is symbol 285
    assert lengths.count(258) == 1 and length_symbol(257) == (284, 5, 30)
    dists = [DBASE[i] + e for i in range(30) for e in sorted({0, (1 << DEXT[i]) - 1})]
    for k in range(max(len(lengths), len(dists))):
        s.lit(1 + k % 3).match(lengths[k % len(lengths)], dists[k % len(dists)])
    for l in (LBASE[26] + 31, LBASE[24], LBASE[27] + 30):
        s.match(l, 32768).match(l, DBASE[28] + 8191)         # symbols 283, 281, 284 and 29, 28: the longest codes
    for b in s.rng.permutation(256):
        s.byte(int(b))
    ll_lens = leaf_lengths(286, 15, 0.85, s.rng)
    assert ll_lens.count(15) >= 150                          # ranks in sorted[] up to 285
    order = [int(v) for v in s.rng.permutation(257)] + list(range(257, 281)) + [285, 282, 281, 283, 284]
    s.blocks[-1][2].update(ll=assign(order, ll_lens, 286),
                           dl=assign([int(v) for v in s.rng.permutation(28)] + [28, 29], PAIRS_30, 30))
    opts = s.blocks[-1][2]
    assert all(opts["ll"][c] == 15 for c in (281, 283, 284)) and opts["dl"][28] == opts["dl"][29] == 15
    _add(out, "every match symbol, deep codes", s)

    # the chain over sixteen distance symbols (1 .. 15 bits, each decoded) and a flat literal/length code
    s = Script(202).begin("dynamic").lit(600)
    dsyms = [int(v) for v in s.rng.permutation(18)[:16]]
    for k in range(64):
        s.lit(k % 2).match(3 + k % 9, DBASE[dsyms[k % 16]])
    ll, _ = codes_for(s.tok, s.rng, 9, 0.0)
    s.blocks[0][2].update(ll=ll, dl=assign(dsyms, leaf_lengths(16, 15), 18))
    _add(out, "distance chain 1..15", s)

    # the smallest headers: HCLEN = 6 with lengths of 0, 7 and 8 only, and HCLEN = 5 with 0 and 8
    s = Script(203).begin("dynamic")
    vals = [int(v) for v in s.rng.permutation(256)[:254]]
    for k in range(400):
        s.byte(vals[k % 254])
    ll = assign(vals + [256], [8] * 254 + [7], 257)
    s.blocks[0][2].update(ll=ll, dl=[0], items=[(v, 0) for v in ll + [0]], cl=assign([0, 7, 8], [2, 2, 1], 19))
    _add(out, "HCLEN 6", s)
    s = Script(204).begin("dynamic")
    vals = [int(v) for v in s.rng.permutation(256)[:255]]
    for k in range(400):
        s.byte(vals[k % 255])
    ll = assign(vals + [256], [8] * 256, 257)
    s.blocks[0][2].update(ll=ll, dl=[0], items=[(v, 0) for v in ll + [0]], cl=assign([0, 8], [1, 1], 19))
    _add(out, "HCLEN 5", s)

    # repeats that begin among the literal/length lengths and end among the distance lengths
    for sym in (16, 17, 18, "16 of the last literal/length length"):
        s = Script(205).begin("dynamic").lit(300, 7)
        for k in range(40):
            s.lit(k % 3, 7).match(3 + k % 6, 21 + k % 12)    # length symbols 257 .. 262, distance symbols 8 and 9
        if sym == 17 or sym == 18:
            # 263 .. 285 unused, and the distance symbols 0 .. 7: one run of zeros over the border
            hlit, zeros = (265, 10) if sym == 17 else (286, 31)
            ll = assign(list(range(7)) + list(range(256, 263)), leaf_lengths(14, 6, 0.5, s.rng), hlit)
            dl = [0] * 8 + [1, 1]
            items = pack_lengths(ll[:263]) + [(sym, zeros - (3 if sym == 17 else 11))] + [(1, 0), (1, 0)]
            assert hlit - 263 + 8 == zeros
        else:
            # 257 .. 262 and the distance symbols 0 .. 9 all of 4 bits: one run over the border
            ll = assign(list(range(7)) + list(range(256, 263)), [3, 3] + [4] * 12, 263)
            dl = [4] * 10 + [3, 3, 3]
            assert sum(1 << (15 - l) for l in ll if l) == 1 << 15 and sum(1 << (15 - l) for l in dl) == 1 << 15
            if sym == 16:
                items = pack_lengths(ll[:259]) + [(16, 3), (16, 3), (4, 0), (4, 0)] + pack_lengths(dl[10:])
            else:
                items = pack_lengths(ll) + [(16, 3), (16, 1)] + pack_lengths(dl[10:])
        s.blocks[0][2].update(ll=ll, dl=dl, items=items)
        _add(out, f"repeat {sym} over the border", s)

    # degenerate sets: literals only and no distance code; one distance code of one bit, used; a block of
    # nothing but a one-bit end-of-block code
    s = Script(206).begin("dynamic").lit(500, 40)
    ll, _ = codes_for(s.tok, s.rng, 12, 0.5)
    s.blocks[0][2].update(ll=ll, dl=[0])
    _add(out, "no distance code", s)
    s = Script(207).begin("dynamic").lit(20)
    for k in range(100):
        s.lit(k % 4 == 0).match(3 + k % 40, 7 + k % 2)       # distance symbol 5 and its extra bit
    ll, _ = codes_for(s.tok, s.rng, 10, 0.5)
    s.blocks[0][2].update(ll=ll, dl=[0] * 5 + [1])
    _add(out, "a single distance code of one bit", s)
    s = Script(208).begin("fixed").lit(10).begin("dynamic", ll=[0] * 256 + [1], dl=[0]).begin("fixed").lit(10)
    _add(out, "a block of a one-bit end-of-block code", s)

    # overlapping matches: distance p below the length, first of a batch (copied by one lane, k mod p)
    # and deep inside one (copied by the wave)
    for name, periods in (("1..24", range(1, 25)), ("25..48", range(25, 49)), ("49..70", range(49, 71)),
                          ("127..257", (127, 128, 129, 255, 256, 257))):
        s = Script(209).begin("dynamic").lit(260)
        for p in periods:
            ls = [l for l in sorted({max(3, p + 1), 63, 64, 65, 127, 128, 129, 258}) if l > p]
            for k, l in enumerate(ls):
                s.lit(1 + (k + p) % 5).match(l, p)
            s.to_batch(0).match(ls[p % len(ls)], p).match(258, p)
            s.lit(p % 7).to_batch(0).match(ls[(p + 1) % len(ls)], p)
        ll, dl = codes_for(s.tok, s.rng, 11, 0.3)
        s.blocks[0][2].update(ll=ll, dl=dl)
        _add(out, f"overlapping matches, periods {name}", s)

    # what a match may read of its own batch
    s = Script(210).begin("dynamic").lit(400)
    for end in (0, -1, 1, 0, 1, -1):
        for at in (0, 1, 17, 63):                            # the match as symbol `at` of its batch
            for length in (3, 40):
                if at or end <= 0:                           # the first symbol's source cannot end above it
                    s.lit(1).to_batch(at).source_end(length, end)
    for end in (0, 1, -1):                                   # the batch's first byte is itself a match's
        for at in (1, 30):
            s.lit(1).to_batch(0).match(4 + at % 4, 7).to_batch(at).source_end(6, end)
    for k in range(6):                                       # chains: each match reads the one before
        s.to_batch(5 * k).lit(3)
        for j in range(3 + k):
            s.match(4 + 9 * j + k, 3 + j + k)
        s.lit(1).match(5, 1).match(20, 4).match(100, 22).match(258, 130)
    for k in range(8):                                       # a match that reads literals of its own batch
        s.to_batch(8 * k).lit(10).match(3 + k, 3 + k).lit(2).match(9, 11 + k)
    ll, dl = codes_for(s.tok, s.rng, 12, 0.3)
    s.blocks[0][2].update(ll=ll, dl=dl)
    _add(out, "matches that read their own batch", s)

    # blocks of 62 .. 65 and 127 .. 129 symbols before the end-of-block code: it falls last in a batch,
    # first in one, and alone in one
    s = Script(211).begin("fixed").lit(100, 30)
    for k, n in enumerate((62, 63, 64, 65, 127, 128, 129, 64, 63)):
        s.begin("dynamic" if k % 3 else "fixed")
        while len(s.tok) < n:
            if len(s.tok) % 5 == 4:
                s.match(3 + len(s.tok) % 30, 1 + (len(s.tok) * 7) % 90)
            else:
                s.lit(1, 30)
    _add(out, "blocks that end at the batch border", s)

    # stored blocks: empty between Huffman blocks, of 65535 bytes, behind a block that ends at each bit
    # phase, and matches that reach back across them
    s = Script(212).begin("fixed").lit(50, 20)
    s.stored(0).begin("dynamic").lit(30, 20).match(40, 60).stored(0).stored(0).begin("fixed").match(10, 100)
    _add(out, "empty stored blocks between Huffman blocks", s)
    s = Script(213).begin("fixed").lit(9).stored(65535).begin("dynamic").match(258, 65535 - 40000).match(258, 32768).lit(5)
    _add(out, "a stored block of 65535 bytes", s)
    s, phases = Script(214), []
    for k in range(8):
        s.begin("fixed").lit(3, 100)
        for _ in range(k):
            s.byte(200 + k)                                  # 9-bit codes: one more bit each
        s.stored(23 + k)
    s.begin("dynamic").match(30, 31).match(258, 200).lit(4)
    data, st = s.stream(phases=phases)
    assert sorted(phases) == list(range(8)), phases
    out.append(("stored blocks at every bit phase", data, st))

    # the fixed tables, overwritten by a dynamic block, are wanted again
    s = Script(215).begin("fixed").lit(80, 256)
    for k in range(30):
        s.match(3 + k, 1 + 2 * k)
    s.begin("dynamic").lit(200, 12)
    for k in range(30):
        s.match(4 + 5 * k, 5 + 9 * k)
    s.begin("fixed").lit(40, 256)
    for k in range(60):
        s.lit(k % 2).match(3 + (k * 37) % 256, 1 + (k * 53) % 500)
    s.stored(10).begin("fixed").lit(10).match(258, 300).begin("dynamic").lit(70, 5).begin("fixed").match(100, 3)
    _add(out, "fixed, dynamic, fixed", s)

    # windows below 32 KiB: CINFO 1 .. 6
    rng = np.random.default_rng(216)
    few = rng.integers(0, 9, 6000, dtype=np.uint8).tobytes()
    for wbits in range(9, 15):
        co = zlib.compressobj(6, zlib.DEFLATED, wbits)
        st = co.compress(few) + co.flush()
        assert st[0] == (wbits - 8) << 4 | 8
        out.append((f"window of {1 << wbits} bytes", few, st))
    for name, data, st in out:
        assert zlib.decompress(st) == data, name
        assert len(data) <= 72000, name
    assert len({o[0] for o in out}) == len(out)
    return out


def random_deflate_streams(seed):
    """(name, data, stream): a few fixed, dynamic and stored blocks of 200 .. 3000 random tokens in
    all, under random complete codes whose longest length is drawn from 7 .. 15.  Distances lean to
    1 .. 70, to sources that end about their batch's first byte, and to the full 32 KiB."""
    s = Script(1000 + seed)
    rng = s.rng
    if seed % 2:
        s.stored(32768 + int(rng.integers(0, 300)))
    total = int(rng.integers(200, 3001))
    values = int(rng.choice([3, 20, 256]))
    while total > 0:
        kind = ("dynamic", "fixed", "dynamic", "stored")[int(rng.integers(0, 4))]
        if kind == "stored":
            s.stored(int(rng.choice([0, 1, 7, 100, 1000])))
            continue
        n = min(total, int(rng.integers(1, 900)))
        total -= n
        s.begin(kind)
        for _ in range(n):
            if len(s.out) < 3 or rng.random() < 0.45:
                s.lit(1, values)
                continue
            length = int(rng.choice([3, 4, 5, 8, 17, 63, 64, 65, 130, 257, 258, int(rng.integers(3, 259))]))
            if len(s.out) > 50000:                           # the stream's data stays at about 70 KB
                length = 3 + length % 6
            how, have = rng.random(), min(len(s.out), 32768)
            if how < 0.35:
                dist = int(rng.integers(1, 71))
            elif how < 0.6:
                dist = len(s.out) + min(length, 40) - s.batch_start() - int(rng.integers(-1, 2))
            elif how < 0.8:
                dist = have - int(rng.integers(0, 3))
            else:
                dist = int(rng.integers(1, have + 1))
            s.match(length, max(1, min(dist, have)))
        if kind == "dynamic":
            ll, dl = codes_for(s.tok, rng, int(rng.integers(7, 16)), float(rng.choice([0.2, 0.6, 0.9])), int(rng.integers(0, 6)))
            s.blocks[-1][2].update(ll=ll, dl=dl)
    if s.blocks[-1][0] == "stored" and rng.random() < 0.5:
        s.begin("fixed")
    data, st = s.stream()
    return f"sweep {seed}", data, st


@functools.lru_cache(maxsize=None)
def sweep_streams():
    return [random_deflate_streams(seed) for seed in range(16)]


# ---- a census: a plain inflater that counts what the streams hold -----------------------------------

def _puff_tables(lens):
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    offs = [0] * 17
    for l in range(1, 16):
        offs[l + 1] = offs[l] + count[l]
    symbol = [0] * max(1, sum(count))
    for k, l in enumerate(lens):
        if l:
            symbol[offs[l]] = k
            offs[l] += 1
    return count, symbol


def deflate_census(stream):
    """What a good zlib stream holds, by a bit-by-bit inflater of its own (RFC 1951 read plainly, no
    tables, nothing of the product): a dict of
      blocks            {type: count}
      litlen_bits, dist_bits, codelen_bits   {code length: symbols decoded at it}
      length_symbols, distance_symbols       {symbol: set of extra-bit values decoded}
      hclen             set of HCLEN values (4 .. 19)
      overlaps          set of distances below their match's length
      crossing_repeats  set of 16/17/18 whose run begins below HLIT and ends above it
      repeats_at_hlit   set of 16/17/18 whose run begins at HLIT exactly (a 16 there copies the last
                        literal/length length into distance lengths only)
      distance_sets     set of "empty" / "single" (a dynamic block's distance code of no or one code)
      data              the inflated bytes."""
    s = bytes(stream)
    assert s[0] & 15 == 8 and (s[0] << 8 | s[1]) % 31 == 0 and not s[1] & 0x20
    pos = 16
    c = {"blocks": {}, "litlen_bits": {}, "dist_bits": {}, "codelen_bits": {}, "length_symbols": {},
         "distance_symbols": {}, "hclen": set(), "overlaps": set(), "crossing_repeats": set(), "repeats_at_hlit": set(),
         "distance_sets": set()}
    out = bytearray()

    def bits(n):
        nonlocal pos
        assert pos + n <= 8 * len(s), "the stream ends early"
        v = (int.from_bytes(s[pos >> 3:(pos >> 3) + 4], "little") >> (pos & 7)) & ((1 << n) - 1)
        pos += n
        return v

    def decode(table, tally):
        count, symbol = table
        code = first = index = 0
        for l in range(1, 16):
            code |= bits(1)
            if code - count[l] < first:
                tally[l] = tally.get(l, 0) + 1
                return symbol[index + code - first]
            index += count[l]
            first = (first + count[l]) << 1
            code <<= 1
        raise AssertionError("no such code")

    last = 0
    while not last:
        last, kind = bits(1), bits(2)
        c["blocks"][kind] = c["blocks"].get(kind, 0) + 1
        assert kind < 3
        if kind == 0:
            pos = (pos + 7) & ~7
            n = bits(16)
            assert bits(16) == n ^ 0xFFFF and (pos >> 3) + n <= len(s)
            out += s[pos >> 3:(pos >> 3) + n]
            pos += 8 * n
            continue
        if kind == 1:
            lit, dist = _puff_tables(FIXED_LL), _puff_tables(FIXED_DL)
        else:
            hlit, hdist, hclen = bits(5) + 257, bits(5) + 1, bits(4) + 4
            c["hclen"].add(hclen)
            cl = [0] * 19
            for k in range(hclen):
                cl[ORDER[k]] = bits(3)
            table, lens = _puff_tables(cl), []
            while len(lens) < hlit + hdist:
                sym = decode(table, c["codelen_bits"])
                if sym < 16:
                    lens.append(sym)
                    continue
                rep = 3 + bits(2) if sym == 16 else 3 + bits(3) if sym == 17 else 11 + bits(7)
                if len(lens) < hlit < len(lens) + rep:
                    c["crossing_repeats"].add(sym)
                if len(lens) == hlit:
                    c["repeats_at_hlit"].add(sym)
                lens += [lens[-1] if sym == 16 else 0] * rep
            assert len(lens) == hlit + hdist and lens[256]
            used = [l for l in lens[hlit:] if l]
            if not used:
                c["distance_sets"].add("empty")
            elif used == [1]:
                c["distance_sets"].add("single")
            lit, dist = _puff_tables(lens[:hlit]), _puff_tables(lens[hlit:])
        while True:
            sym = decode(lit, c["litlen_bits"])
            if sym < 256:
                out.append(sym)
                continue
            if sym == 256:
                break
            assert sym <= 285
            e = bits(LEXT[sym - 257])
            c["length_symbols"].setdefault(sym, set()).add(e)
            n = LBASE[sym - 257] + e
            ds = decode(dist, c["dist_bits"])
            assert ds <= 29
            e = bits(DEXT[ds])
            c["distance_symbols"].setdefault(ds, set()).add(e)
            d = DBASE[ds] + e
            assert d <= len(out) and n <= 258
            if d < n:
                c["overlaps"].add(d)
            for _ in range(n):
                out.append(out[-d])
    pos = (pos + 7) & ~7
    assert int.from_bytes(s[pos >> 3:(pos >> 3) + 4], "big") == zlib.adler32(bytes(out)) and (pos >> 3) + 4 <= len(s)
    c["data"] = bytes(out)
    return c


def merge_census(parts):
    tot = {}
    for c in parts:
        for key, v in c.items():
            if key == "data":
                continue
            if isinstance(v, set):
                tot.setdefault(key, set()).update(v)
            elif key in ("length_symbols", "distance_symbols"):
                for sym, e in v.items():
                    tot.setdefault(key, {}).setdefault(sym, set()).update(e)
            else:
                for k, n in v.items():
                    tot.setdefault(key, {})
                    tot[key][k] = tot[key].get(k, 0) + n
    return tot


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
    # code sets, repeats and distances that no encoder at hand gets wrong
    dyn = lambda: BitWriter().put(1, 1).put(2, 2)
    four = assign([0x61, 0x62, 256, 257], [2, 2, 2, 2], 258)
    w = write_dynamic(dyn(), [0x61, 0x62, ("sym", 257), ("raw", 0, 9)], four, [0])
    out.append(("a match without a distance code", w.done(64), 64))
    w = write_dynamic(dyn(), [0x61, 0x62, ("sym", 257), ("raw", 1, 1)], four, [1])
    out.append(("the unused code of a single distance code", closed(w, b"abbbb"), 5))
    # Each of the next ones is whole but for its fault: the block reaches its end-of-block code and the
    # Adler-32 is that of the bytes a decoder without the check would write, so only the check named
    # stands between the stream and OMR_OK.  The code without a place in an over-subscribed set belongs
    # to a symbol the block does not use.
    two = assign([0x61, 256], [1, 1], 257)
    copy = assign([0x61, 256, 258], [1, 2, 2], 259)          # 258: a match of four bytes
    for name, tokens, ll, dl in (("incomplete literal/length code", [0x61] * 5, assign([0x61, 256], [2, 2], 257), [0]),
                                 ("incomplete distance code of two codes", [0x61, (4, 1)], copy, [2, 2]),
                                 ("over-subscribed literal/length code", [0x61] * 5,
                                  assign([0x61, 0x62, 256, 257], [1, 2, 2, 2], 258), [0]),
                                 ("over-subscribed distance code", [0x61, (4, 1)], copy, [1, 1, 1])):
        out.append((name, closed(write_dynamic(dyn(), tokens, ll, dl), b"aaaaa"), 5))
    for sym in (16, 17, 18):                                 # one length is left: each repeat is at least three
        w = write_dynamic(dyn(), [0x61] * 5, two, [1], items=pack_lengths(two) + [(sym, 0)], check=False)
        out.append((f"repeat {sym} past HLIT + HDIST", closed(w, b"aaaaa"), 5))
    # 70 literals and a match 71 back: the match is symbol 7 of the second batch (outpos 64, 6 bytes of
    # its own batch before it).  Its output is not defined, so the stream shows a wrong status only: a
    # decoder that compared with outpos alone would refuse it too.
    tokens = [0x30 + k % 10 for k in range(70)] + [(3, 71)]
    out.append(("distance one beyond the bytes produced", deflate_blocks([("fixed", tokens)], finish=False).done(64), 73))
    chain = assign(list(range(14)) + [256, 283], leaf_lengths(16, 15), 284)
    cut = [deflate_blocks([("dynamic", [0] * n + list(range(14)) + [("sym", 283), ("raw", 3, 2)],
                            dict(ll=chain, dl=[1, 1], eob=False))], finish=False) for n in range(8)]
    cut = [w for w in cut if w.n == 0]                       # the stream ends behind two of the five extra bits
    assert len(cut) == 1 and canonical(chain)[283][1] == 15
    out.append(("cut inside the extra bits of a 15-bit code", bytes(cut[0].out), 200))
    out.append(("Adler-32 cut to three bytes", good[:-1], 5000))
    for name, s, e in out:
        try:
            ok = len(zlib.decompress(s)) == e
        except zlib.error:
            ok = False
        assert not ok, name
    return out
