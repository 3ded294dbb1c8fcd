"""Zstandard frames for the K16 tests: the inputs of the golden fixture (tests/golden/zstd_frames.npz,
written by tools/make_zstd_golden.py with libzstd 1.4.8), the fixture's reader, frames crafted by
hand for the forms libzstd was not seen to write, malformed frames, edge frames for the device
decoder, and seeded damage.  Inputs come from the small integer generator below, not from numpy's
RNG, whose streams are not promised across versions; the fixture stores only frames and the
SHA-256 of each input."""
import functools
import hashlib
import os

import numpy as np

import omr
from omr import zarrimage as zi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "zstd_frames.npz")


def rnd(n, seed):
    """n pseudo-random uint32 from a counter hash in plain 64-bit integer arithmetic."""
    with np.errstate(over="ignore"):
        x = (np.arange(n, dtype=np.uint64) + np.uint64(seed) * np.uint64(0x9E3779B9)) * np.uint64(0x9E3779B97F4A7C15)
        x ^= x >> np.uint64(32)
        x *= np.uint64(0xD6E8FEB86659FD93)
        x ^= x >> np.uint64(32)
        x *= np.uint64(0xD6E8FEB86659FD93)
        x ^= x >> np.uint64(32)
    return (x >> np.uint64(16)).astype(np.uint32)


def rbytes(n, seed, mod=256):
    """n pseudo-random bytes below `mod`."""
    return (rnd(n, seed) % mod).astype(np.uint8).tobytes()


def smooth_u16(h, w, seed):
    """A smooth uint16 image with a few bits of noise (integer arithmetic only)."""
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    base = 9000 + ((x - w // 2) ** 2 * 3 + (y - h // 3) ** 2 * 5) // 16 + (x * y) // 64
    return ((base + (rnd(h * w, seed).reshape(h, w) & 31)) & 0xFFFF).astype("<u2")


def records(n, seed, lens=(5, 6, 9, 13, 17, 24, 33), rand=2):
    """n records of a few lengths, each `rand` random bytes and a fixed tail: matches at a handful of
    distances, the same mix all along (libzstd repeats its offset table over them)."""
    r, rb = rnd(n, seed).tolist(), rbytes(n * rand, seed + 1)
    tail = b"0123456789abcdefghijklmnopqrstuvwxyz"
    return b"".join(rb[k * rand:(k + 1) * rand] + tail[:lens[r[k] % len(lens)] - rand] for k in range(n))


def shuffled(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1, a.dtype.itemsize).T.tobytes()


def inputs():
    """name -> bytes: the inputs libzstd was given for the fixture (3 B to 420 KB)."""
    img = smooth_u16(420, 500, 1)
    r = rnd(200000, 2)
    two = np.where(r % 10 == 0, 7, 200).astype(np.uint8)
    five = np.array([3, 3, 3, 90, 91, 92, 250, 251], dtype=np.uint8)[rnd(100000, 3) % 8]
    lens = 3 + rnd(6000, 4) % 38
    runs = np.repeat((rnd(6000, 5) % 251).astype(np.uint8), lens)
    alt = np.empty((9000, 13), dtype=np.uint8)
    alt[:, :5] = (rnd(45000, 6) & 255).reshape(9000, 5)
    alt[:, 5:] = np.frombuffer(b"OMEZARR!", dtype=np.uint8)
    sp = rnd(300000, 7)
    sparse = np.where(sp % 50 == 0, (sp >> 8) & 255, 0).astype(np.uint8)
    return {
        "image_shuffled": shuffled(img),
        "image_high": shuffled(img)[img.size:],
        "image_small_shuffled": shuffled(img[:150, :160]),
        "two_symbols": two.tobytes(),
        "two_symbols_short": two[:20000].tobytes(),
        "five_symbols": five.tobytes(),
        "five_symbols_short": five[:12000].tobytes(),
        "five_uniform": rbytes(3000, 3, 5),
        "records": records(500, 32),
        "runs": runs.tobytes(),
        "runs_short": runs[:9000].tobytes(),
        "alternating": alt.tobytes(),
        "alternating_short": alt[:900].tobytes(),
        "sparse": sparse.tobytes(),
        "sparse_short": sparse[:40000].tobytes(),
        "image_5000": img.tobytes()[:5000],
        "image_300": img.tobytes()[:300],
        "constant": b"\x2a" * 70000,
        "three": b"omr",
    }


CHUNK_IMAGE_SHAPE = (96, 128)


def chunk_image():
    """The uint16 image whose Blosc-Zstd chunks (64 x 48, shuffled, split) are in the fixture as
    libzstd level-5 frames, one per stream."""
    return smooth_u16(CHUNK_IMAGE_SHAPE[0], CHUNK_IMAGE_SHAPE[1], 9)


def chunk_parts():
    """The streams blosc_encode asks a codec for when it writes chunk_image in 64 x 48 chunks."""
    parts = []

    def spy(part):
        parts.append(bytes(part))
        return omr.zstd_encode(part)

    a = chunk_image()
    for cy in range(2):
        for cx in range(2):
            omr.blosc_encode(a[cy * 48:(cy + 1) * 48, cx * 64:(cx + 1) * 64].tobytes(), 2, codec=spy)
    return parts


def sha(data):
    return hashlib.sha256(data).hexdigest()


@functools.lru_cache(maxsize=None)
def golden_frames():
    """[(name, data, frame)] of the fixture, every input checked against its stored SHA-256."""
    z = np.load(GOLDEN)
    data = inputs()
    out = []
    for key in sorted(k for k in z.files if k.startswith("frame/")):
        name = key[len("frame/"):]
        src = name.split("@")[0]
        assert sha(data[src]) == str(z["sha/" + src]), f"the generator no longer makes input {src}"
        out.append((name, data[src], z[key].tobytes()))
    return out


@functools.lru_cache(maxsize=None)
def golden_chunk_frames():
    """{SHA-256 of a stream's bytes: its libzstd level-5 frame} for chunk_parts()."""
    z = np.load(GOLDEN)
    return {k[len("chunk/"):]: z[k].tobytes() for k in z.files if k.startswith("chunk/")}


def golden_codec(part):
    """blosc_encode's codec= that looks a stream's frame up in the fixture."""
    return golden_chunk_frames()[sha(bytes(part))]


REQUIRED_FORMS = {
    "BLOCK_RAW", "BLOCK_RLE", "BLOCK_COMPRESSED", "LIT_RAW", "LIT_HUFFMAN", "LIT_TREELESS", "STREAMS_1", "STREAMS_4",
    "WEIGHTS_DIRECT", "WEIGHTS_FSE", "SEQ_ZERO", "SEQ_SHORT",
    "LL_PREDEFINED", "LL_RLE", "LL_FSE", "LL_REPEAT", "OF_PREDEFINED", "OF_RLE", "OF_FSE", "OF_REPEAT",
    "ML_PREDEFINED", "ML_RLE", "ML_FSE", "ML_REPEAT", "SINGLE_SEGMENT", "WINDOWED",
    "FCS_ABSENT", "FCS_1", "FCS_2", "FCS_4", "CHECKSUM", "MULTI_BLOCK"}
CRAFTED_FORMS = {"LIT_RLE", "SEQ_3BYTE", "FCS_8"}


def period4(n, seed=11):
    """Period-4 data with one changing byte: every four bytes a match of three and one literal."""
    a = np.empty((n // 4, 4), dtype=np.uint8)
    a[:, :3] = (17, 34, 51)
    a[:, 3] = rnd(n // 4, seed) & 255
    return a.tobytes()


def fcs8(frame, n):
    """A single-segment frame of zstd_encode with its content size rewritten as eight bytes."""
    assert frame[4] & 0x20 and not frame[4] & 3
    old = {0: 1, 1: 2, 2: 4, 3: 8}[frame[4] >> 6]
    return frame[:4] + bytes([frame[4] & 0x3F | 0xC0]) + n.to_bytes(8, "little") + frame[5 + old:]


HUF_WEIGHTS = (1, 1, 2)          # direct weights of symbols 0, 1, 2; symbol 3 gets the deduced weight 3
HUF_CODES = {0: (0b000, 3), 1: (0b001, 3), 2: (0b01, 2), 3: (0b1, 1)}    # symbol -> (code, bits), table log 3


def huffman_stream(lits, shift=0):
    """One backward Huffman bit stream of `lits` (symbols 0 .. 3) in the code above; shift: so many
    zero bits too many (positive) below the first symbol, which a decoder must refuse."""
    acc = nb = 0
    for sym in reversed(lits):
        code, n = HUF_CODES[sym]
        acc |= code << nb
        nb += n
    acc = acc << shift | 1 << (nb + shift)
    return acc.to_bytes((nb + shift + 8) // 8, "little")


def huffman_literals(lits, streams=1, treeless=False, weights=HUF_WEIGHTS, shift=0, sf=None):
    """A literals section with Huffman (or treeless) literals: direct weights, one or four streams."""
    n = len(lits)
    tree = b"" if treeless else bytes([127 + len(weights)]) + bytes(
        (weights[k] << 4 | (weights[k + 1] if k + 1 < len(weights) else 0)) for k in range(0, len(weights), 2))
    if streams == 1:
        body = huffman_stream(lits, shift)
    else:
        q = (n + 3) // 4
        parts = [huffman_stream(lits[k * q:(k + 1) * q], shift if k == 3 else 0) for k in range(4)]
        body = b"".join(len(x).to_bytes(2, "little") for x in parts[:3]) + b"".join(parts)
    c = len(tree) + len(body)
    if sf is None:
        sf = (0 if streams == 1 else 1) if max(n, c) < 1024 else 2 if max(n, c) < 16384 else 3
    bits = 10 if sf < 2 else 14 if sf == 2 else 18
    v = (3 if treeless else 2) | sf << 2 | n << 4 | c << (4 + bits)
    return v.to_bytes(3 if sf < 2 else 4 if sf == 2 else 5, "little") + tree + body


def symbols(n, seed):
    """n literals 0 .. 3, skewed as the code above expects."""
    return np.array([3, 3, 3, 3, 2, 2, 1, 0], dtype=np.uint8)[rnd(n, seed) % 8].tobytes()


@functools.lru_cache(maxsize=None)
def crafted_frames():
    """[(name, data, frame)]: the forms not seen from libzstd."""
    out = []
    # a compressed block with RLE literals and no sequences, then one with RLE literals and sequences
    data = b"\x55" * 20
    body = bytes([1 | 20 << 3, 0x55, 0])
    out.append(("rle_literals", data, zi.zstd_frame_header(20) + zi.zstd_block(2, body, True)))
    # RLE literals of 300 with two sequences: 100 literals + a match of 50 at distance 1, twice; 100 literals behind
    body = bytes((300 << 4 | 1 << 2 | 1).to_bytes(2, "little")) + b"\x66"
    seq = zi.zstd_sequences_block(b"", [(100, 1 + 3, 50), (100, 1, 50)])   # the second repeats the offset
    data = b"\x66" * 400
    out.append(("rle_literals_sequences", data, zi.zstd_frame_header(400) + zi.zstd_block(2, body + seq[1:], True)))
    p = period4(128 << 10)
    f = omr.zstd_encode(p)
    out.append(("count_3byte", p, f))
    small = rbytes(3000, 12, 7)
    out.append(("content_size_8", small, fcs8(omr.zstd_encode(small), len(small))))
    return out


def all_good():
    return list(golden_frames()) + list(crafted_frames())


def _raw_frame(data, **kw):
    return zi.zstd_frame_header(len(data), **kw) + zi.zstd_block(0, data, True)


@functools.lru_cache(maxsize=None)
def bad_frames():
    """[(name, frame, expected)]: every one is OMR_INTERNAL."""
    d = rbytes(600, 13, 5)
    good = omr.zstd_encode(d)
    hdr = zi.zstd_frame_header
    blk = zi.zstd_block
    out = [("empty", b"", 0), ("bad_magic", b"\x29" + good[1:], 600),
           ("skippable_frame", b"\x50\x2a\x4d\x18\x04\0\0\0abcd", 4),
           ("second_frame", good + good, 600), ("trailing_byte", good + b"\0", 600),
           ("reserved_bit", good[:4] + bytes([good[4] | 8]) + good[5:], 600),
           ("dictionary_id", good[:4] + bytes([good[4] | 1]) + b"\x07" + good[5:], 600),
           ("content_size_differs", good, 601), ("content_size_differs_short", good, 599),
           ("block_type_3", hdr(4) + (4 << 3 | 3 << 1 | 1).to_bytes(3, "little") + b"abcd", 4),
           ("oversize_block", hdr(8, single_segment=False)[:5] + bytes([0]) + hdr(8, single_segment=False)[6:] +
            blk(0, b"x" * 1025, True), 1025),
           ("oversize_block_single_segment", hdr(8) + blk(0, b"x" * 9, True), 8),
           ("raw_block_truncated", hdr(8) + blk(0, b"x" * 8, True)[:-1], 8),
           ("no_last_block", hdr(8) + blk(0, b"x" * 8, False), 8),
           ("output_short", hdr(8, content_size=False, single_segment=False) + blk(0, b"x" * 7, True), 8),
           ("output_long", hdr(8, content_size=False, single_segment=False) + blk(0, b"x" * 9, True), 8),
           ("rle_block_long", hdr(8, content_size=False, single_segment=False) + blk(1, b"x", True, 9), 8),
           ("window_too_large", b"\x28\xb5\x2f\xfd\x00" + bytes([22 << 3]) + blk(0, b"x" * 8, True), 8)]

    def compressed(body, n=64, last=True):
        return hdr(n) + blk(2, body, last)

    seqs = zi.zstd_sequences_block
    lit20 = bytes(range(20))
    lit4 = symbols(40, 14)
    assert omr.zstd_decode_host(compressed(huffman_literals(lit4) + b"\0", 40), 40) == lit4
    assert omr.zstd_decode_host(compressed(huffman_literals(lit4, streams=4) + b"\0", 40), 40) == lit4
    ok_body = seqs(lit20, [(20, 20 + 3, 44)])
    assert omr.zstd_decode_host(compressed(ok_body), 64) == (lit20 * 4)[:64]
    out += [
        ("treeless_first_block", compressed(huffman_literals(lit4, treeless=True) + b"\0", 40), 40),
        ("huffman_stream_not_consumed", compressed(huffman_literals(lit4, shift=8) + b"\0", 40), 40),
        ("huffman_stream_one_bit_over", compressed(huffman_literals(lit4, shift=1) + b"\0", 40), 40),
        ("huffman_stream_too_short", compressed(huffman_literals(lit4 + b"\3", shift=0)[:3] + huffman_literals(lit4)[3:] + b"\0", 41), 41),
        ("huffman_fourth_stream_not_consumed", compressed(huffman_literals(lit4, streams=4, shift=8) + b"\0", 40), 40),
        ("huffman_zero_final_byte", compressed(huffman_literals(lit4)[:-1] + b"\0\0", 40), 40),
        ("weights_not_power_of_two", compressed(huffman_literals(lit4, weights=(1, 1, 1, 1, 1)) + b"\0", 40), 40),
        ("weight_over_11", compressed(huffman_literals(lit4, weights=(12, 1)) + b"\0", 40), 40),
        ("weights_all_zero", compressed(huffman_literals(lit4, weights=(0, 0)) + b"\0", 40), 40),
        ("repeat_table_first_block", compressed(bytes([20 << 3]) + lit20 + bytes([1, 0xC0]) + ok_body[23:]), 64),
        ("reserved_mode_bits", compressed(ok_body[:22] + bytes([1]) + ok_body[23:]), 64),
        # an FSE table description whose accuracy log is 10 (literal lengths allow 9)
        ("accuracy_log_over", compressed(bytes([20 << 3]) + lit20 + bytes([1, 0x80, 0x05]) + ok_body[23:]), 64),
        ("offset_log_over", compressed(bytes([20 << 3]) + lit20 + bytes([1, 0x20, 0x04]) + ok_body[23:]), 64),
        ("rle_offset_code_32", compressed(bytes([20 << 3]) + lit20 + bytes([1, 0x10, 32]) + ok_body[23:]), 64),
        ("zero_final_byte", compressed(ok_body[:-1] + b"\0"), 64),
        ("stream_not_consumed", compressed(ok_body[:23] + b"\0" + ok_body[23:]), 64),
        ("stream_too_short", compressed(ok_body[:23] + ok_body[24:]), 64),
        ("offset_beyond_output", compressed(seqs(lit20, [(20, 21 + 3, 44)])), 64),
        ("offset_beyond_output_first", compressed(seqs(lit20, [(0, 1 + 3, 44)]), 64), 64),
        ("repeat_offset_zero", compressed(seqs(lit20, [(0, 3, 44)])), 64),        # ll 0, value 3: rep[0] - 1 = 0
        ("literals_overrun", compressed(seqs(lit20, [(21, 20 + 3, 43)])), 64),
        ("output_past_expected", compressed(seqs(lit20, [(20, 20 + 3, 45)])), 64),
        ("output_short_of_expected", compressed(seqs(lit20, [(20, 20 + 3, 43)])), 64),
        ("sequences_after_count_zero", compressed(bytes([20 << 3]) + lit20 + bytes([0, 0]), 20), 20),
        ("literals_past_block", compressed(bytes([30 << 3]) + lit20, 30), 30),
    ]
    ck = omr.zstd_encode(d, checksum=True)
    out.append(("wrong_checksum", ck[:-1] + bytes([ck[-1] ^ 1]), 600))
    out.append(("checksum_missing", ck[:-4], 600))
    return out


@functools.lru_cache(maxsize=None)
def edge_frames():
    """[(name, data, frame)] for the device decoder's paths, from the project's encoder and the crafter."""
    seqs, hdr, blk = zi.zstd_sequences_block, zi.zstd_frame_header, zi.zstd_block
    out = []
    for n in (0, 1, 131072, 131073):
        d = rbytes(n, 20 + n % 7, 3)
        out.append((f"size_{n}", d, omr.zstd_encode(d)))
        out.append((f"size_{n}_windowed_checksum", d, omr.zstd_encode(d, checksum=True, content_size=False, single_segment=False)))

    def one_block(name, lits, ss, n=None):
        body = seqs(lits, ss)
        frame_n = sum(a + c for a, _, c in ss) + len(lits) - sum(a for a, _, _ in ss) if n is None else n
        frame = hdr(frame_n) + blk(2, body, True)
        out.append((name, omr.zstd_decode_host(frame, frame_n), frame))

    base = rbytes(700, 21)
    # rounds of exactly 64 and 65 sequences, and the sequence count forms 127 / 128 and 0x7EFF / 0x7F00
    for ns in (64, 65, 127, 128):
        one_block(f"sequences_{ns}", base[:ns * 2 + 5], [(2, 2 + 3 + (k % 3), 3 + k % 9) for k in range(ns)])
    for ns in (0x7EFF, 0x7F00):
        lits = rbytes(ns + 9, 22)
        one_block(f"sequences_{ns:#x}", lits, [(1, 4 + 3, 3) if k else (9, 4 + 3, 3) for k in range(ns)])
    # matches at distance 1, 2 and 3 longer than the distance; a match of 65,539 bytes and more
    for dist in (1, 2, 3):
        one_block(f"distance_{dist}", base[:10], [(7, dist + 3, 200 + dist), (1, dist + 3, 5)])
    one_block("match_65539", base[:40], [(30, 29 + 3, 65539), (2, 7 + 3, 65000)])
    one_block("literals_70000", rbytes(70000, 23), [(69990, 69000 + 3, 40)])
    # repeat offsets with zero literal length: value 1 -> rep[1], 2 -> rep[2], 3 -> rep[0] - 1, and the rotation
    one_block("repeat_offsets", base[:64], [(10, 5 + 3, 4), (0, 1, 6), (0, 2, 5), (0, 3, 7), (3, 1, 4), (2, 2, 4), (1, 3, 9),
                                             (0, 9 + 3, 3), (0, 3, 5)])
    # a match that reaches into the block before (a raw block, then a compressed one), and one into an RLE block
    first = base[:100]
    body = seqs(base[100:110], [(4, 100 + 3, 60), (2, 150 + 3, 30)])
    frame = hdr(100 + 50 + 100) + blk(0, first, False) + blk(1, b"\x09", False, 50) + blk(2, body, True)
    out.append(("match_into_earlier_blocks", omr.zstd_decode_host(frame, 250), frame))
    # literal totals around the one-to-four-stream boundary and not divisible by four: libzstd is not needed for
    # these, the golden frames hold Huffman literals; here raw literal totals with every header size
    for n in (31, 32, 4095, 4096):
        one_block(f"raw_literals_{n}", rbytes(n, 24), [(n - 1, 5 + 3, 9)])
    # Huffman literals in the crafter's code: one stream up to its largest total, four streams from their
    # smallest, totals that are no multiple of four (the fourth stream shorter, or empty), every size format,
    # and a treeless block behind a block with a tree
    for n, streams in ((1, 1), (1022, 1), (1023, 1), (6, 4), (7, 4), (9, 4), (1021, 4), (1023, 4), (1024, 4), (1026, 4),
                       (16383, 4), (16385, 4), (70001, 4)):
        lits = symbols(n, 25 + n % 5)
        out.append((f"huffman_{n}_in_{streams}", lits, hdr(n, single_segment=False) + blk(2, huffman_literals(lits, streams) + b"\0", True)))
    lits = symbols(3000, 26)
    body = huffman_literals(lits[:2000], 4) + seqs(b"", [(1500, 700 + 3, 333)])[1:]
    frame = hdr(3333) + blk(2, body, False) + blk(2, huffman_literals(lits[2000:], 1, treeless=True) + b"\0", True)
    out.append(("huffman_sequences_then_treeless", omr.zstd_decode_host(frame, 3333), frame))
    return out


def damaged(frame, count, seed):
    """`count` copies of `frame`, each with one to three bytes changed (seeded)."""
    r = rnd(count * 7, seed).tolist()
    out = []
    for k in range(count):
        b = bytearray(frame)
        for j in range(1 + r[7 * k] % 3):
            at = r[7 * k + 1 + 2 * j] % len(b)
            b[at] ^= 1 + r[7 * k + 2 + 2 * j] % 255
        out.append(bytes(b))
    return out


def truncations(frame):
    """Every length up to 64 and 16 evenly spaced ones beyond."""
    n = len(frame)
    cuts = list(range(min(n, 65)))
    if n > 65:
        cuts += [65 + (n - 66) * k // 15 for k in range(16)]
    return sorted(set(c for c in cuts if c < n))


def dump(directory):
    """Everything the stand-alone sanitizer program (tools/zstd_read_check.cpp) reads, as files:
    index.txt lists `kind file expected` (kind good, bad, blosc), and two groups g_blosc and g_zstd
    of one uint16 image sit beside it with its pixels in pixels.bin."""
    os.makedirs(directory, exist_ok=True)
    lines = []

    def put(kind, k, data, expected):
        name = f"{kind}_{k:03d}.bin"
        with open(os.path.join(directory, name), "wb") as f:
            f.write(data)
        lines.append(f"{kind} {name} {expected}")

    k = 0
    for name, data, frame in all_good() + list(edge_frames()):
        if len(frame) <= 50000:
            put("good", k, frame, len(data))
            k += 1
    for k, (name, frame, expected) in enumerate(bad_frames()):
        put("bad", k, frame, expected)
    d = inputs()
    for k, (data, ts, kw) in enumerate([(d["image_small_shuffled"][:20000], 2, {}), (d["runs_short"], 1, {}),
                                        (d["image_5000"], 2, {"split": False}), (d["alternating_short"], 4, {"blocksize": 4096})]):
        put("blosc", k, omr.blosc_encode(data, ts, codec="zstd", **kw), len(data))
    a = chunk_image()[None, None, None]
    omr.write_zarr(os.path.join(directory, "g_blosc"), a, chunk=(64, 48), compressor="blosc", blosc={"cname": "zstd"},
                   dimension_separator=".")
    omr.write_zarr(os.path.join(directory, "g_zstd"), a, chunk=(64, 48), compressor="zstd", dimension_separator=".")
    with open(os.path.join(directory, "pixels.bin"), "wb") as f:
        f.write(a.tobytes())
    with open(os.path.join(directory, "index.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
