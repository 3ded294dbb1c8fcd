"""ZarrImage: OME-Zarr pixel data (K14), and write_zarr, the small writer that makes the test and
probe groups.

The third backend of pixelsService.getPixelBuffer beside the ROMIO file (pixbuf.PixelBuffer) and
the tiled TIFF (tiffimage.TiffImage): a Zarr v2 directory as bioformats2raw writes it, one 5-D
TCZYX array per resolution and one file per chunk.  Reads go through libomr.so: get_tile on the
host (plain serial inflate), read_regions and render_tiles with the zlib chunks inflated on the GPU
(omr_inflate.hip).  Blosc chunks with LZ4 inside (K15, bioformats2raw's default) are read when the
image is opened with codecs=("zlib", "blosc"): their streams are decoded on the GPU by
omr_blosc.hip.  Blosc chunks with Zstd inside and the bare zstd codec (K16) open with "blosc-zstd" and
"zstd" in codecs: their Zstandard frames are decoded on the GPU by omr_zstd.hip.  lz4_encode,
zstd_encode and blosc_encode are small pure-Python encoders for the tests and the probes, so that
neither needs an outside library.
"""
import ctypes
import json
import os
import zlib

import numpy as np

from . import _lib
from ._lib import lib
from ._segimage import _SegImage
from .tiffimage import _NP_NAMES


def lz4_encode(data):
    """One LZ4 block of `data`: a small greedy encoder (a table of the last position of every four
    bytes, longer steps over what does not compress).  As the format asks of an encoder, the last
    five bytes are literals and no match starts within the last twelve."""
    data = bytes(data)
    n = len(data)
    out = bytearray()

    def sequence(lits, offset=0, mlen=0):
        ll = len(lits)
        ml = mlen - 4 if mlen else 0
        out.append(min(ll, 15) << 4 | min(ml, 15))
        if ll >= 15:
            out.extend(b"\xff" * ((ll - 15) // 255))
            out.append((ll - 15) % 255)
        out.extend(lits)
        if mlen:
            out.extend(offset.to_bytes(2, "little"))
            if ml >= 15:
                out.extend(b"\xff" * ((ml - 15) // 255))
                out.append((ml - 15) % 255)

    anchor = i = 0
    table = {}
    misses = 0
    while i + 12 <= n:
        key = data[i:i + 4]
        cand = table.get(key)
        table[key] = i
        if cand is None or i - cand > 65535:
            misses += 1
            i += 1 + (misses >> 5)
            continue
        misses = 0
        m, top = 4, n - 5 - i                      # the match ends before the last five bytes
        while m + 64 <= top and data[cand + m:cand + m + 64] == data[i + m:i + m + 64]:
            m += 64
        while m < top and data[cand + m] == data[i + m]:
            m += 1
        sequence(data[anchor:i], i - cand, m)
        i += m
        anchor = i
    sequence(data[anchor:])
    return bytes(out)


# ---- Zstandard (K16): a small encoder of RFC 8878 frames ---------------------------------------

_LL_DEFAULT = [4, 3] + [2] * 11 + [1] * 3 + [2] * 9 + [3, 2] + [1] * 5 + [-1] * 4
_OF_DEFAULT = [1] * 6 + [2] * 3 + [1] * 15 + [-1] * 5
_ML_DEFAULT = [1, 4, 3] + [2] * 6 + [1] * 37 + [-1] * 7
_LL_BASE = list(range(16)) + [16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384,
                              32768, 65536]
_LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
_ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195,
                                 16387, 32771, 65539]
_ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ZSTD_BLOCK_MAX = 128 << 10


def _fse_decode_table(freq, log):
    """The FSE decoding table of a normalized distribution (RFC 8878 4.1.1): [(symbol, bits, base)]."""
    size = 1 << log
    sym, nxt, high = [0] * size, {}, size
    for s, f in enumerate(freq):
        if f == -1:
            high -= 1
            sym[high] = s
            nxt[s] = 1
    step, pos = (size >> 1) + (size >> 3) + 3, 0
    for s, f in enumerate(freq):
        if f <= 0:
            continue
        nxt[s] = f
        for _ in range(f):
            sym[pos] = s
            pos = (pos + step) & (size - 1)
            while pos >= high:
                pos = (pos + step) & (size - 1)
    assert pos == 0
    table = []
    for i in range(size):
        x = nxt[sym[i]]
        nxt[sym[i]] += 1
        nb = log - (x.bit_length() - 1)
        table.append((sym[i], nb, (x << nb) - size))
    return table


def _fse_encoder(freq, log):
    """Per symbol the states that decode it, as (base, bits, state): an encoder that must leave
    the decoder in state t picks the one whose [base, base + 2^bits) holds t."""
    enc = {}
    for i, (s, nb, base) in enumerate(_fse_decode_table(freq, log)):
        enc.setdefault(s, []).append((base, nb, i))
    return {s: sorted(v) for s, v in enc.items()}


_ZSTD_ENC = None


def _code_of(bases, v):
    import bisect
    return bisect.bisect_right(bases, v) - 1


def xxh64(data, seed=0):
    """XXH64 of `data` (the content checksum of a Zstandard frame is its low 32 bits)."""
    M = (1 << 64) - 1
    P1, P2, P3, P4, P5 = (0x9E3779B185EBCA87, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x85EBCA77C2B2AE63,
                          0x27D4EB2F165667C5)

    def rotl(v, r):
        return (v << r | v >> (64 - r)) & M

    def rnd(acc, inp):
        return rotl((acc + inp * P2) & M, 31) * P1 & M

    n, i = len(data), 0
    if n >= 32:
        v = [(seed + P1 + P2) & M, (seed + P2) & M, seed, (seed - P1) & M]
        words = np.frombuffer(data[:n // 32 * 32], dtype="<u8").tolist()
        for k, w in enumerate(words):
            v[k & 3] = rnd(v[k & 3], w)
        i = n // 32 * 32
        h = (rotl(v[0], 1) + rotl(v[1], 7) + rotl(v[2], 12) + rotl(v[3], 18)) & M
        for k in range(4):
            h = ((h ^ rnd(0, v[k])) * P1 + P4) & M
    else:
        h = (seed + P5) & M
    h = (h + n) & M
    while i + 8 <= n:
        h = (rotl(h ^ rnd(0, int.from_bytes(data[i:i + 8], "little")), 27) * P1 + P4) & M
        i += 8
    if i + 4 <= n:
        h = (rotl(h ^ (int.from_bytes(data[i:i + 4], "little") * P1 & M), 23) * P2 + P3) & M
        i += 4
    while i < n:
        h = rotl(h ^ (data[i] * P5 & M), 11) * P1 & M
        i += 1
    h ^= h >> 33
    h = h * P2 & M
    h ^= h >> 29
    h = h * P3 & M
    return h ^ h >> 32


def zstd_sequences_block(literals, seqs):
    """The body of a compressed block: `literals` raw, seqs = [(literal length, offset value, match
    length)] coded with the predefined tables into the backward bit stream.  The offset value is
    the coded one: 1, 2, 3 name repeat offsets, v > 3 is the distance v - 3."""
    global _ZSTD_ENC
    if _ZSTD_ENC is None:
        _ZSTD_ENC = (_fse_encoder(_LL_DEFAULT, 6), _fse_encoder(_OF_DEFAULT, 5), _fse_encoder(_ML_DEFAULT, 6))
    ell, eof, eml = _ZSTD_ENC
    n = len(literals)
    if n < 32:
        out = bytearray([n << 3])
    elif n < 4096:
        out = bytearray((n << 4 | 1 << 2).to_bytes(2, "little"))
    else:
        out = bytearray((n << 4 | 3 << 2).to_bytes(3, "little"))
    out += literals
    ns = len(seqs)
    if ns < 128:
        out.append(ns)
    elif ns < 0x7F00:
        out += bytes([(ns >> 8) + 128, ns & 255])
    else:
        out += bytes([255]) + (ns - 0x7F00).to_bytes(2, "little")
    if ns == 0:
        return bytes(out)
    out.append(0)                                          # all three tables predefined
    acc = nacc = 0
    bits = bytearray()

    def put(v, nb):
        nonlocal acc, nacc
        acc |= v << nacc
        nacc += nb
        if nacc >= 64:
            bits.extend((acc & ((1 << 64) - 1)).to_bytes(8, "little"))
            acc >>= 64
            nacc -= 64

    def leave(enc, code, target):
        """(bits to write, state): the state decoding `code` from which the decoder goes to target."""
        for base, nb, state in enc[code]:
            if base <= target < base + (1 << nb):
                return target - base, nb, state
        raise AssertionError("no FSE state")

    sl = so = sm = None
    for k in range(ns - 1, -1, -1):                        # the decoder reads what is written last first
        ll, ov, ml = seqs[k]
        lc, oc, mc = _code_of(_LL_BASE, ll), ov.bit_length() - 1, _code_of(_ML_BASE, ml)
        assert ov >= 1 and ml >= 3 and oc <= 28
        if sl is None:
            sl, so, sm = ell[lc][0][2], eof[oc][0][2], eml[mc][0][2]
        else:
            vo, no, so = leave(eof, oc, so)
            vm, nm, sm = leave(eml, mc, sm)
            vl, nl, sl = leave(ell, lc, sl)
            put(vo, no)
            put(vm, nm)
            put(vl, nl)
        put(ll - _LL_BASE[lc], _LL_BITS[lc])
        put(ml - _ML_BASE[mc], _ML_BITS[mc])
        put(ov - (1 << oc), oc)
    put(sm, 6)
    put(so, 5)
    put(sl, 6)
    put(1, 1)
    bits.extend(acc.to_bytes((nacc + 7) // 8, "little"))
    return bytes(out) + bytes(bits)


def zstd_frame_header(n, checksum=False, content_size=True, single_segment=True):
    """Magic and frame header for a frame of n bytes."""
    if single_segment:
        assert content_size, "a single-segment frame states its size"
        flag, field = (0, n.to_bytes(1, "little")) if n < 256 else (1, (n - 256).to_bytes(2, "little")) if n < 65792 \
            else (2, n.to_bytes(4, "little")) if n < 1 << 32 else (3, n.to_bytes(8, "little"))
        return b"\x28\xb5\x2f\xfd" + bytes([flag << 6 | 0x20 | (4 if checksum else 0)]) + field
    wlog = max(10, (max(n, 1) - 1).bit_length())
    flag, field = (0, b"") if not content_size else (1, (n - 256).to_bytes(2, "little")) if 256 <= n < 65792 \
        else (2, n.to_bytes(4, "little")) if n < 1 << 32 else (3, n.to_bytes(8, "little"))
    return b"\x28\xb5\x2f\xfd" + bytes([flag << 6 | (4 if checksum else 0), (wlog - 10) << 3]) + field


def zstd_block(kind, body, last, size=None):
    """A block header and body: kind 0 raw, 1 RLE (body one byte, `size` its run), 2 compressed."""
    size = len(body) if size is None else size
    return (size << 3 | kind << 1 | (1 if last else 0)).to_bytes(3, "little") + body


def zstd_encode(data, checksum=False, content_size=True, single_segment=True):
    """`data` as one Zstandard frame: a small greedy encoder (a table of the last position of every
    three bytes, minimum match 3, repeat offsets where they fall out).  Blocks of up to 128 KiB:
    RLE when a block is one byte repeated, compressed (raw literals, sequences coded with the
    predefined tables) when that is smaller, else raw.  Matches reach back over the whole frame;
    a frame with a window descriptor states a window that holds all of it."""
    data = bytes(data)
    n = len(data)
    out = bytearray(zstd_frame_header(n, checksum, content_size, single_segment))
    reps = [1, 4, 8]
    table = {}
    start = 0
    while True:
        end = min(n, start + ZSTD_BLOCK_MAX)
        last = end == n
        block = data[start:end]
        if len(block) > 1 and block == block[:1] * len(block):
            out += zstd_block(1, block[:1], last, len(block))
            for i in range(start, max(start, end - 2)):    # later blocks may still match into this one
                table[data[i:i + 3]] = i
        else:
            lits, seqs, trial = bytearray(), [], list(reps)
            anchor = i = start
            misses = 0
            while i + 3 <= end:
                key = data[i:i + 3]
                cand = table.get(key)
                table[key] = i
                if cand is None:
                    misses += 1
                    i += 1 + (misses >> 6)
                    continue
                misses = 0
                m, top = 3, end - i
                while m + 64 <= top and data[cand + m:cand + m + 64] == data[i + m:i + m + 64]:
                    m += 64
                while m < top and data[cand + m] == data[i + m]:
                    m += 1
                ll, off = i - anchor, i - cand
                r = trial
                if ll:
                    ov = 1 if off == r[0] else 2 if off == r[1] else 3 if off == r[2] else off + 3
                else:
                    ov = 1 if off == r[1] else 2 if off == r[2] else 3 if off == r[0] - 1 else off + 3
                idx = ov - 1 + (0 if ll else 1) if ov <= 3 else 3
                if idx == 1:
                    trial = [off, r[0], r[2]]
                elif idx >= 2:
                    trial = [off, r[0], r[1]]
                lits += data[anchor:i]
                seqs.append((ll, ov, m))
                i += m
                anchor = i
            lits += data[anchor:end]
            body = zstd_sequences_block(bytes(lits), seqs) if seqs else None
            if body is not None and len(body) < len(block):
                out += zstd_block(2, body, last)
                reps = trial
            else:
                out += zstd_block(0, block, last)
        if last:
            break
        start = end
    if checksum:
        out += (xxh64(data) & 0xFFFFFFFF).to_bytes(4, "little")
    return bytes(out)


def _shuffle(block, typesize):
    q = len(block) // typesize
    a = np.frombuffer(block, dtype=np.uint8)
    return a[:q * typesize].reshape(q, typesize).T.tobytes() + block[q * typesize:]


def blosc_encode(data, typesize, shuffle=1, blocksize=0, split=None, memcpy=False, codec="lz4"):
    """`data` as one Blosc 1 chunk (the container as recalled, see omr.h) with LZ4 inside, or with
    codec "zstd" one Zstandard frame of zstd_encode per stream (compressor format 4), or with a
    callable bytes -> frame the frames it returns (format 4 as well): shuffle 0
    or 1 (byte shuffle per block, flag 0x01); blocksize 0: one block of up to 256 KiB, a multiple of
    typesize; split None or True: a block is typesize streams where the format's rule allows it,
    False: flag 0x10 (do not split); a stream that does not compress is stored raw; memcpy: flag
    0x02, the bytes follow the header as they are."""
    data = bytes(data)
    n = len(data)
    assert 1 <= typesize <= 255 and shuffle in (0, 1) and n > 0
    if blocksize <= 0:
        blocksize = min(n, 256 << 10)
        if blocksize > typesize:
            blocksize -= blocksize % typesize
    encode = lz4_encode if codec == "lz4" else zstd_encode if codec == "zstd" else codec
    assert callable(encode), f"unknown Blosc codec {codec!r}"
    flags = (1 if codec == "lz4" else 4) << 5 | (1 if shuffle else 0) | (0x10 if split is False else 0) | (2 if memcpy else 0)

    def header(cbytes):
        return bytes([2, 1, flags, typesize]) + b"".join(int(v).to_bytes(4, "little") for v in (n, blocksize, cbytes))

    if memcpy:
        return header(n + 16) + data
    nblocks = (n + blocksize - 1) // blocksize
    body, bstarts, at = bytearray(), [], 16 + 4 * nblocks
    for b in range(nblocks):
        block = data[b * blocksize:(b + 1) * blocksize]
        leftover = len(block) < blocksize
        if shuffle and typesize > 1:
            block = _shuffle(block, typesize)
        nsplits = typesize if (split is not False and typesize <= 16 and blocksize // typesize >= 128
                               and not leftover) else 1
        if nsplits > 1:
            assert blocksize % typesize == 0, "a split block holds whole elements"
        ne = len(block) // nsplits
        bstarts.append(at + len(body))
        for k in range(nsplits):
            part = block[k * ne:(k + 1) * ne]
            stream = encode(part)
            if len(stream) >= ne:
                stream = part                            # stored raw: csize == neblock
            body += len(stream).to_bytes(4, "little") + stream
    return header(at + len(body)) + b"".join(v.to_bytes(4, "little") for v in bstarts) + bytes(body)


def write_zarr(path, planes, levels=(), chunk=(256, 256), byteorder="<", compressor="zlib", level=1, strategy=None,
               dimension_separator="/", skip_zero_chunks=False, zarray_overrides=None, blosc=None):
    """Write a [t][c][z][y][x] array as the image group `path` of an OME-Zarr (Zarr v2, NGFF 0.4
    multiscales metadata): array "0" holds `planes`, arrays "1", "2", ... hold `levels` (arrays of
    the same [t][c][z] with their own [y][x]).  chunk = (w, h): chunks [1, 1, 1, h, w], edge chunks
    stored whole; byteorder "<" or ">"; compressor "zlib" (stdlib zlib at `level`, `strategy` one
    of zlib.Z_* or None for the default) or None; dimension_separator "/" (as bioformats2raw) or
    "."; skip_zero_chunks: an all-zero chunk is not written; zarray_overrides = {key: value}
    replaces entries of every .zarray (to make groups a reader must reject).  compressor "blosc":
    chunks written by blosc_encode with the arguments in `blosc` = {"shuffle", "blocksize", "split",
    "memcpy", "typesize" (default: the sample size)}, and its "cname" (default "lz4") and "clevel"
    (default 5) written to the .zarray beside them; cname "zstd" makes the chunks' streams
    Zstandard frames (blosc_encode's codec, which "codec" in `blosc` overrides, for instance with a
    callable).  compressor "zstd": every chunk one frame of zstd_encode under {"id": "zstd"}."""
    planes = np.asarray(planes)
    assert planes.ndim == 5, "planes must be [t][c][z][y][x]"
    arrays = [planes] + [np.asarray(lv) for lv in levels]
    for lv in arrays[1:]:
        assert lv.ndim == 5 and lv.shape[:3] == planes.shape[:3] and lv.dtype == planes.dtype
    assert compressor in ("zlib", "blosc", "zstd", None) and dimension_separator in ("/", ".")
    bl = dict(blosc or {})
    cmeta = {"id": "zlib", "level": level} if compressor == "zlib" else None
    if compressor == "zstd":
        cmeta = {"id": "zstd", "level": level, "checksum": False}
    if compressor == "blosc":
        cmeta = {"id": "blosc", "cname": bl.pop("cname", "lz4"), "clevel": bl.pop("clevel", 5),
                 "shuffle": bl.get("shuffle", 1), "blocksize": bl.get("blocksize", 0)}
        bl.setdefault("typesize", planes.dtype.itemsize)
        bl.setdefault("codec", "zstd" if cmeta["cname"] == "zstd" else "lz4")
    dt = planes.dtype
    fdt = dt.newbyteorder(byteorder) if dt.itemsize > 1 else dt
    dtype_name = ("|" if dt.itemsize == 1 else byteorder) + dt.kind + str(dt.itemsize)
    cw, ch = chunk
    path = str(path)
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, ".zgroup"), "w") as f:
        json.dump({"zarr_format": 2}, f)
    axes = [{"name": "t", "type": "time"}, {"name": "c", "type": "channel"}, {"name": "z", "type": "space"},
            {"name": "y", "type": "space"}, {"name": "x", "type": "space"}]
    datasets = [{"path": str(k), "coordinateTransformations": [{"type": "scale", "scale": [1.0, 1.0, 1.0, float(2 ** k), float(2 ** k)]}]}
                for k in range(len(arrays))]
    with open(os.path.join(path, ".zattrs"), "w") as f:
        json.dump({"multiscales": [{"version": "0.4", "axes": axes, "datasets": datasets}]}, f, indent=1)
    for k, a in enumerate(arrays):
        adir = os.path.join(path, str(k))
        os.makedirs(adir, exist_ok=True)
        meta = {"zarr_format": 2, "shape": list(a.shape), "chunks": [1, 1, 1, ch, cw], "dtype": dtype_name,
                "compressor": cmeta, "fill_value": 0, "order": "C",
                "filters": None, "dimension_separator": dimension_separator}
        meta.update(zarray_overrides or {})
        with open(os.path.join(adir, ".zarray"), "w") as f:
            json.dump(meta, f, indent=1)
        st, sc, sz, h, w = a.shape
        for t in range(st):
            for c in range(sc):
                for z in range(sz):
                    for cy in range((h + ch - 1) // ch):
                        for cx in range((w + cw - 1) // cw):
                            part = a[t, c, z, cy * ch:(cy + 1) * ch, cx * cw:(cx + 1) * cw]
                            if skip_zero_chunks and not part.any():
                                continue
                            full = np.zeros((ch, cw), dtype=fdt)
                            full[:part.shape[0], :part.shape[1]] = part
                            raw = full.tobytes()
                            if compressor == "blosc":
                                raw = blosc_encode(raw, **bl)
                            elif compressor == "zstd":
                                raw = zstd_encode(raw)
                            elif compressor:
                                co = zlib.compressobj(level, zlib.DEFLATED, 15, 8,
                                                      zlib.Z_DEFAULT_STRATEGY if strategy is None else strategy)
                                raw = co.compress(raw) + co.flush()
                            name = dimension_separator.join(str(v) for v in (t, c, z, cy, cx))
                            file = os.path.join(adir, name)
                            os.makedirs(os.path.dirname(file), exist_ok=True)
                            with open(file, "wb") as f:
                                f.write(raw)


class ZarrImage(_SegImage):
    """An open OME-Zarr image group (omr_zarr_image): `path` is the image (series) group, for
    instance image.zarr/0.  Z, C and T come from the array shape; OME-XML is not read."""

    CODECS = {"zlib": _lib.ZARR_CODEC_ZLIB, "blosc": _lib.ZARR_CODEC_BLOSC,
              "blosc-zstd": _lib.ZARR_CODEC_BLOSC_ZSTD, "zstd": _lib.ZARR_CODEC_ZSTD}
    _CLOSE, _GET_TILE = "omr_zarr_image_close", "omr_zarr_image_get_tile"
    _READ_REGIONS, _RENDER_TILES = "omr_zarr_image_read_regions_device", "omr_render_zarr_tiles"

    def __init__(self, path, codecs=("zlib",)):
        """codecs: the chunk compressors accepted, ("zlib",) as omr_zarr_image_open or any of
        "zlib", "blosc" (LZ4 inside), "blosc-zstd" and "zstd" (omr_zarr_image_open_ex);
        uncompressed groups always open."""
        h = ctypes.c_void_p()
        if tuple(codecs) == ("zlib",):
            st = lib.omr_zarr_image_open(str(path).encode(), ctypes.byref(h))
        else:
            mask = 0
            for name in codecs:
                if name not in self.CODECS:
                    raise _lib.OmrError(_lib.INVALID_ARGUMENT, f"unknown Zarr codec {name!r}")
                mask |= self.CODECS[name]
            opt = _lib.ZarrOpenOptions(ctypes.sizeof(_lib.ZarrOpenOptions), mask)
            st = lib.omr_zarr_image_open_ex(str(path).encode(), ctypes.byref(opt), ctypes.byref(h))
        if st != _lib.OK:
            raise _lib.OmrError(st, f"cannot open Zarr image {path}")
        self.h = h
        i = _lib.ZarrInfo()
        _lib.check(lib.omr_zarr_image_info(self.h, ctypes.byref(i)))
        self.info = {n: int(getattr(i, n)) for n, _ in _lib.ZarrInfo._fields_}
        self.size_x, self.size_y = i.size_x, i.size_y
        self.size_z, self.size_c, self.size_t = i.size_z, i.size_c, i.size_t
        self.pixel_type = i.pixel_type
        self.big_endian = bool(i.big_endian)
        self.dtype = np.dtype((">" if self.big_endian else "<") + _NP_NAMES[self.pixel_type])
        sizes = (ctypes.c_int32 * (2 * i.n_levels))()
        n = lib.omr_zarr_image_level_sizes(self.h, sizes, i.n_levels)
        self.level_sizes = [[sizes[2 * k], sizes[2 * k + 1]] for k in range(n)]


def inflate_host(stream, expected):
    """The host inflate alone (omr_inflate_host): a zlib stream into exactly `expected` bytes, or
    OmrError(INTERNAL)."""
    return _decode_host(lib.omr_inflate_host, stream, expected)


def _decode_host(fn, stream, expected):
    src = np.frombuffer(bytes(stream), dtype=np.uint8)
    out = np.zeros(max(int(expected), 1), dtype=np.uint8)
    _lib.check(fn(src.ctypes.data if src.size else None, src.size, out.ctypes.data, int(expected)))
    return out[:int(expected)].tobytes()


def lz4_decode_host(stream, expected):
    """The host LZ4 decoder alone (omr_lz4_decode_host): one LZ4 block into exactly `expected`
    bytes, or OmrError(INTERNAL)."""
    return _decode_host(lib.omr_lz4_decode_host, stream, expected)


def blosc_decode_host(chunk, expected, inner=("lz4",)):
    """One Blosc 1 chunk into exactly `expected` bytes, or OmrError(INTERNAL); inner: the codecs
    its streams may be in, "lz4" and/or "zstd" (omr_blosc_decode_host_ex)."""
    names = {"lz4": _lib.BLOSC_INNER_LZ4, "zstd": _lib.BLOSC_INNER_ZSTD}
    mask = 0
    for name in inner:
        if name not in names:
            raise _lib.OmrError(_lib.INVALID_ARGUMENT, f"unknown Blosc inner codec {name!r}")
        mask |= names[name]
    return _decode_host(lambda *a: lib.omr_blosc_decode_host_ex(*a, mask), chunk, expected)


def zstd_decode_host(frame, expected):
    """The host Zstandard decoder alone (omr_zstd_decode_host): one frame into exactly `expected`
    bytes, or OmrError(INTERNAL)."""
    return _decode_host(lib.omr_zstd_decode_host, frame, expected)


def zstd_frame_forms(frame):
    """The forms a good frame uses (omr_zstd_frame_forms), as a set of names of _lib.ZSTD_FORM_NAMES."""
    src = np.frombuffer(bytes(frame), dtype=np.uint8)
    words = (ctypes.c_uint32 * _lib.ZSTD_FORM_WORDS)()
    _lib.check(lib.omr_zstd_frame_forms(src.ctypes.data if src.size else None, src.size, words))
    bits = sum(int(w) << (32 * k) for k, w in enumerate(words))
    return {n for k, n in enumerate(_lib.ZSTD_FORM_NAMES) if bits >> k & 1}
