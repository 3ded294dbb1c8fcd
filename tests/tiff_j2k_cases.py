"""The JPEG 2000 fixture (tests/golden/tiff_j2k.npz, written by tools/make_tiff_j2k_golden.py: raw
reversible codestreams and TIFF files that hold such streams, as byte arrays, with the pixels
OpenJPEG decodes them to) for the host and the GPU tests of K19, with the byte-level helpers that
make refused and damaged variants.  Nothing here needs Pillow."""
import os
import struct

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiff_j2k.npz")
_Z = np.load(GOLDEN)
STREAMS = sorted(k[2:-4] for k in _Z.files if k.startswith("s.") and k.endswith(".j2k"))
FILES = sorted(k[:-4] for k in _Z.files if k.endswith(".tif"))
TRUNCATED = [n for n in STREAMS if n.endswith("_truncated")]
ACCEPT = ("jpeg2000", "samples")


def _pixels(name):
    return _Z[name + ".px"] if name + ".px" in _Z.files else _Z[str(_Z[name + ".same"])]


def stream(name):
    return _Z["s." + name + ".j2k"].tobytes()


def stream_pixels(name):
    """[h][w] or [h][w][3], uint8 or uint16: OpenJPEG's decode of the stream."""
    return _pixels("s." + name)


def shape_of(name):
    """(width, height, samples, bits) of a stream."""
    px = stream_pixels(name)
    return px.shape[1], px.shape[0], 1 if px.ndim == 2 else 3, 8 * px.dtype.itemsize


def raw(name):
    return _Z[name + ".tif"].tobytes()


def pixels(name):
    """[c][h][w] uint8 or uint16 (host byte order): the file's samples, one plane per channel."""
    return _pixels(name)


def write(tmp, name, data=None):
    path = os.path.join(str(tmp), name + ".tif")
    with open(path, "wb") as f:
        f.write(raw(name) if data is None else data)
    return path


def segments_of(data):
    """[(x, y, w, h, offset, count)] of the first IFD of a classic TIFF in either byte order."""
    bo = "<" if data[:2] == b"II" else ">"
    at = struct.unpack_from(bo + "I", data, 4)[0]
    t = {}
    for k in range(struct.unpack_from(bo + "H", data, at)[0]):
        tag, typ, cnt = struct.unpack_from(bo + "HHI", data, at + 2 + 12 * k)
        size = {1: 1, 2: 1, 3: 2, 4: 4, 7: 1}[typ] * cnt
        pos = at + 2 + 12 * k + 8
        if size > 4:
            pos = struct.unpack_from(bo + "I", data, pos)[0]
        t[tag] = list(struct.unpack(bo + "%d%s" % (cnt, {1: "B", 3: "H", 4: "I", 7: "B"}[typ]), bytes(data[pos:pos + size])))
    W, H = t[256][0], t[257][0]
    if 322 in t:
        tw, th = t[322][0], t[323][0]
        boxes = [(x, y, tw, th) for y in range(0, H, th) for x in range(0, W, tw)]
        offs, cnts = t[324], t[325]
    else:
        rps = min(t[278][0], H)
        boxes = [(0, y, W, min(rps, H - y)) for y in range(0, H, rps)]
        offs, cnts = t[273], t[279]
    return [b + (o, c) for b, o, c in zip(boxes, offs, cnts)]


def patched_file(name, segment, variant):
    """The fixture file with `variant` applied to segment number `segment` (the length must not change)."""
    data = bytearray(raw(name))
    o, c = segments_of(data)[segment][4:6]
    new = variant(bytes(data[o:o + c]))
    assert len(new) == c
    data[o:o + c] = new
    return bytes(data)


# ---- a codestream's marker segments ----------------------------------------------------------------

SIZ, COD, QCD, COM, SOT, SOD = 0x51, 0x52, 0x5C, 0x64, 0x90, 0x93


def marker_at(s, marker):
    """Position of marker segment `marker` in the main or tile-part header (of SOD itself for SOD)."""
    pos = 2
    while True:
        assert s[pos] == 0xFF
        if s[pos + 1] == marker:
            return pos
        assert s[pos + 1] != SOD
        pos += 2 + struct.unpack_from(">H", s, pos + 2)[0]


def edited(s, marker, offset, value, mask=0xFF):
    """The stream with byte `offset` of the marker segment's body (behind its length word) replaced
    in the bits of `mask`."""
    out = bytearray(s)
    at = marker_at(out, marker) + 4 + offset
    out[at] = (out[at] & ~mask & 0xFF) | (value & mask)
    return bytes(out)


def renamed(s, marker, new):
    out = bytearray(s)
    out[marker_at(out, marker) + 1] = new
    return bytes(out)


# COD's body: Scod, progression, layers (2), MCT, levels, xcb, ycb, code-block style, transform, precincts
# QCD's body: Sqcd (style | guard << 5), then one byte per subband (exponent << 3)
# SIZ's body: Rsiz (2), Xsiz, Ysiz, XOsiz, YOsiz, XTsiz, YTsiz, XTOsiz, YTOsiz (4 each), Csiz (2), then Ssiz, XRsiz, YRsiz per component
# SOT's body: Isot (2), Psot (4), TPsot, TNsot

# name of the refusal -> (variant of a stream, words the reason must hold)
REFUSED = {
    "9/7": (lambda s: edited(s, COD, 9, 0), "9/7"),
    "quantisation style 1": (lambda s: edited(s, QCD, 0, 1, 31), "derived"),
    "quantisation style 2": (lambda s: edited(s, QCD, 0, 2, 31), "expounded"),
    "bypass": (lambda s: edited(s, COD, 8, 1), "bypass"),
    "reset": (lambda s: edited(s, COD, 8, 2), "reset"),
    "terminate-all": (lambda s: edited(s, COD, 8, 4), "termination on each"),
    "vertically causal": (lambda s: edited(s, COD, 8, 8), "vertically causal"),
    "predictable termination": (lambda s: edited(s, COD, 8, 16), "predictable termination"),
    "segmentation symbols": (lambda s: edited(s, COD, 8, 32), "segmentation symbols"),
    "SOP": (lambda s: edited(s, COD, 0, 2, 2), "SOP"),
    "EPH": (lambda s: edited(s, COD, 0, 4, 4), "EPH"),
    "COC": (lambda s: renamed(s, COM, 0x53), "COC"),
    "QCC": (lambda s: renamed(s, COM, 0x5D), "QCC"),
    "RGN": (lambda s: renamed(s, COM, 0x5E), "RGN"),
    "POC": (lambda s: renamed(s, COM, 0x5F), "POC"),
    "PPM": (lambda s: renamed(s, COM, 0x60), "PPM"),
    "PPT": (lambda s: renamed(s, COM, 0x61), "PPT"),
    "several tiles": (lambda s: edited(s, SIZ, 21, 16), "several tiles"),                  # XTsiz = 16 on a wider image
    "several tile-parts": (lambda s: edited(s, SOT, 6, 1), "tile-parts"),
    "image offset": (lambda s: edited(s, SIZ, 13, 1), "offsets"),
    "tile offset": (lambda s: edited(s, SIZ, 33, 1), "offsets"),
    "subsampled": (lambda s: edited(s, SIZ, 37, 2), "subsampled"),
    "signed": (lambda s: edited(s, SIZ, 36, 0x80, 0x80), "signed"),
    "12-bit": (lambda s: edited(s, SIZ, 36, 11), "precision"),
    "JP2 wrapper": (lambda s: b"\x00\x00\x00\x0cjP  \r\n\x87\n" + s, "JP2"),
}


def with_small_exponents(s):
    """Every subband's exponent 1: with two guard bits no block may have more than two bit-planes."""
    out = bytearray(s)
    at = marker_at(out, QCD)
    n = struct.unpack_from(">H", out, at + 2)[0] - 3
    for k in range(n):
        out[at + 5 + k] = 1 << 3
    return bytes(out)


def cut_with_eoc(s, keep):
    """The first `keep` bytes behind SOD, Psot = 0 (the tile-part runs up to EOC) and EOC: the packets run out of bytes."""
    out = bytearray(s)
    struct.pack_into(">I", out, marker_at(out, SOT) + 6, 0)
    return bytes(out[:marker_at(out, SOD) + 2 + keep]) + b"\xff\xd9"


# name -> variant of a stream that must give OMR_INTERNAL
DAMAGED = {
    "cut inside SIZ": lambda s: s[:20],
    "cut inside COD": lambda s: s[:marker_at(s, COD) + 6],
    "cut behind SOD": lambda s: s[:marker_at(s, SOD) + 2],
    "cut inside the packets": lambda s: s[:marker_at(s, SOD) + 2 + (len(s) - marker_at(s, SOD)) // 2],
    "packets past the tile-part": lambda s: cut_with_eoc(s, (len(s) - marker_at(s, SOD)) // 2),
    "packet header cut": lambda s: cut_with_eoc(s, 0),
    "more passes or zero bit-planes than M_b": with_small_exponents,
    "no EOC": lambda s: s[:-2],
}


def with_empty_packet(s):
    """The first packet's header byte 0: an empty packet (for a stream whose packet says `nothing included`)."""
    out = bytearray(s)
    at = marker_at(out, SOD) + 2
    assert out[at] == 0x80 and bytes(out[at + 1:]) == b"\xff\xd9"
    out[at] = 0
    return bytes(out)


def with_body_damage(s, seed):
    """Forty bytes of the second half of the packets replaced: no header can be told from a body
    here, so the result is any status but a crash; tests use it on streams of one packet."""
    rng = np.random.default_rng(seed)
    out = bytearray(s)
    lo = marker_at(out, SOD) + 2 + (len(out) - marker_at(out, SOD)) // 2
    for at in rng.integers(lo, len(out) - 2, 40):
        out[at] = int(rng.integers(0, 256))
    return bytes(out)
