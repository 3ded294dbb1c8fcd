"""The JPEG-compressed TIFF fixture (tests/golden/tiff_jpeg.npz, written by
tools/make_tiff_jpeg_golden.py: files as byte arrays, and the pixels libtiff and libjpeg-turbo
agree on) for the host and the GPU tests of K17, with the byte-level helpers that make refused and
damaged variants.  Nothing here needs Pillow."""
import os
import struct

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiff_jpeg.npz")
_Z = np.load(GOLDEN)
NAMES = sorted(k[:-4] for k in _Z.files if k.endswith(".tif"))
FORMS = ("EOB_EARLY", "FULL_BLOCK", "ZRL", "LONG_CODE", "DC_CAT9", "STUFFED_FF", "RESTART", "PAD_BITS", "TABLE_OVERRIDE")
ACCEPT = ("jpeg", "samples")


def raw(name):
    return _Z[name + ".tif"].tobytes()


def pixels(name):
    """[c][h][w] uint8: the expected samples, one plane per channel."""
    px = _Z[name + ".px"]
    return px[None] if px.ndim == 2 else np.ascontiguousarray(np.moveaxis(px, -1, 0))


def spp(name):
    return pixels(name).shape[0]


def write(tmp, name, data=None):
    path = os.path.join(str(tmp), name + ".tif")
    with open(path, "wb") as f:
        f.write(raw(name) if data is None else data)
    return path


def ifd_of(data):
    """{tag: (position of the entry's value field, type, count, values or bytes)} of the first IFD (II, classic)."""
    assert data[:4] == b"II*\0"
    at = struct.unpack_from("<I", data, 4)[0]
    out = {}
    for k in range(struct.unpack_from("<H", data, at)[0]):
        tag, typ, cnt = struct.unpack_from("<HHI", data, at + 2 + 12 * k)
        size = {1: 1, 2: 1, 3: 2, 4: 4, 5: 8, 7: 1}[typ] * cnt
        field = at + 2 + 12 * k + 8
        pos = field if size <= 4 else struct.unpack_from("<I", data, field)[0]
        blob = bytes(data[pos:pos + size])
        out[tag] = (field, typ, cnt, blob if typ in (1, 2, 7) else list(struct.unpack("<%d%s" % (cnt, {3: "H", 4: "I"}[typ]), blob)))
    return out


def segments_of(data):
    """(tables or b"", [(x, y, w, h, offset, count)], W, H, spp, ycbcr)."""
    t = ifd_of(data)
    W, H = t[256][3][0], t[257][3][0]
    n = t[277][3][0] if 277 in t else 1
    if 322 in t:
        tw, th = t[322][3][0], t[323][3][0]
        boxes = [(x, y, tw, th) for y in range(0, H, th) for x in range(0, W, tw)]
        offs, cnts = t[324][3], t[325][3]
    else:
        rps = min(t[278][3][0], H)
        boxes = [(0, y, W, min(rps, H - y)) for y in range(0, H, rps)]
        offs, cnts = t[273][3], t[279][3]
    return (t[347][3] if 347 in t else b""), [b + (o, c) for b, o, c in zip(boxes, offs, cnts)], W, H, n, t[262][3][0] == 6


def streams_of(name):
    """(tables, [(x, y, w, h, stream)], spp, ycbcr) of a fixture file."""
    data = raw(name)
    tables, segs, W, H, n, ycc = segments_of(data)
    return tables, [(x, y, w, h, data[o:o + c]) for (x, y, w, h, o, c) in segs], n, ycc


def expected_segment(name, x, y, w, h):
    """The stored pixels of a segment's part inside the image: [rows][cols] or [rows][cols][3]."""
    px = pixels(name)[:, y:y + h, x:x + w]
    return px[0] if px.shape[0] == 1 else np.moveaxis(px, 0, -1)


def sos_at(stream):
    """Position of the first entropy-coded byte (behind the SOS header)."""
    pos = 2
    while True:
        assert stream[pos] == 0xFF
        m = stream[pos + 1]
        n = struct.unpack_from(">H", stream, pos + 2)[0]
        pos += 2 + n
        if m == 0xDA:
            return pos


def marker_at(stream, marker):
    """Position of marker segment `marker` in the header."""
    pos = 2
    while True:
        assert stream[pos] == 0xFF
        if stream[pos + 1] == marker:
            return pos
        assert stream[pos + 1] != 0xDA
        pos += 2 + struct.unpack_from(">H", stream, pos + 2)[0]


# ---- variants of a stream ------------------------------------------------------------------------

def as_progressive(stream):
    s = bytearray(stream)
    s[marker_at(s, 0xC0) + 1] = 0xC2
    return bytes(s)


def as_12bit(stream):
    s = bytearray(stream)
    s[marker_at(s, 0xC0) + 4] = 12
    return bytes(s)


def as_two_scans(stream):
    sos = marker_at(stream, 0xDA)
    assert stream[-2:] == b"\xff\xd9"
    return stream[:-2] + stream[sos:]


def with_undefined_code(stream):
    """Sixteen one-bits where the first DC code stands: no Huffman code is all ones."""
    s = bytearray(stream)
    at = sos_at(s)
    s[at:at + 4] = b"\xff\x00\xff\x00"
    return bytes(s)


def with_swapped_rst(stream):
    s = bytearray(stream)
    a, b = s.find(b"\xff\xd0", sos_at(s)), s.find(b"\xff\xd1", sos_at(s))
    if a < 0 or b < 0:
        # one restart marker only: RST0 becomes RST1, which is out of order just the same
        assert a >= 0
        s[a + 1] = 0xD1
        return bytes(s)
    s[a + 1], s[b + 1] = 0xD1, 0xD0
    return bytes(s)


def with_wrong_frame_size(stream):
    s = bytearray(stream)
    at = marker_at(s, 0xC0)
    h = struct.unpack_from(">H", s, at + 5)[0]
    struct.pack_into(">H", s, at + 5, h + 8)
    return bytes(s)


def patched_file(name, segment, variant):
    """The fixture file with `variant` applied to segment number `segment` (the length must not change)."""
    data = bytearray(raw(name))
    _, segs, _, _, _, _ = segments_of(data)
    o, c = segs[segment][4], segs[segment][5]
    new = variant(bytes(data[o:o + c]))
    assert len(new) == c
    data[o:o + c] = new
    return bytes(data)
