"""The streams of the split JPEG entropy decode's tests (K18): every segment of
tests/golden/tiff_jpeg.npz and the bare streams of tests/golden/jpeg_split.npz (written by
tools/make_jpeg_split_golden.py: long restart intervals, with the pixels libjpeg-turbo decodes),
and helpers that run the serial and the split host decoder side by side.  Nothing here needs Pillow."""
import os

import numpy as np

import omr
import tiff_jpeg_cases as jc
from omr import _lib

_Z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_split.npz"))
SPLIT_NAMES = sorted(k[:-4] for k in _Z.files if k.endswith(".jpg"))


class Stream:
    def __init__(self, ident, data, w, h, n, ycc, tables):
        self.id, self.data, self.w, self.h, self.n, self.ycc, self.tables = ident, data, w, h, n, ycc, tables

    def args(self):
        return (self.w, self.h, self.n, self.ycc, self.tables)


def split_pixels(name):
    key = name + ".px" if name + ".px" in _Z.files else _Z[name + ".same"].tobytes().decode() + ".px"
    return _Z[key]


def split_stream(name):
    px = split_pixels(name)
    n = 1 if px.ndim == 2 else 3
    return Stream(name, _Z[name + ".jpg"].tobytes(), px.shape[1], px.shape[0], n, n == 3, None)


def tiff_streams(name):
    tables, segs, n, ycc = jc.streams_of(name)
    return [Stream("%s.%d" % (name, k), s, w, h, n, ycc, tables or None) for k, (x, y, w, h, s) in enumerate(segs)]


SPLIT = [split_stream(name) for name in SPLIT_NAMES]
TIFF = [s for name in jc.NAMES for s in tiff_streams(name)]
ALL = SPLIT + TIFF


def serial(s, data=None):
    """(status, bytes or None) of omr_jpeg_decode_host."""
    try:
        return _lib.OK, omr.jpeg_decode_host(s.data if data is None else data, *s.args()).tobytes()
    except omr.OmrError as e:
        return e.status, None


def split(s, bits, lanes, data=None):
    """(status, bytes or None, stats or None) of omr_jpeg_decode_host_split."""
    try:
        px, stats = omr.jpeg_decode_host_split(s.data if data is None else data, *s.args(), subsequence_bits=bits, lanes=lanes)
        return _lib.OK, px.tobytes(), stats
    except omr.OmrError as e:
        return e.status, None, None


def entropy_span(data):
    """[first, end) of the entropy-coded bytes of a stream without restart markers whose scan ends at the final EOI."""
    first = jc.sos_at(data)
    end = len(data) - 2
    assert data[end:] == b"\xff\xd9"
    while data[end - 1] == 0xFF:                             # fill bytes before EOI
        end -= 1
    return first, end
