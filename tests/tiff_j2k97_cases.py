"""The irreversible JPEG 2000 fixture (tests/golden/tiff_j2k97.npz, written by
tools/make_tiff_j2k97_golden.py: raw 9/7 codestreams and TIFF files that hold such streams, as byte
arrays, with the pixels OpenJPEG decodes them to and, per entry, the number of samples where the
host decoder differed from OpenJPEG when the fixture was made) for the host and the GPU tests of
K20.  The byte-level helpers that make refused and damaged variants are tiff_j2k_cases'.  Nothing
here needs Pillow."""
import os

import numpy as np

from tiff_j2k_cases import (COD, COM, DAMAGED, QCD, REFUSED, SIZ, SOD, SOT, edited, marker_at, renamed,  # noqa: F401
                            segments_of, with_body_damage)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiff_j2k97.npz")
_Z = np.load(GOLDEN)
STREAMS = sorted(k[2:-4] for k in _Z.files if k.startswith("s.") and k.endswith(".j2k"))
FILES = sorted(k[:-4] for k in _Z.files if k.endswith(".tif"))
MIXED = "mixed_tiles_33005"
ACCEPT = ("jpeg2000", "jpeg2000-lossy", "samples")
OPENJPEG = str(_Z["openjpeg"])
# K19's refusals that K20 lifts behind its flag (the transform and the quantisation style then have to match)
NOW_ALLOWED = ("9/7", "quantisation style 1", "quantisation style 2")


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


def differing(name):
    """The number of samples of a stream or file where the host decoder differed from OpenJPEG when the fixture was made."""
    return int(_Z["diff." + name])


def raw(name):
    return _Z[name + ".tif"].tobytes()


def pixels(name):
    """[c][h][w] uint8 or uint16 (host byte order): OpenJPEG's decode of the file's segments, one plane per channel."""
    return _pixels(name)


def write(tmp, name, data=None):
    path = os.path.join(str(tmp), name + ".tif")
    with open(path, "wb") as f:
        f.write(raw(name) if data is None else data)
    return path


def patched_file(name, segment, variant):
    """The fixture file with `variant` applied to segment number `segment` (the length must not change)."""
    data = bytearray(raw(name))
    o, c = segments_of(data)[segment][4:6]
    new = variant(bytes(data[o:o + c]))
    assert len(new) == c
    data[o:o + c] = new
    return bytes(data)


def segment_bytes(name, segment):
    data = raw(name)
    o, c = segments_of(data)[segment][4:6]
    return data[o:o + c]


def assert_agrees_with_openjpeg(got, want, name):
    """Equality where the fixture's tool counted no differing sample; elsewhere a difference of 1 at
    the most (two float32 evaluations of one formula part on a rounding tie only) on no more
    samples than the tool counted: the host decoder is deterministic, so there is no margin."""
    assert got.dtype == want.dtype and got.shape == want.shape, name
    if differing(name) == 0:
        assert got.tobytes() == want.tobytes(), name
        return
    d = np.abs(got.astype(np.int64) - want.astype(np.int64))
    assert d.max() <= 1 and int((d > 0).sum()) <= differing(name), (name, int(d.max()), int((d > 0).sum()))
