#!/usr/bin/env python3
"""Writes tests/golden/jpeg_split.npz: a handful of bare baseline JPEG streams with long restart
intervals, for the split entropy decode (K18), each with the pixels libjpeg-turbo decodes.

Run on a machine with Pillow (libjpeg-turbo inside); the tests that read the fixture do not need
it.  Entries (NAME.jpg the stream, NAME.px its pixels, [h][w] or [h][w][3]; an entry without
pixels of its own names the entry that has them in NAME.same):

  noise420      256 x 256, 4:2:0, quality 85, noise over ramps, no restart markers
  noise444_q100 64 x 64, 4:4:4, quality 100: long codes and full blocks
  flat420       128 x 128, 4:2:0, one grey value: the stream is periodic, guessed states settle slowly
  noise422      96 x 48, 4:2:2
  grey          80 x 56, one component
  noise420_rst  noise420 with a restart interval of 64 MCUs: several long intervals, each restarting the predictor

The tool asserts that the library's host decoder gives Pillow's pixels on each.

    python3 tools/make_jpeg_split_golden.py
"""
import io
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "jpeg_split.npz")


def noise(w, h, seed, amplitude=48):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    a = np.stack([x * 255 // (w - 1), y * 255 // (h - 1), (x + y) * 255 // (w + h - 2)], -1).astype(np.int32)
    a += rng.integers(-amplitude, amplitude + 1, size=a.shape)
    return np.clip(a, 0, 255).astype(np.uint8)


def encode(arr, **kw):
    from PIL import Image
    f = io.BytesIO()
    Image.fromarray(arr).save(f, format="JPEG", **kw)
    return f.getvalue()


def main():
    from PIL import Image
    sys.path.insert(0, os.path.join(REPO, "omero-ms-image-region_amd"))
    import omr
    big = noise(256, 256, 11)
    entries = [("noise420", big, dict(quality=85, subsampling="4:2:0"), None),
               ("noise444_q100", noise(64, 64, 12, 128), dict(quality=100, subsampling="4:4:4"), None),
               ("flat420", np.full((128, 128, 3), 128, np.uint8), dict(quality=85, subsampling="4:2:0"), None),
               ("noise422", noise(96, 48, 13), dict(quality=90, subsampling="4:2:2"), None),
               ("grey", np.ascontiguousarray(noise(80, 56, 14)[:, :, 1]), dict(quality=85), None),
               ("noise420_rst", big, dict(quality=85, subsampling="4:2:0", restart_marker_blocks=64), "noise420")]
    arrays = {}
    for name, arr, kw, same in entries:
        stream = encode(arr, **kw)
        px = np.asarray(Image.open(io.BytesIO(stream)))
        n = 1 if px.ndim == 2 else 3
        ours = omr.jpeg_decode_host(stream, px.shape[1], px.shape[0], n, n == 3)
        assert np.array_equal(ours, px), name + ": the host decoder differs from libjpeg-turbo"
        assert (b"\xff\xd0" in stream) == ("restart_marker_blocks" in kw), name
        arrays[name + ".jpg"] = np.frombuffer(stream, dtype=np.uint8)
        if same:
            assert np.array_equal(px, arrays[same + ".px"]), name + ": restart markers changed the pixels"
            arrays[name + ".same"] = np.frombuffer(same.encode(), dtype=np.uint8)
        else:
            arrays[name + ".px"] = px
        print("%-14s %6d bytes  %s" % (name, len(stream), sorted(omr.jpeg_stream_forms(stream))))
    np.savez_compressed(GOLDEN, **arrays)
    print("wrote %s: %d bytes" % (GOLDEN, os.path.getsize(GOLDEN)))


def unpack(dst):
    """The fixture's streams into dst for tools/jpeg_split_check.cpp, in the form
    tools/make_tiff_jpeg_golden.py --unpack gives the TIFF fixture's: NAME.0.jpg beside an empty
    NAME.tables, with split_streams.txt (`name 0 width height spp ycbcr 0` per stream).  Needs no Pillow."""
    os.makedirs(dst, exist_ok=True)
    z = np.load(GOLDEN)
    with open(os.path.join(dst, "split_streams.txt"), "w") as idx:
        for key in sorted(z.files):
            if not key.endswith(".jpg"):
                continue
            name = key[:-4]
            px = z[name + ".px"] if name + ".px" in z.files else z[z[name + ".same"].tobytes().decode() + ".px"]
            open(os.path.join(dst, name + ".0.jpg"), "wb").write(z[key].tobytes())
            open(os.path.join(dst, name + ".tables"), "wb").close()
            idx.write("%s 0 %d %d %d %d 0\n" % (name, px.shape[1], px.shape[0], 1 if px.ndim == 2 else 3, int(px.ndim == 3)))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--unpack":
        unpack(sys.argv[2])
    else:
        main()
