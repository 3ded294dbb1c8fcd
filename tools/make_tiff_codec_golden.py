#!/usr/bin/env python3
"""Writes tests/golden/tiff_codecs.npz: whole small TIFF files of a real encoder for the TIFF codec
tests (tests/test_tiff_codecs_host.py, tests/test_tiff_codecs_gpu.py).

libtiff through Pillow (the fixture in the repository was written with Pillow 12.2, libtiff 4.7.1)
writes the 150 x 70 images of tests/tiff_codec_cases.py (GOLDEN_FILES, golden_pixels) as strips of
32 rows, so the last strip has 6: Deflate and zstd with Predictor 1 and 2 on uint8 and uint16,
float32 Deflate with Predictor 3, and chunky uint8 RGB Deflate with Predictor 1 and 2.  This Pillow
writes little-endian strips only, and neither 64-bit samples nor 16-bit RGB: those forms are covered
by the project's own writer.  The fixture stores every file ("file/<name>") and its pixels
("pixels/<name>", [samples][70][150]); each file is read back here with Pillow and with the
library's host route before it is kept.

    python tools/make_tiff_codec_golden.py      # needs the built library and Pillow with libtiff
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "omero-ms-image-region_amd"), os.path.join(REPO, "tests")]

import omr  # noqa: E402
import tiff_codec_cases as tc  # noqa: E402
from PIL import Image, TiffImagePlugin, features  # noqa: E402


def main():
    import tempfile
    print("Pillow", Image.__version__, "libtiff", features.version("libtiff"))
    arrays = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, (dtype, spp, comp, pred, _) in tc.GOLDEN_FILES.items():
            px = tc.golden_pixels(name)
            im = Image.fromarray(px[0] if spp == 1 else np.ascontiguousarray(np.moveaxis(px, 0, -1)))
            ifd = TiffImagePlugin.ImageFileDirectory_v2()
            ifd[278] = 32
            if pred != 1:
                ifd[317] = pred
            path = os.path.join(tmp, name + ".tif")
            im.save(path, compression=comp, tiffinfo=ifd)
            with Image.open(path) as back:
                got = np.array(back)
                assert back.tag_v2[278] == 32 and back.tag_v2.get(317, 1) == pred, name
                assert back.tag_v2[259] == (50000 if comp == "zstd" else 8), name
            assert np.array_equal(got if spp == 1 else np.moveaxis(got, -1, 0), px[0] if spp == 1 else px), name
            with omr.TiffImage(path, 1, spp, 1, accept=tc.golden_need(name)) as img:
                assert not img.info["tiled"] and img.info["segment_height"] == 32 and not img.big_endian
                for c in range(spp):
                    assert img.get_tile(0, 0, c, 0, 0, 0, tc.W, tc.H).tobytes() == px[c].tobytes(), (name, c)
            with open(path, "rb") as f:
                data = f.read()
            arrays["file/" + name] = np.frombuffer(data, dtype=np.uint8)
            arrays["pixels/" + name] = px
            print(f"  {name}: {len(data)} bytes")
    np.savez_compressed(tc.GOLDEN, **arrays)
    print(tc.GOLDEN, os.path.getsize(tc.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
