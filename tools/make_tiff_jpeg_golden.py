#!/usr/bin/env python3
"""Writes tests/golden/tiff_jpeg.npz: small JPEG-compressed TIFF files (Compression 7) as byte
arrays, and the pixels two independent decoders agree on.

Run on a machine with Pillow (libtiff and libjpeg-turbo inside); the tests that read the fixture
need neither.  For every entry the tool asserts that libtiff's decode of the whole file
(Image.open) equals the libjpeg-turbo decode of each segment's spliced stream (SOI + the tables
of tag 347 + the segment's own markers and data), and stores those pixels; where Pillow cannot
read a form as a whole file it stores the per-segment decode and says so.  It then asserts that
omr_jpeg_stream_forms finds every coding form of FORMS somewhere in the fixture, and that the
library's host decoder gives the stored pixels.

    python3 tools/make_tiff_jpeg_golden.py                 # writes the fixture
    python3 tools/make_tiff_jpeg_golden.py --unpack DIR    # the fixture's files into DIR (for jpeg-read-check)
"""
import io
import os
import struct
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "tiff_jpeg.npz")
FORMS = ("EOB_EARLY", "FULL_BLOCK", "ZRL", "LONG_CODE", "DC_CAT9", "STUFFED_FF", "RESTART", "PAD_BITS", "TABLE_OVERRIDE",
         "MULTI_TABLE", "COM", "FILL_BYTES", "TABLES_STREAM")


def picture(w, h, seed):
    """[h][w][3] uint8: smooth ramps, noise of +-20, and flat saturated patches of pure red, blue,
    white and black (they make the colour clamp and the IDCT clamp act)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    a = np.stack([x * 255 // max(w - 1, 1), y * 255 // max(h - 1, 1), (x + y) * 255 // max(w + h - 2, 1)], -1).astype(np.int32)
    noisy = slice(w // 3, 2 * w // 3)
    a[:, noisy] += rng.integers(-20, 21, size=a[:, noisy].shape)
    a[h // 4:h // 2, noisy] = rng.integers(0, 256, size=a[h // 4:h // 2, noisy].shape)   # busy: long codes, full blocks
    a = np.clip(a, 0, 255)
    ph, pw = max(h // 5, 9), max(w // 8, 9)
    for k, colour in enumerate(((255, 0, 0), (0, 0, 255), (255, 255, 255), (0, 0, 0))):
        x0 = 3 + k * (pw + 2)
        a[h - ph - 2:h - 2, x0:x0 + pw] = colour
        a[1:1 + ph // 2, w - x0 - pw:w - x0] = colour
    return a.astype(np.uint8)


def ifd_of(raw):
    """{tag: (type, count, values or bytes)} of the first IFD of a little-endian classic TIFF."""
    assert raw[:4] == b"II*\0"
    at = struct.unpack_from("<I", raw, 4)[0]
    out = {}
    for k in range(struct.unpack_from("<H", raw, at)[0]):
        tag, typ, cnt = struct.unpack_from("<HHI", raw, at + 2 + 12 * k)
        size = {1: 1, 2: 1, 3: 2, 4: 4, 5: 8, 7: 1}[typ] * cnt
        pos = at + 2 + 12 * k + 8
        if size > 4:
            pos = struct.unpack_from("<I", raw, pos)[0]
        data = raw[pos:pos + size]
        out[tag] = bytes(data) if typ in (1, 2, 7) else list(struct.unpack("<%d%s" % (cnt, {3: "H", 4: "I", 5: "II"}[typ]), data))
    return out


def segments_of(raw):
    """(tables or b"", [(x, y, w, h, stream)], image w, h, spp, photometric) of a JPEG TIFF."""
    t = ifd_of(raw)
    W, H = t[256][0], t[257][0]
    spp = t.get(277, [1])[0]
    if 322 in t:
        tw, th = t[322][0], t[323][0]
        boxes = [(x, y, tw, th) for y in range(0, H, th) for x in range(0, W, tw)]
        offs, cnts = t[324], t[325]
    else:
        rps = min(t.get(278, [H])[0], H)
        boxes = [(0, y, W, min(rps, H - y)) for y in range(0, H, rps)]
        offs, cnts = t[273], t[279]
    segs = [(x, y, w, h, bytes(raw[o:o + c])) for (x, y, w, h), o, c in zip(boxes, offs, cnts)]
    return t.get(347, b""), segs, W, H, spp, t[262][0]


def spliced(tables, stream):
    """A segment as a whole stream: the tables of tag 347 in front of its own markers."""
    assert stream[:2] == b"\xff\xd8"
    return stream if not tables else b"\xff\xd8" + tables[2:-2] + stream[2:]


def by_segments(raw):
    """The image as libjpeg-turbo decodes its segments one by one: [h][w] or [h][w][3]."""
    from PIL import Image
    tables, segs, W, H, spp, _ = segments_of(raw)
    out = np.zeros((H, W) if spp == 1 else (H, W, spp), dtype=np.uint8)
    for (x, y, w, h, stream) in segs:
        im = Image.open(io.BytesIO(spliced(tables, stream)))
        im.draft(None, None)
        px = np.asarray(im.convert("L" if spp == 1 else "RGB") if im.mode not in ("L", "RGB") else im)
        assert px.shape[:2] == (h, w), (px.shape, w, h)
        part = px[:H - y, :W - x]
        out[y:y + part.shape[0], x:x + part.shape[1]] = part
    return out


def rewrite_markers(stream):
    """The same entropy-coded data behind rewritten marker segments: every DHT merged into one
    (several tables per segment), a COM segment, and fill FF bytes before SOS and before EOI."""
    sys.path.insert(0, os.path.join(REPO, "omero-ms-image-region_amd"))
    from omr.tiffimage import _jpeg_markers
    head, rest = _jpeg_markers(stream)
    dht = b"".join(s[4:] for (m, s) in head if m == 0xC4)
    out = [s for (m, s) in head if m != 0xC4]
    out.append(b"\xff\xc4" + struct.pack(">H", 2 + len(dht)) + dht)
    out.append(b"\xff\xfe" + struct.pack(">H", 2 + 7) + b"fixture")
    assert rest[-2:] == b"\xff\xd9"
    return b"\xff\xd8" + b"".join(out) + b"\xff\xff" + rest[:-2] + b"\xff\xff\xff\xd9"


def entries(tmp):
    """name -> TIFF bytes."""
    from PIL import Image
    sys.path.insert(0, os.path.join(REPO, "omero-ms-image-region_amd"))
    import omr
    rgb = picture(150, 70, 1)
    odd = picture(101, 75, 2)
    out = {}

    def pillow(name, arr, **kw):
        f = io.BytesIO()
        Image.fromarray(arr).save(f, format="TIFF", compression="jpeg", tiffinfo={278: 16}, **kw)
        out[name] = f.getvalue()

    def ours(name, arr, **kw):
        path = os.path.join(tmp, name + ".tif")
        planes = np.moveaxis(arr, -1, 0)[None, :, None]      # [t][c][z][y][x]
        omr.write_tiled_tiff(path, planes, compression=7, samples_per_pixel=3, **kw)
        out[name] = open(path, "rb").read()

    pillow("grey_strips", np.ascontiguousarray(rgb[:, :, 1]), quality=80)
    pillow("rgb_strips", rgb, quality=80)
    for sub in ("4:4:4", "4:2:2", "4:2:0"):
        ours("ycc%s_tiles" % sub.replace(":", ""), rgb, tile=(80, 16), jpeg=dict(quality=85, subsampling=sub, tables="inline"))
    ours("ycc420_tiles_shared", rgb, tile=(80, 16), jpeg=dict(quality=85, subsampling="4:2:0", tables="shared"))
    ours("ycc420_rst_q30", rgb, tile=(80, 16), jpeg=dict(quality=30, subsampling="4:2:0", restart_blocks=3, tables="inline"))
    ours("ycc420_rst_q95_opt", rgb, tile=(80, 16),
         jpeg=dict(quality=95, subsampling="4:2:0", restart_blocks=3, optimize=True, tables="shared"))
    ours("ycc420_strips_odd", odd, rows_per_strip=16, jpeg=dict(quality=85, subsampling="4:2:0", tables="inline"))
    ours("ycc422_strips_odd", odd, rows_per_strip=16, jpeg=dict(quality=90, subsampling="4:2:2", tables="shared"))
    ours("rgb_tiles_rewritten", rgb, tile=(80, 16), jpeg=dict(quality=98, photometric="rgb", tables="inline", rewrite=rewrite_markers))
    return out


def build():
    import tempfile
    from PIL import Image
    sys.path.insert(0, os.path.join(REPO, "omero-ms-image-region_amd"))
    import omr
    arrays, met = {}, set()
    with tempfile.TemporaryDirectory() as tmp:
        for name, raw in entries(tmp).items():
            tables, segs, W, H, spp, photo = segments_of(raw)
            px = by_segments(raw)
            try:
                whole = np.asarray(Image.open(io.BytesIO(raw)))
                assert whole.shape == px.shape and np.array_equal(whole, px), name + ": libtiff and libjpeg-turbo differ"
                how = "libtiff == libjpeg-turbo"
            except (OSError, ValueError, SyntaxError) as e:
                how = "per-segment libjpeg-turbo decode only (Pillow: %s)" % e
            for (x, y, w, h, stream) in segs:
                met |= omr.jpeg_stream_forms(stream, tables)
                ours = omr.jpeg_decode_host(stream, w, h, spp, photo == 6, tables)
                part = px[y:y + h, x:x + w]
                assert np.array_equal(ours[:part.shape[0], :part.shape[1]], part), (name, x, y)
            print("%-22s %6d bytes  %s" % (name, len(raw), how))
            arrays[name + ".tif"] = np.frombuffer(raw, dtype=np.uint8)
            arrays[name + ".px"] = px
    missing = [f for f in FORMS if f not in met]
    assert not missing, "forms the fixture does not reach: %s" % missing
    np.savez_compressed(GOLDEN, **arrays)
    print("wrote %s: %d bytes, forms %s" % (GOLDEN, os.path.getsize(GOLDEN), sorted(met)))


def unpack(dst):
    """The fixture into dst for tools/jpeg_read_check.cpp: every file and its pixels (chunky), with
    index.txt (`name spp width height` per file), and every segment's stream as name.K.jpg beside
    name.tables, with streams.txt (`name K width height spp ycbcr tables_length` per stream)."""
    os.makedirs(dst, exist_ok=True)
    z = np.load(GOLDEN)
    with open(os.path.join(dst, "index.txt"), "w") as idx, open(os.path.join(dst, "streams.txt"), "w") as sidx:
        for key in z.files:
            if not key.endswith(".tif"):
                continue
            name = key[:-4]
            raw = z[key].tobytes()
            px = z[name + ".px"]
            open(os.path.join(dst, key), "wb").write(raw)
            px.tofile(os.path.join(dst, name + ".px"))
            idx.write("%s %d %d %d\n" % (name, 1 if px.ndim == 2 else px.shape[2], px.shape[1], px.shape[0]))
            tables, segs, W, H, spp, photo = segments_of(raw)
            open(os.path.join(dst, name + ".tables"), "wb").write(tables)
            for k, (x, y, w, h, stream) in enumerate(segs):
                open(os.path.join(dst, "%s.%d.jpg" % (name, k)), "wb").write(stream)
                sidx.write("%s %d %d %d %d %d %d\n" % (name, k, w, h, spp, int(photo == 6), len(tables)))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--unpack":
        unpack(sys.argv[2])
    else:
        build()
