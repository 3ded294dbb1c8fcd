#!/usr/bin/env python3
"""Writes tests/golden/tiff_j2k.npz: reversible JPEG 2000 codestreams and small TIFF files that hold
such streams in their segments (Compression 33003, 33004, 33005, 34712), as byte arrays, with the
pixels OpenJPEG decodes them to (NAME.px, or NAME.same naming the entry that holds the same pixels).

Run on a machine with Pillow (OpenJPEG inside: features.check("jpg_2000")); the tests that read the
fixture need neither.  For every stream the tool asserts that Pillow's decode equals the library's
host decoder byte for byte -- and, but for the two truncated streams, the source picture -- and
stores Pillow's pixels.  It then asserts that omr_j2k_stream_forms finds EVERY coding form of
_lib.J2K_FORM_NAMES somewhere in the fixture.

    python3 tools/make_tiff_j2k_golden.py                 # writes the fixture
    python3 tools/make_tiff_j2k_golden.py --unpack DIR    # the fixture's streams and files into DIR (for j2k-read-check)
"""
import io
import os
import struct
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "tiff_j2k.npz")
sys.path.insert(0, os.path.join(REPO, "omero-ms-image-region_amd"))


def picture(w, h, seed, channels=1):
    """uint8 [h][w] or [h][w][3]: smooth waves with a little noise, a busy patch and flat saturated patches."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    v = 128 + 90 * np.sin(x / 9.0) * np.cos(y / 7.0) + rng.normal(0, 5, (h, w))
    if channels == 3:
        v = np.stack([v, 0.8 * v + 20 * np.sin(y / 5.0), 255 - v], -1) + rng.normal(0, 3, (h, w, 3))
    v[h // 4:h // 2, w // 3:w // 2] = rng.integers(0, 256, size=v[h // 4:h // 2, w // 3:w // 2].shape)
    v[:max(h // 6, 1), :max(w // 6, 1)] = 255
    v[h - max(h // 6, 1):, w - max(w // 6, 1):] = 0
    return np.clip(v, 0, 255).astype(np.uint8)


def picture16(w, h, seed, noise):
    rng = np.random.default_rng(seed)
    if noise:
        return rng.integers(0, 65536, (h, w)).astype(np.uint16)
    y, x = np.mgrid[0:h, 0:w]
    return np.clip(30000 + 20000 * np.sin(x / 20.0) * np.cos(y / 15.0) + rng.normal(0, 12, (h, w)), 0, 65535).astype(np.uint16)


def streams():
    """name -> (source picture, Pillow save options, truncated)."""
    out = {}
    odd = picture(101, 75, 2, 3)
    for prog in ("LRCP", "RLCP", "RPCL", "PCRL", "CPRL"):
        out["rgb_101x75_" + prog.lower()] = (odd, dict(mct=1, num_resolutions=3, codeblock_size=(16, 16), precinct_size=(32, 32),
                                                     quality_mode="rates", quality_layers=[8, 1], progression=prog), False)
    out["grey_1x1"] = (np.array([[77]], np.uint8), {}, False)
    out["grey_33x40_nodwt"] = (picture(33, 40, 3), dict(num_resolutions=1), False)
    out["grey_41x37_cb4"] = (picture(41, 37, 4), dict(codeblock_size=(4, 4), num_resolutions=3), False)
    out["grey_150x70_cb64x16"] = (picture(150, 70, 5), dict(codeblock_size=(64, 16)), False)
    out["grey_1100x9_cb1024x4"] = (picture(1100, 9, 6), dict(codeblock_size=(1024, 4), num_resolutions=2), False)
    out["grey_zero_64"] = (np.zeros((64, 64), np.uint8), {}, False)
    out["grey_flat128_8_nodwt"] = (np.full((8, 8), 128, np.uint8), dict(num_resolutions=1), False)   # nothing coded: the tests cut its packet
    out["rgb_white_50"] = (np.full((50, 50, 3), 255, np.uint8), dict(mct=1), False)
    out["u16_noise_64"] = (picture16(64, 64, 7, True), {}, False)
    out["u16_smooth_128"] = (picture16(128, 128, 8, False), {}, False)
    out["rgb_128_truncated"] = (picture(128, 128, 9, 3), dict(mct=1, quality_mode="rates", quality_layers=[12, 6]), True)
    out["u16_96x80_truncated"] = (picture16(96, 80, 10, False), dict(quality_mode="rates", quality_layers=[5]), True)
    return out


def tiny_with_most_resolutions(encode):
    """A 5 x 3 picture at the largest num_resolutions the encoder takes: one-sample-wide subbands."""
    a = picture(5, 3, 11)
    for n in range(6, 0, -1):
        try:
            return "grey_5x3_res%d" % n, a, dict(num_resolutions=n), encode(a, dict(num_resolutions=n))
        except (OSError, ValueError):
            continue
    raise AssertionError("no num_resolutions accepted for 5 x 3")


def files(tmp):
    """name -> (TIFF bytes, [c][h][w] pixels): tiles of 64 x 32 on 150 x 70 and strips of 16 rows (the
    last of 6), 8-bit grey and RGB and 16-bit in both byte orders, every compression number once."""
    import omr
    out = {}
    grey, rgb, deep = picture(150, 70, 12), picture(150, 70, 13, 3), picture16(150, 70, 14, False)
    opts = dict(num_resolutions=3, codeblock_size=(32, 16))

    def one(name, planes, **kw):
        path = os.path.join(tmp, name + ".tif")
        omr.write_tiled_tiff(path, planes[None, :, None], jpeg2000=opts, **kw)
        out[name] = (open(path, "rb").read(), planes)

    one("grey_tiles_33003", grey[None], tile=(64, 32), compression=33003)
    one("grey_strips_34712", grey[None], rows_per_strip=16, compression=34712)
    one("rgb_tiles_33005", np.ascontiguousarray(np.moveaxis(rgb, -1, 0)), tile=(64, 32), compression=33005, samples_per_pixel=3)
    one("u16le_tiles_33004", deep[None], tile=(64, 32), compression=33004, byteorder="<")
    one("u16be_strips_34712", deep[None], rows_per_strip=16, compression=34712, byteorder=">")
    return out


def tiff_segments(raw):
    """[(x, y, w, h, stream)], W, H, spp, bits, big-endian of the first IFD of a classic TIFF."""
    bo = "<" if raw[:2] == b"II" else ">"
    at = struct.unpack_from(bo + "I", raw, 4)[0]
    t = {}
    for k in range(struct.unpack_from(bo + "H", raw, at)[0]):
        tag, typ, cnt = struct.unpack_from(bo + "HHI", raw, at + 2 + 12 * k)
        size = {1: 1, 2: 1, 3: 2, 4: 4, 7: 1}[typ] * cnt
        pos = at + 2 + 12 * k + 8
        if size > 4:
            pos = struct.unpack_from(bo + "I", raw, pos)[0]
        t[tag] = list(struct.unpack(bo + "%d%s" % (cnt, {1: "B", 3: "H", 4: "I", 7: "B"}[typ]), raw[pos:pos + size]))
    W, H = t[256][0], t[257][0]
    if 322 in t:
        tw, th = t[322][0], t[323][0]
        boxes = [(x, y, tw, th) for y in range(0, H, th) for x in range(0, W, tw)]
        offs, cnts = t[324], t[325]
    else:
        rps = min(t[278][0], H)
        boxes = [(0, y, W, min(rps, H - y)) for y in range(0, H, rps)]
        offs, cnts = t[273], t[279]
    return [b + (bytes(raw[o:o + c]),) for b, o, c in zip(boxes, offs, cnts)], W, H, t.get(277, [1])[0], t[258][0], bo == ">"


def build():
    import tempfile
    from PIL import Image
    import omr
    from omr import _lib
    from omr.tiffimage import _j2k_encode
    arrays, met = {}, set()

    def store(key, px):
        """The pixels under key, or -- several entries hold the same picture -- the key that has them."""
        for other, have in arrays.items():
            if other.endswith(".px") and have.dtype == px.dtype and have.shape == px.shape and np.array_equal(have, px):
                arrays[key[:-3] + ".same"] = np.array(other)
                return
        arrays[key] = px

    def pin(name, a, stream, truncated):
        ref = np.asarray(Image.open(io.BytesIO(stream)))
        assert ref.shape == a.shape and ref.dtype == a.dtype, (name, ref.shape, ref.dtype)
        assert truncated != np.array_equal(ref, a), name + (": not truncated" if truncated else ": not lossless")
        h, w = a.shape[:2]
        ours = omr.j2k_decode_host(stream, w, h, 1 if a.ndim == 2 else 3, 8 * a.dtype.itemsize)
        assert ours.dtype == ref.dtype and np.array_equal(ours, ref), name + ": the host decoder and OpenJPEG differ"
        forms = omr.j2k_stream_forms(stream)
        met.update(forms)
        return ref, forms

    for name, (a, opt, truncated) in streams().items():
        stream = _j2k_encode(a, opt)
        ref, forms = pin(name, a, stream, truncated)
        arrays["s." + name + ".j2k"] = np.frombuffer(stream, dtype=np.uint8)
        store("s." + name + ".px", ref)
        print("%-26s %6d bytes  %2d forms%s" % (name, len(stream), len(forms), "  (truncated: OpenJPEG's pixels)" if truncated else ""))
    name, a, opt, stream = tiny_with_most_resolutions(_j2k_encode)
    ref, forms = pin(name, a, stream, False)
    arrays["s." + name + ".j2k"] = np.frombuffer(stream, dtype=np.uint8)
    store("s." + name + ".px", ref)
    print("%-26s %6d bytes  %2d forms" % (name, len(stream), len(forms)))
    with tempfile.TemporaryDirectory() as tmp:
        for name, (raw, planes) in files(tmp).items():
            segs, W, H, spp, bits, big = tiff_segments(raw)
            for (x, y, w, h, stream) in segs:
                ref = np.asarray(Image.open(io.BytesIO(stream)))
                ours = omr.j2k_decode_host(stream, w, h, spp, bits)
                assert np.array_equal(ours, ref), (name, x, y)
                part = planes[:, y:y + h, x:x + w]
                got = ref[None] if spp == 1 else np.moveaxis(ref, -1, 0)
                assert np.array_equal(got[:, :part.shape[1], :part.shape[2]], part), (name, x, y)
                met.update(omr.j2k_stream_forms(stream))
            with omr.TiffImage(os.path.join(tmp, name + ".tif"), 1, spp, 1, accept=("jpeg2000", "samples")) as img:
                for c in range(spp):
                    assert np.array_equal(img.get_tile(0, 0, c, 0, 0, 0, W, H), planes[c]), (name, c)
            arrays[name + ".tif"] = np.frombuffer(raw, dtype=np.uint8)
            store(name + ".px", planes)
            print("%-26s %6d bytes  %d segments" % (name, len(raw), len(segs)))
    missing = [f for f in _lib.J2K_FORM_NAMES if f not in met]
    assert not missing, "forms the fixture does not reach: %s" % missing
    np.savez_compressed(GOLDEN, **arrays)
    print("wrote %s: %d bytes, all %d forms met" % (GOLDEN, os.path.getsize(GOLDEN), len(_lib.J2K_FORM_NAMES)))


def pixels_of(z, name):
    return z[name + ".px"] if name + ".px" in z.files else z[str(z[name + ".same"])]


def unpack(dst):
    """The fixture into dst for tools/j2k_read_check.cpp: every stream as name.j2k with its pixels
    name.px (chunky, host byte order) and streams.txt (`name width height samples bits` per stream);
    every file as name.tif with its pixels name.tif.px ([c][h][w], host byte order) and files.txt
    (`name width height channels bits` per file)."""
    os.makedirs(dst, exist_ok=True)
    z = np.load(GOLDEN)
    with open(os.path.join(dst, "streams.txt"), "w") as sidx, open(os.path.join(dst, "files.txt"), "w") as fidx:
        for key in z.files:
            if key.startswith("s.") and key.endswith(".j2k"):
                name = key[2:-4]
                px = pixels_of(z, "s." + name)
                open(os.path.join(dst, name + ".j2k"), "wb").write(z[key].tobytes())
                px.tofile(os.path.join(dst, name + ".px"))
                sidx.write("%s %d %d %d %d\n" % (name, px.shape[1], px.shape[0], 1 if px.ndim == 2 else 3, 8 * px.dtype.itemsize))
            elif key.endswith(".tif"):
                name = key[:-4]
                px = pixels_of(z, name)
                open(os.path.join(dst, key), "wb").write(z[key].tobytes())
                px.tofile(os.path.join(dst, key + ".px"))
                fidx.write("%s %d %d %d %d\n" % (name, px.shape[2], px.shape[1], px.shape[0], 8 * px.dtype.itemsize))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--unpack":
        unpack(sys.argv[2])
    else:
        build()
