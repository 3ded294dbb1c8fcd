"""TiffImage: tiled TIFF / OME-TIFF pixel data (K13), and write_tiled_tiff, the small writer that
makes the test and probe files.

The second backend of pixelsService.getPixelBuffer beside the ROMIO file (pixbuf.PixelBuffer):
pyramidal OME-TIFF as raw2ometiff writes it, one IFD per plane and the lower resolutions in
SubIFDs.  Reads go through libomr.so: get_tile on the host (plain serial LZW decoder), read_regions
and render_tiles with the LZW segments decoded on the GPU (omr_tiffread.hip).  With accept=...
(omr_tiff_image_open_ex) also Deflate and zstd segments, the floating-point predictor and chunky
pixels of several samples (RGB), each channel one sample, and with "jpeg" baseline JPEG segments
(Compression 7, K17: omr_jpegdec.hip), grey, RGB or YCbCr converted to RGB, and with "jpeg2000"
reversible JPEG 2000 codestreams (Compression 33003, 33004, 33005, 34712, K19: omr_j2kdec.hip), with
"jpeg2000-lossy" irreversible ones (K20).
"""
import ctypes
import struct
import zlib

import numpy as np

from . import _lib
from ._lib import lib
from ._segimage import _SegImage

_NP_NAMES = {_lib.PIXELS_INT8: "i1", _lib.PIXELS_UINT8: "u1", _lib.PIXELS_INT16: "i2", _lib.PIXELS_UINT16: "u2",
             _lib.PIXELS_INT32: "i4", _lib.PIXELS_UINT32: "u4", _lib.PIXELS_FLOAT: "f4", _lib.PIXELS_DOUBLE: "f8"}
DIMENSION_ORDERS = ("XYZCT", "XYZTC", "XYCZT", "XYCTZ", "XYTZC", "XYTCZ")


def lzw_encode(data, early_clear=0, eoi=True):
    """TIFF LZW as libtiff writes it: MSB-first codes from 9 bits, Clear (256) first, EOI (257)
    last; the writer widens when its own next entry reaches 512, 1024 and 2048 (the reader, one
    entry behind, when its reaches 511, 1023, 2047: "early change") and clears at 4094.
    early_clear = k > 0: a Clear after every k entries as well.  eoi = False: no EOI code."""
    data = bytes(data)
    out = bytearray()
    acc = nbits = 0

    def put(code, width):
        nonlocal acc, nbits
        acc = (acc << width) | code
        nbits += width
        while nbits >= 8:
            nbits -= 8
            out.append((acc >> nbits) & 0xFF)
        acc &= (1 << nbits) - 1

    width, nxt, table = 9, 258, {}
    put(256, width)
    if data:
        w = data[0]
        for c in data[1:]:
            key = (w << 8) | c
            hit = table.get(key)
            if hit is not None:
                w = hit
                continue
            put(w, width)
            table[key] = nxt
            nxt += 1
            if nxt in (512, 1024, 2048):
                width += 1
            if nxt == 4094 or (early_clear and nxt - 258 >= early_clear):
                put(256, width)
                width, nxt, table = 9, 258, {}
            w = c
        put(w, width)
        nxt += 1
        if nxt == 4094:
            put(256, width)
            width = 9
        elif nxt in (512, 1024, 2048):
            width += 1
    if eoi:
        put(257, width)
    if nbits:
        out.append((acc << (8 - nbits)) & 0xFF)
    return bytes(out)


class _LzwJob:
    """lzw_encode with its options, picklable for a process pool's map."""

    def __init__(self, early_clear, eoi):
        self.early_clear, self.eoi = early_clear, eoi

    def __call__(self, raw):
        return lzw_encode(raw, self.early_clear, self.eoi)


def _predict(seg, k=1):
    """Horizontal differencing (Predictor 2) of a [rows][cols] array, in the sample's own width;
    with k interleaved samples per pixel, per component: k columns apart."""
    u = np.ascontiguousarray(seg.astype(seg.dtype.newbyteorder("="))).view("u%d" % seg.dtype.itemsize)
    d = u.copy()
    d[:, k:] = u[:, k:] - u[:, :-k]
    return d


def _predict_fp(seg):
    """The floating-point predictor (Predictor 3, libtiff's fpDiff) of a [rows][cols] float array:
    each row as byte planes, the most significant byte of every sample first (whatever the file's
    byte order), then byte differences (mod 256) along the whole row.  Returns [rows][cols * B] u1."""
    rows, cols = seg.shape
    b = np.ascontiguousarray(seg.astype(seg.dtype.newbyteorder(">"))).view("u1").reshape(rows, cols, seg.dtype.itemsize)
    b = np.ascontiguousarray(b.transpose(0, 2, 1)).reshape(rows, -1)
    d = b.copy()
    d[:, 1:] = b[:, 1:] - b[:, :-1]
    return d


def _jpeg_markers(stream):
    """A JPEG stream as ([(marker, whole marker segment) up to SOS, SOI left out], the rest from SOS on)."""
    assert stream[:2] == b"\xff\xd8"
    pos, out = 2, []
    while True:
        assert stream[pos] == 0xFF
        m = stream[pos + 1]
        if m == 0xDA:
            return out, stream[pos:]
        n = struct.unpack_from(">H", stream, pos + 2)[0]
        out.append((m, stream[pos:pos + 2 + n]))
        pos += 2 + n


def _jpeg_encode(seg, opt):
    """One segment ([rows][cols] or [rows][cols][3] uint8) as a whole baseline JFIF stream, by Pillow."""
    import io
    from PIL import Image
    im = Image.fromarray(np.ascontiguousarray(seg))
    kw = dict(format="JPEG", quality=int(opt.get("quality", 85)), optimize=bool(opt.get("optimize", False)))
    if opt.get("restart_blocks"):
        kw["restart_marker_blocks"] = int(opt["restart_blocks"])
    if seg.ndim == 3:
        if opt.get("photometric", "ycbcr") == "rgb":
            kw.update(keep_rgb=True, subsampling="4:4:4")
        else:
            kw["subsampling"] = opt.get("subsampling", "4:4:4")
    f = io.BytesIO()
    im.save(f, **kw)
    return f.getvalue()


def _j2k_encode(seg, opt):
    """One segment ([rows][cols] uint8 or uint16, or [rows][cols][3] uint8) as a raw JPEG 2000
    codestream, by Pillow's OpenJPEG; opt: Pillow's save options (num_resolutions, codeblock_size,
    precinct_size, quality_mode, quality_layers, progression, mct ...); reversible unless opt says
    "irreversible": True (the 9/7 transform, K20)."""
    import io
    from PIL import Image
    kw = dict(opt)
    kw.pop("rewrite", None)
    kw.update(format="JPEG2000", no_jp2=True, irreversible=bool(opt.get("irreversible", False)))
    f = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(seg)).save(f, **kw)
    return f.getvalue()


class _J2kJob:
    """_j2k_encode with its options, picklable for a process pool's map."""

    def __init__(self, opt):
        self.opt = {k: v for k, v in opt.items() if k != "rewrite"}

    def __call__(self, seg):
        return _j2k_encode(seg, self.opt)


def _zstd_job(raw):
    from .zarrimage import zstd_encode
    return zstd_encode(raw)


def write_tiled_tiff(path, planes, levels=(), tile=(256, 256), rows_per_strip=None, byteorder="<", bigtiff=False,
                     compression=1, predictor=1, early_clear=0, eoi=True, dimension_order="XYZCT",
                     skip_zero_segments=False, tag_overrides=None, mapper=map, samples_per_pixel=1, encoder=None,
                     jpeg=None, jpeg2000=None):
    """Write a [t][c][z][y][x] array as a TIFF with one IFD per plane (in `dimension_order`), and
    `levels` (arrays of the same [t][c][z] with their own [y][x]) as SubIFDs of each plane.
    tile = (w, h), or rows_per_strip = n for strips; byteorder "<" (II) or ">" (MM); compression 1,
    5 (LZW, lzw_encode with early_clear / eoi), 8 or 32946 (Deflate: zlib.compress) or 50000
    (omr.zstd_encode); predictor 1, 2 (integer samples up to 32 bits) or 3 (float32 and float64,
    one sample per pixel); samples_per_pixel = k > 1: every k consecutive channels are interleaved
    into one chunky IFD (tags 277 = k, 284 = 1, Photometric 2 from three samples on, the others
    ExtraSamples), predictor 2 then k samples apart, and the chain holds c / k IFDs per (z, t);
    skip_zero_segments: an all-zero segment is written with byte count 0; tag_overrides = {tag:
    value} replaces the value written for a SHORT tag (to make files a reader must reject); mapper:
    a map() that encodes the segments of one image, e.g. a multiprocessing pool's for big files;
    encoder: a function bytes -> bytes in place of the codec's own (libzstd's, say, for 50000).
    compression 7 (uint8, one sample or three): baseline JPEG segments encoded by Pillow (imported
    here, a test and tooling aid), edge tiles padded by edge replication; jpeg = {"quality": 85,
    "subsampling": "4:4:4" | "4:2:2" | "4:2:0", "restart_blocks": MCUs per restart interval,
    "optimize": False, "photometric": "ycbcr" | "rgb" for three samples (a single sample is grey),
    "tables": "inline" (whole streams) | "shared" (the first segment's DQT / DHT in tag 347 and
    every marker segment equal to one of them cut out of the streams)}.
    compression 33003, 33004, 33005 or 34712 (uint8 with one sample or three, uint16 with one):
    one raw reversible JPEG 2000 codestream per segment, encoded by Pillow's OpenJPEG (a test and
    tooling aid as well), edge tiles padded by edge replication and a last strip coded at its own
    height; jpeg2000 = Pillow's save options ({"num_resolutions": 3, "codeblock_size": (16, 16),
    "precinct_size": (32, 32), "quality_mode": "rates", "quality_layers": [8, 1], "progression":
    "RPCL", "mct": 1 ...}), "irreversible": True for the 9/7 transform (the default is the reversible
    5/3 one) and "rewrite": a function stream -> stream.
    Returns {"ifds": [offset per plane], "subifds": [[offsets] per plane]}."""
    planes = np.asarray(planes)
    assert planes.ndim == 5, "planes must be [t][c][z][y][x]"
    levels = [np.asarray(lv) for lv in levels]
    st, sc, sz = planes.shape[:3]
    spp = int(samples_per_pixel)
    assert 1 <= spp and sc % spp == 0, "samples_per_pixel must divide the channel count"
    assert predictor != 3 or (planes.dtype.kind == "f" and spp == 1), "predictor 3: float samples, one per pixel"
    for lv in levels:
        assert lv.ndim == 5 and lv.shape[:3] == planes.shape[:3] and lv.dtype == planes.dtype
    assert dimension_order in DIMENSION_ORDERS
    dt = planes.dtype
    kind = {"u": 1, "i": 2, "f": 3}[dt.kind]
    bo = byteorder
    fdt = dt.newbyteorder(bo) if dt.itemsize > 1 else dt
    tag_overrides = dict(tag_overrides or {})
    jpeg = dict(jpeg or {})
    if compression == 7:
        assert dt == np.uint8 and spp in (1, 3) and predictor == 1, "JPEG: uint8, one or three samples, no predictor"
    jpeg_ycc = compression == 7 and spp == 3 and jpeg.get("photometric", "ycbcr") != "rgb"
    j2k = compression in _lib.J2K_COMPRESSIONS
    jpeg2000 = dict(jpeg2000 or {})
    if j2k:
        assert predictor == 1 and ((dt == np.uint8 and spp in (1, 3)) or (dt == np.uint16 and spp == 1)), \
            "JPEG 2000: uint8 with one or three samples or uint16 with one, no predictor"
    buf = bytearray(b"II" if bo == "<" else b"MM")
    if bigtiff:
        buf += struct.pack(bo + "HHHQ", 43, 8, 0, 0)
    else:
        buf += struct.pack(bo + "HI", 42, 0)
    osz, ofmt = (8, "Q") if bigtiff else (4, "I")

    def segments(img):
        """(offsets, counts, geometry tags) of one image; the data goes into buf."""
        h, w = img.shape[:2]
        if rows_per_strip is None:
            tw, th = tile
            boxes = [(x, y, tw, th) for y in range(0, h, th) for x in range(0, w, tw)]
        else:
            boxes = [(0, y, w, min(rows_per_strip, h - y)) for y in range(0, h, rows_per_strip)]
        raws = []
        shared = None
        for (x, y, bw, bh) in boxes if compression == 7 else ():
            part = img[y:y + bh, x:x + bw]
            pad = [(0, bh - part.shape[0]), (0, bw - part.shape[1])] + [(0, 0)] * (img.ndim - 2)
            stream = _jpeg_encode(np.pad(part, pad, mode="edge"), jpeg)
            if jpeg.get("rewrite"):                      # a function stream -> stream (the fixture's marker rewrites)
                stream = jpeg["rewrite"](stream)
            if jpeg.get("tables", "inline") == "shared":
                head, rest = _jpeg_markers(stream)
                if shared is None:
                    shared = [s for (m, s) in head if m in (0xDB, 0xC4)]
                stream = b"\xff\xd8" + b"".join(s for (m, s) in head if s not in shared) + rest
            raws.append(stream)
        if j2k:
            parts = []
            for (x, y, bw, bh) in boxes:
                part = img[y:y + bh, x:x + bw]
                pad = [(0, bh - part.shape[0]), (0, bw - part.shape[1])] + [(0, 0)] * (img.ndim - 2)
                parts.append(np.pad(part, pad, mode="edge"))
            raws = list(mapper(_J2kJob(jpeg2000), parts))
            if jpeg2000.get("rewrite"):
                raws = [jpeg2000["rewrite"](r) for r in raws]
        for (x, y, bw, bh) in () if compression == 7 or j2k else boxes:
            seg = np.zeros((bh, bw) + img.shape[2:], dtype=fdt)
            part = img[y:y + bh, x:x + bw]
            seg[:part.shape[0], :part.shape[1]] = part
            if skip_zero_segments and not part.any():
                raws.append(None)
                continue
            seg = seg.reshape(bh, -1)                    # chunky: bw * spp samples per row
            if predictor == 2:
                seg = _predict(seg, spp).astype(np.dtype("u%d" % dt.itemsize).newbyteorder(bo) if dt.itemsize > 1 else "u1")
            elif predictor == 3:
                seg = _predict_fp(seg)
            raws.append(seg.tobytes())
        job = {5: _LzwJob(early_clear, eoi), 8: zlib.compress, 32946: zlib.compress, 50000: _zstd_job}.get(compression)
        if encoder is not None and job is not None:
            job = encoder
        if job is not None:
            todo = [r for r in raws if r is not None]
            done = iter(list(mapper(job, todo)))
            raws = [None if r is None else next(done) for r in raws]
        offs, cnts = [], []
        for raw in raws:
            if raw is None:
                offs.append(0)
                cnts.append(0)
                continue
            if len(buf) % 2:
                buf.append(0)
            offs.append(len(buf))
            cnts.append(len(raw))
            buf.extend(raw)
        if rows_per_strip is None:
            geom = [(322, "H", [tile[0]]), (323, "H", [tile[1]]), (324, ofmt, offs), (325, ofmt, cnts)]
        else:
            geom = [(273, ofmt, offs), (278, "I", [rows_per_strip]), (279, ofmt, cnts)]
        if shared is not None:
            geom.append((347, "B", list(b"\xff\xd8" + b"".join(shared) + b"\xff\xd9")))
        return geom

    def ifd_entries(img, n_sub):
        h, w = img.shape[:2]
        ent = [(256, "I", [w]), (257, "I", [h]), (258, "H", [8 * dt.itemsize] * spp), (259, "H", [compression]),
               (262, "H", [2 if spp >= 3 else 1]), (277, "H", [spp]), (284, "H", [1]), (339, "H", [kind] * spp)]
        n_extra = spp - 3 if spp >= 3 else spp - 1
        if n_extra:
            ent.append((338, "H", [0] * n_extra))        # ExtraSamples: unspecified data
        if predictor != 1 or 317 in tag_overrides:
            ent.append((317, "H", [predictor]))
        if compression == 7 and spp == 3:
            ent = [e for e in ent if e[0] != 262] + [(262, "H", [6 if jpeg_ycc else 2])]
            if jpeg_ycc:
                hv = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}[jpeg.get("subsampling", "4:4:4")]
                ent.append((530, "H", list(hv)))
        if 266 in tag_overrides:
            ent.append((266, "H", [1]))
        ent += segments(img)
        if n_sub:
            ent.append((330, ofmt, [0] * n_sub))     # patched once the SubIFDs have their places
        ent = [(t, f, [tag_overrides[t]] if t in tag_overrides else v) for (t, f, v) in ent]
        return sorted(ent)

    tcode = {"H": 3, "I": 4, "Q": 16, "B": 7}

    def emit_ifd(ent, next_at_end=True):
        """Out-of-line values, then the IFD itself; returns (ifd offset, {tag: position of its values})."""
        where = {}
        fields = []
        for (t, f, v) in ent:
            raw = struct.pack(bo + f * len(v), *v)
            if len(raw) <= osz:
                fields.append(raw.ljust(osz, b"\0"))
                where[t] = None
            else:
                if len(buf) % 2:
                    buf.append(0)
                where[t] = len(buf)
                fields.append(struct.pack(bo + ofmt, len(buf)))
                buf.extend(raw)
        if len(buf) % 2:
            buf.append(0)
        at = len(buf)
        buf.extend(struct.pack(bo + ("Q" if bigtiff else "H"), len(ent)))
        for (t, f, v), field in zip(ent, fields):
            if where[t] is None:
                where[t] = len(buf) + (12 if bigtiff else 8)
            buf.extend(struct.pack(bo + "HH" + ofmt, t, tcode[f], len(v)) + field)
        buf.extend(struct.pack(bo + ofmt, 0))            # next IFD: patched by the caller
        return at, where

    # plane order along the chain: the first letter behind XY varies fastest
    sizes = {"Z": sz, "C": sc // spp, "T": st}
    order = dimension_order[2:]
    result = {"ifds": [], "subifds": []}
    prev_next = 8 if bigtiff else 4                         # where the offset of the next main IFD goes
    n_planes = sz * (sc // spp) * st

    def image_of(a, t, c, z):
        """The pixels of IFD (t, c, z): [y][x], or [y][x][spp] of the channels c * spp .. interleaved."""
        return a[t, c, z] if spp == 1 else np.moveaxis(a[t, c * spp:(c + 1) * spp, z], 0, -1)

    for k in range(n_planes):
        idx, r = {}, k
        for letter in order:
            idx[letter] = r % sizes[letter]
            r //= sizes[letter]
        t, c, z = idx["T"], idx["C"], idx["Z"]
        subs = []
        for lv in levels:
            at, _ = emit_ifd(ifd_entries(image_of(lv, t, c, z), 0))
            subs.append(at)
        at, where = emit_ifd(ifd_entries(image_of(planes, t, c, z), len(subs)))
        if subs:
            struct.pack_into(bo + ofmt * len(subs), buf, where[330], *subs)
        struct.pack_into(bo + ofmt, buf, prev_next, at)
        n_ent = struct.unpack_from(bo + ("Q" if bigtiff else "H"), buf, at)[0]
        prev_next = at + ((8 + 20 * n_ent) if bigtiff else (2 + 12 * n_ent))
        result["ifds"].append(at)
        result["subifds"].append(subs)
    with open(path, "wb") as f:
        f.write(buf)
    return result


class TiffImage(_SegImage):
    """An open tiled TIFF / OME-TIFF (omr_tiff_image).  The caller gives Z, C, T and the dimension
    order as for PixelBuffer; OME-XML is not parsed."""

    _CLOSE, _GET_TILE = "omr_tiff_image_close", "omr_tiff_image_get_tile"
    _READ_REGIONS, _RENDER_TILES = "omr_tiff_image_read_regions_device", "omr_render_tiff_tiles"

    def __init__(self, path, size_z=1, size_c=1, size_t=1, dimension_order="XYZCT", accept=()):
        """accept: the further forms a file may use, any of "deflate", "zstd", "predictor3" and
        "samples", "jpeg", "jpeg2000" and "jpeg2000-lossy" (omr_tiff_image_open_ex); empty: the plain open, which refuses them all.  size_c
        counts every sample of a chunky image as a channel (3 for an RGB image)."""
        h = ctypes.c_void_p()
        accept = (accept,) if isinstance(accept, str) else tuple(accept)
        if not accept:
            st = lib.omr_tiff_image_open(str(path).encode(), int(size_z), int(size_c), int(size_t),
                                         str(dimension_order).encode(), ctypes.byref(h))
        else:
            bits = 0
            for name in accept:
                if name not in _lib.TIFF_ACCEPT:
                    raise _lib.OmrError(_lib.INVALID_ARGUMENT, f"unknown TIFF form {name!r}")
                bits |= _lib.TIFF_ACCEPT[name]
            opt = _lib.TiffOpenOptions(ctypes.sizeof(_lib.TiffOpenOptions), bits)
            st = lib.omr_tiff_image_open_ex(str(path).encode(), int(size_z), int(size_c), int(size_t),
                                            str(dimension_order).encode(), ctypes.byref(opt), ctypes.byref(h))
        if st != _lib.OK:
            raise _lib.OmrError(st, f"cannot open TIFF image {path}")
        self.h = h
        i = _lib.TiffInfo()
        _lib.check(lib.omr_tiff_image_info(self.h, ctypes.byref(i)))
        self.info = {n: int(getattr(i, n)) for n, _ in _lib.TiffInfo._fields_}
        self.size_x, self.size_y = i.size_x, i.size_y
        self.size_z, self.size_c, self.size_t = i.size_z, i.size_c, i.size_t
        self.pixel_type = i.pixel_type
        self.samples_per_pixel = int(lib.omr_tiff_image_samples_per_pixel(self.h))
        self.big_endian = bool(i.big_endian)
        self.dtype = np.dtype((">" if self.big_endian else "<") + _NP_NAMES[self.pixel_type])
        sizes = (ctypes.c_int32 * (2 * i.n_levels))()
        n = lib.omr_tiff_image_level_sizes(self.h, sizes, i.n_levels)
        self.level_sizes = [[sizes[2 * k], sizes[2 * k + 1]] for k in range(n)]


def lzw_decode_host(stream, expected):
    """The host LZW decoder alone (omr_lzw_decode_host): `expected` bytes, or OmrError(INTERNAL)."""
    src = np.frombuffer(bytes(stream), dtype=np.uint8)
    out = np.zeros(max(int(expected), 1), dtype=np.uint8)
    _lib.check(lib.omr_lzw_decode_host(src.ctypes.data if src.size else None, src.size, out.ctypes.data, int(expected)))
    return out[:int(expected)].tobytes()


def _decode_host_frame(call, stream, width, height, samples, dtype=np.uint8, tables=None, failed=None):
    """The buffers of a host decode of one frame: call(tables pointer, tables size, source pointer,
    source size, output pointer, why buffer, its size) -> status; anything but OK raises OmrError
    with `failed`, or with what the call wrote into the why buffer.  Returns [height][width] or
    [height][width][samples] of dtype."""
    src = np.frombuffer(bytes(stream), dtype=np.uint8)
    tab = np.frombuffer(bytes(tables or b""), dtype=np.uint8)
    n = int(width) * int(height) * int(samples)
    out = np.zeros(max(n, 1), dtype=dtype)
    why = ctypes.create_string_buffer(160)
    st = call(tab.ctypes.data if tab.size else None, tab.size, src.ctypes.data if src.size else None, src.size,
              out.ctypes.data, why, 160)
    if st != _lib.OK:
        raise _lib.OmrError(st, failed or why.value.decode())
    out = out[:n]
    return out.reshape(height, width) if samples == 1 else out.reshape(height, width, samples)


def jpeg_decode_host(stream, width, height, samples=1, ycbcr=False, tables=None):
    """The host JPEG decoder alone (omr_jpeg_decode_host): [height][width] or [height][width][3]
    uint8, or OmrError (INVALID_ARGUMENT: a form out of scope, named in the message; INTERNAL: damage)."""
    return _decode_host_frame(
        lambda tab, ntab, src, nsrc, out, why, nwhy: lib.omr_jpeg_decode_host(
            tab, ntab, src, nsrc, int(width), int(height), int(samples), int(bool(ycbcr)), out, why, nwhy),
        stream, width, height, samples, tables=tables)


def jpeg_decode_host_split(stream, width, height, samples=1, ycbcr=False, tables=None, subsequence_bits=1024, lanes=256):
    """jpeg_decode_host with the entropy decode done as K18 does it (omr_jpeg_decode_host_split): a
    workgroup of `lanes` lanes over subsequences of subsequence_bits bits, played by host loops.
    Returns (pixels, stats): the pixels and errors of jpeg_decode_host, and a dict with the
    subsequences, rounds, max_settle_iterations and redecodes of the decode."""
    stats = _lib.JpegSplitStats()
    px = _decode_host_frame(
        lambda tab, ntab, src, nsrc, out, why, nwhy: lib.omr_jpeg_decode_host_split(
            tab, ntab, src, nsrc, int(width), int(height), int(samples), int(bool(ycbcr)), int(subsequence_bits),
            int(lanes), out, ctypes.byref(stats)),
        stream, width, height, samples, tables=tables, failed="jpeg: split decode failed")
    return px, {f: int(getattr(stats, f)) for f, _ in _lib.JpegSplitStats._fields_}


def jpeg_stream_forms(stream, tables=None):
    """The forms a good stream uses (omr_jpeg_stream_forms), as a set of names of _lib.JPEG_FORM_NAMES."""
    src = np.frombuffer(bytes(stream), dtype=np.uint8)
    tab = np.frombuffer(bytes(tables or b""), dtype=np.uint8)
    bits = ctypes.c_uint32(0)
    _lib.check(lib.omr_jpeg_stream_forms(tab.ctypes.data if tab.size else None, tab.size,
                                         src.ctypes.data if src.size else None, src.size, ctypes.byref(bits)))
    return {n for k, n in enumerate(_lib.JPEG_FORM_NAMES) if bits.value >> k & 1}


def j2k_decode_host(stream, width, height, samples=1, bits=8):
    """The host JPEG 2000 decoder alone (omr_j2k_decode_host): [height][width] or [height][width][3],
    uint8 or uint16, or OmrError (INVALID_ARGUMENT: a form out of scope, named in the message;
    INTERNAL: damage)."""
    return _decode_host_frame(
        lambda tab, ntab, src, nsrc, out, why, nwhy: lib.omr_j2k_decode_host(
            src, nsrc, int(width), int(height), int(samples), int(bits), out, why, nwhy),
        stream, width, height, samples, dtype=np.uint16 if bits == 16 else np.uint8)


def j2k_stream_forms(stream):
    """The coding forms a good codestream uses (omr_j2k_stream_forms), as a set of names of _lib.J2K_FORM_NAMES."""
    src = np.frombuffer(bytes(stream), dtype=np.uint8)
    bits = ctypes.c_uint64(0)
    _lib.check(lib.omr_j2k_stream_forms(src.ctypes.data if src.size else None, src.size, ctypes.byref(bits)))
    return {n for k, n in enumerate(_lib.J2K_FORM_NAMES) if bits.value >> k & 1}


def _decode_batch_device(ctx, streams, sizes, samples, bytes_per_sample, view, call):
    """The buffers of a batch decode on ctx's GPU: streams[i] with a frame of sizes[i] = (width,
    height) and samples of bytes_per_sample bytes; call(blob, offsets, lengths, widths, heights,
    n, output, output offsets, statuses) -> status makes the lib call, all but n as addresses.  The
    outputs lie 16-byte aligned with at least 16 guard bytes of 0xA5 behind each, which must come
    back untouched.  Returns ([arrays, [h][w] or [h][w][samples], viewed as `view`], [status per stream])."""
    import torch
    n = len(streams)
    blob = np.frombuffer(b"".join(bytes(s) for s in streams) or b"\0", dtype=np.uint8)
    lens = np.array([len(s) for s in streams], dtype=np.uint32)
    offs = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]).astype(np.uint64) if n else np.zeros(0, np.uint64)
    ws = np.array([int(w) for w, _ in sizes], dtype=np.int32)
    hs = np.array([int(h) for _, h in sizes], dtype=np.int32)
    nbytes = [int(w) * int(h) * samples * bytes_per_sample for w, h in sizes]
    doffs = np.array([sum((b + 31) // 16 * 16 for b in nbytes[:i]) for i in range(n)], dtype=np.uint64)
    total = sum((b + 31) // 16 * 16 for b in nbytes)
    out = torch.full((max(total, 16),), 0xA5, dtype=torch.uint8, device=f"cuda:{ctx.device}")
    ctx.order_after_torch()
    status = np.zeros(max(n, 1), dtype=np.int32)
    _lib.check(call(blob.ctypes.data, offs.ctypes.data, lens.ctypes.data, ws.ctypes.data, hs.ctypes.data, n, out.data_ptr(),
                    doffs.ctypes.data, status.ctypes.data), ctx.h)
    host = out.cpu().numpy()
    got = []
    for i, (w, h) in enumerate(sizes):
        a = host[int(doffs[i]):int(doffs[i]) + nbytes[i]]
        assert (host[int(doffs[i]) + nbytes[i]:int(doffs[i]) + (nbytes[i] + 31) // 16 * 16] == 0xA5).all(), "bytes behind a stream overwritten"
        a = a.view(view)
        got.append(a.reshape(h, w) if samples == 1 else a.reshape(h, w, samples))
    return got, [int(v) for v in status[:n]]


def j2k_decode_batch_device(ctx, streams, sizes, samples=1, bits=8):
    """K19 alone (omr_j2k_decode_batch_device): streams[i] with a frame of sizes[i] = (width, height),
    decoded on ctx's GPU.  Returns ([arrays, [h][w] or [h][w][3], uint8 or uint16], [status per stream])."""
    return _decode_batch_device(
        ctx, streams, sizes, samples, bits // 8, "<u2" if bits == 16 else "u1",
        lambda blob, offs, lens, ws, hs, n, out, doffs, status: lib.omr_j2k_decode_batch_device(
            ctx.h, blob, offs, lens, ws, hs, n, int(samples), int(bits), out, doffs, status))


def jpeg_decode_batch_device(ctx, streams, sizes, samples=1, ycbcr=False, tables=None):
    """K17 alone (omr_jpeg_decode_batch_device): streams[i] with a frame of sizes[i] = (width,
    height), decoded on ctx's GPU.  Returns ([uint8 arrays, [h][w] or [h][w][3]], [status per stream])."""
    tab = np.frombuffer(bytes(tables or b""), dtype=np.uint8)
    return _decode_batch_device(
        ctx, streams, sizes, samples, 1, "u1",
        lambda blob, offs, lens, ws, hs, n, out, doffs, status: lib.omr_jpeg_decode_batch_device(
            ctx.h, tab.ctypes.data if tab.size else None, tab.size, blob, offs, lens, ws, hs, n, int(samples),
            int(bool(ycbcr)), out, doffs, status))
