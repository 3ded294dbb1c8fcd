"""The files of the TIFF codec tests (test_tiff_codecs_host.py, test_tiff_codecs_gpu.py): the forms
omr_tiff_image_open_ex adds to the reader -- Deflate and zstd segments, the floating-point
predictor, chunky pixels of several samples -- written by omr.write_tiled_tiff (libtiff through
Pillow writes only little-endian strips of 8-bit RGB and of 8-, 16- and 32-bit grey: those are the
golden files of tests/golden/tiff_codecs.npz, made by tools/make_tiff_codec_golden.py with the
pixel functions below).

Every file is 150 x 70 with one SubIFD level of 75 x 35.  Tiles are (80, 16): a row of a tile is 64
+ 16 columns, so the predictor's carry crosses a 64-column step, and the right and bottom tiles
hang over the edge; strips have 16 rows, the last one 6."""
import os
import zlib

import numpy as np

import omr

W, H, LW, LH = 150, 70, 75, 35
ACCEPT_ALL = ("deflate", "zstd", "predictor3", "samples")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiff_codecs.npz")
NAMES = ("int8", "uint8", "int16", "uint16", "int32", "uint32", "float32", "float64")


def pixels(name, channels, w, h, seed, smooth=True, amp=23):
    """[1][channels][1][h][w]: a ramp with noise of `amp` levels on it (matches and literals for the
    coders), the integers reaching into the type's high bytes; smooth=False: noise alone."""
    rng = np.random.default_rng(seed)
    shape = (1, channels, 1, h, w)
    dt = np.dtype(name)
    if dt.kind == "f":
        a = np.round(rng.standard_normal(shape) * amp) / 16 + (np.arange(w) // 5 if smooth else 0)
        return a.astype(dt)
    bits = 8 * dt.itemsize
    a = rng.integers(0, amp if smooth else 1 << min(bits, 31), shape)
    if smooth:
        a = a + (np.arange(w) * 3)[None, None, None, None, :] + (np.arange(h) * 5)[None, None, None, :, None]
        a = a * (1 + (1 << (bits - 8)) // 61)                # up into the high bytes
    return (a % (1 << bits)).astype("u%d" % dt.itemsize).view(dt)


class Case:
    """One written file: its name, the writer's arguments and what the reader must be told."""

    def __init__(self, name, dtype, compression, predictor=1, spp=1, bo="<", bigtiff=False, strips=False,
                 zero_rows=False):
        self.name, self.dtype, self.compression, self.predictor, self.spp = name, dtype, compression, predictor, spp
        self.bo, self.bigtiff, self.strips, self.zero_rows = bo, bigtiff, strips, zero_rows
        self.size_c = 2 * spp if spp > 1 else 2              # two IFDs per level
        need = set()
        if compression in (8, 32946):
            need.add("deflate")
        if compression == 50000:
            need.add("zstd")
        if predictor == 3:
            need.add("predictor3")
        if spp > 1:
            need.add("samples")
        self.need = tuple(sorted(need))

    def __repr__(self):
        return self.name

    def planes(self):
        seed = zlib.crc32(self.name.encode())
        lv0 = pixels(self.dtype, self.size_c, W, H, seed)
        lv1 = pixels(self.dtype, self.size_c, LW, LH, seed + 1)
        if self.zero_rows:                                   # segment row 2 of level 0 (rows 32..47): byte count 0
            lv0[:, :, :, 32:48, :] = 0
        return lv0, lv1

    def write(self, path):
        """Writes the file; returns (level 0, level 1) as [1][c][1][h][w] and the writer's result."""
        lv0, lv1 = self.planes()
        kw = {"rows_per_strip": 16} if self.strips else {"tile": (80, 16)}
        res = omr.write_tiled_tiff(path, lv0, levels=[lv1], byteorder=self.bo, bigtiff=self.bigtiff,
                                   compression=self.compression, predictor=self.predictor,
                                   samples_per_pixel=self.spp, skip_zero_segments=self.zero_rows, **kw)
        return lv0, lv1, res

    def open(self, path, accept=None):
        return omr.TiffImage(path, 1, self.size_c, 1, accept=self.need if accept is None else accept)


def _cases():
    out = []
    k = 0
    # each of the eight pixel types with Deflate and with zstd; layout, byte order, container and
    # (where the type has one) Predictor 2 go round
    for dtype in NAMES:
        for comp, word in ((8, "deflate"), (50000, "zstd")):
            pred = 2 if (k % 3 != 0 and dtype != "float64") else 1
            bo = "<>"[(k // 2) % 2] if comp == 8 else "><"[(k // 2) % 2]
            strips, big = bool(k % 2), bool((k // 3) % 2)
            out.append(Case(f"{dtype}-{word}-p{pred}-{'be' if bo == '>' else 'le'}-{'strips' if strips else 'tiles'}"
                            f"{'-big' if big else ''}", dtype, comp, pred, 1, bo, big, strips))
            k += 1
    # the floating-point predictor: both types, both byte orders, compressed and stored
    for dtype in ("float32", "float64"):
        for bo in "<>":
            for comp, word in ((8, "deflate"), (1, "stored"), (50000, "zstd")):
                if comp == 50000 and bo == ">":
                    continue
                strips = comp == 1 and bo == ">"
                out.append(Case(f"{dtype}-{word}-p3-{'be' if bo == '>' else 'le'}-{'strips' if strips else 'tiles'}",
                                dtype, comp, 3, 1, bo, dtype == "float64" and comp == 8, strips))
    # chunky pixels: 3 and 4 samples of 8 and 16 bits, Predictor 1 and 2, both byte orders (the
    # swapped strided scan); the codecs go round, LZW and stored segments among them
    comps = ((8, "deflate"), (50000, "zstd"), (5, "lzw"), (1, "stored"))
    j = 0                                                    # counts (spp, type)
    for spp in (3, 4):
        for dtype in ("uint8", "uint16"):
            for pred in (1, 2):
                for b, bo in enumerate("<>"):
                    comp, word = comps[(j + 2 * b) % 4] if pred == 1 else comps[(j + b) % 2]
                    strips = bool((j + b + pred) % 2)
                    out.append(Case(f"{dtype}x{spp}-{word}-p{pred}-{'be' if bo == '>' else 'le'}-"
                                    f"{'strips' if strips else 'tiles'}", dtype, comp, pred, spp, bo, (j + pred) % 3 == 0, strips))
            j += 1
    out.append(Case("uint16x3-lzw-p2-be-tiles", "uint16", 5, 2, 3, ">"))
    out.append(Case("uint8x4-stored-p2-le-strips", "uint8", 1, 2, 4, "<", False, True))
    # a segment row with byte count 0, grey and RGB; Compression 32946
    out.append(Case("uint16-deflate-p2-zero-tiles", "uint16", 8, 2, 1, "<", False, False, zero_rows=True))
    out.append(Case("uint8x3-zstd-p2-zero-strips", "uint8", 50000, 2, 3, "<", False, True, zero_rows=True))
    out.append(Case("uint16-32946-p2-le-tiles", "uint16", 32946, 2, 1, "<"))
    return out


CASES = _cases()
CASE_BY_NAME = {c.name: c for c in CASES}


class Files:
    """The written files of a test module, each made once (a module-scoped fixture keeps one)."""

    def __init__(self, directory):
        self.dir = directory
        self.made = {}

    def get(self, case):
        if case.name not in self.made:
            path = os.path.join(str(self.dir), case.name + ".tif")
            lv0, lv1, res = case.write(path)
            self.made[case.name] = (path, lv0, lv1, res)
        return self.made[case.name]


# ---- the golden files (libtiff through Pillow) ------------------------------------------------------

# name -> (dtype, samples, Pillow compression, Predictor, smooth): 150 x 70, RowsPerStrip 32
GOLDEN_FILES = {
    "uint8-deflate-p1": ("uint8", 1, "tiff_adobe_deflate", 1, False),
    "uint8-deflate-p2": ("uint8", 1, "tiff_adobe_deflate", 2, True),
    "uint16-deflate-p1": ("uint16", 1, "tiff_adobe_deflate", 1, True),
    "uint16-deflate-p2": ("uint16", 1, "tiff_adobe_deflate", 2, True),
    "uint8-zstd-p1": ("uint8", 1, "zstd", 1, True),
    "uint8-zstd-p2": ("uint8", 1, "zstd", 2, True),
    "uint16-zstd-p1": ("uint16", 1, "zstd", 1, True),
    "uint16-zstd-p2": ("uint16", 1, "zstd", 2, True),
    "float32-deflate-p3": ("float32", 1, "tiff_adobe_deflate", 3, True),
    "uint8x3-deflate-p1": ("uint8", 3, "tiff_adobe_deflate", 1, True),
    "uint8x3-deflate-p2": ("uint8", 3, "tiff_adobe_deflate", 2, True),
}


def golden_pixels(name):
    """[samples][70][150] of a golden file."""
    dtype, spp, _, _, smooth = GOLDEN_FILES[name]
    return pixels(dtype, spp, W, H, zlib.crc32(("golden " + name).encode()), smooth, amp=3)[0, :, 0]


def golden_need(name):
    dtype, spp, comp, pred, _ = GOLDEN_FILES[name]
    need = {"zstd" if comp == "zstd" else "deflate"}
    if pred == 3:
        need.add("predictor3")
    if spp > 1:
        need.add("samples")
    return tuple(sorted(need))


def load_golden(directory):
    """The golden files written out under `directory`: {name: (path, pixels [samples][70][150])}; the
    pixels stored in the fixture must be the ones golden_pixels makes."""
    z = np.load(GOLDEN)
    out = {}
    for name in GOLDEN_FILES:
        path = os.path.join(str(directory), "golden-" + name + ".tif")
        with open(path, "wb") as f:
            f.write(z["file/" + name].tobytes())
        px = z["pixels/" + name]
        assert px.tobytes() == golden_pixels(name).tobytes() and px.dtype == golden_pixels(name).dtype, name
        out[name] = (path, px)
    return out


# ---- finding a segment in a classic little-endian file ------------------------------------------------

def segment_table(raw, ifd):
    """(position of the offsets array, position of the counts array, count) of the IFD at `ifd` of a
    classic little-endian TIFF with more than one segment."""
    import struct
    n = struct.unpack_from("<H", raw, ifd)[0]
    where = {}
    for k in range(n):
        tag, typ, count, value = struct.unpack_from("<HHII", raw, ifd + 2 + 12 * k)
        where[tag] = (typ, count, value)
    offs = where.get(324) or where[273]
    cnts = where.get(325) or where[279]
    assert offs[0] == 4 and cnts[0] == 4 and offs[1] == cnts[1] > 1
    return offs[2], cnts[2], offs[1]


# ---- inputs of the sanitizer check (tools/tiff_read_check.cpp, `make tiff-read-check`) ------------------

def dump(directory):
    """Good files of every new form for tiff_read_check: <name>.tif, <name>.px (level 0 as
    [channel][y][x] in the file's byte order) and manifest.txt with a line `name size_c accept
    bytes-per-sample` per file.  The golden files of libtiff and one written file per form."""
    os.makedirs(directory, exist_ok=True)
    bits = {"deflate": 1, "zstd": 2, "predictor3": 4, "samples": 8}
    lines = []

    def keep(name, path, size_c, need, px):
        with open(path, "rb") as f, open(os.path.join(directory, name + ".tif"), "wb") as g:
            g.write(f.read())
        with open(os.path.join(directory, name + ".px"), "wb") as g:
            g.write(np.ascontiguousarray(px).tobytes())
        lines.append("%s %d %d %d" % (name, size_c, sum(bits[n] for n in need), px.dtype.itemsize))

    for name, (path, px) in load_golden(directory).items():
        keep("golden-" + name + "-kept", path, px.shape[0], golden_need(name), px)
        os.remove(path)
    picks = [lambda c: c.compression == 8 and c.spp == 1 and c.predictor == 2 and c.strips,
             lambda c: c.compression == 50000 and c.spp == 1 and c.predictor == 2 and not c.strips,
             lambda c: c.predictor == 3 and c.dtype == "float32" and c.bo == "<" and c.compression == 8,
             lambda c: c.predictor == 3 and c.dtype == "float64" and c.bo == ">" and c.compression == 1,
             lambda c: c.predictor == 3 and c.compression == 50000,
             lambda c: c.spp == 3 and c.predictor == 2 and c.compression == 8,
             lambda c: c.spp == 4 and c.dtype == "uint16" and c.predictor == 2 and c.bo == ">",
             lambda c: c.spp == 3 and c.compression == 5,
             lambda c: c.zero_rows and c.spp == 3,
             lambda c: c.bigtiff and c.compression == 50000]
    files = Files(directory)
    done = set()
    for pick in picks:
        case = next((c for c in CASES if pick(c)), None)
        if case is None or case.name in done:
            continue
        done.add(case.name)
        path, lv0, _, _ = files.get(case)
        fdt = lv0.dtype.newbyteorder(case.bo) if lv0.dtype.itemsize > 1 else lv0.dtype
        keep("case-" + case.name, path, case.size_c, case.need, lv0[0, :, 0].astype(fdt))
        os.remove(path)
    with open(os.path.join(directory, "manifest.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    return lines
