"""PixelBuffer: the ROMIO repository pixel file the render path reads tiles from.

Mirrors upstream ome.io.nio.RomioPixelBuffer as used by
pixelsService.getPixelBuffer(pixels, false) (ImageRegionRequestHandler.java:302-309): one file of
big-endian planes in XYZCT order.  Reads go through libomr.so (pread; no numpy fallback).
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import lib

_BE_DTYPES = {_lib.PIXELS_INT8: ">i1", _lib.PIXELS_UINT8: ">u1", _lib.PIXELS_INT16: ">i2",
              _lib.PIXELS_UINT16: ">u2", _lib.PIXELS_INT32: ">i4", _lib.PIXELS_UINT32: ">u4",
              _lib.PIXELS_FLOAT: ">f4", _lib.PIXELS_DOUBLE: ">f8"}


def write_romio(path, pixels, pixel_type):
    """Write a [t][c][z][y][x] array as a ROMIO pixel file (big-endian, XYZCT plane order)."""
    a = np.ascontiguousarray(np.asarray(pixels).astype(_BE_DTYPES[pixel_type]))
    assert a.ndim == 5, "pixels must be [t][c][z][y][x]"
    a.tofile(path)


PYRAMID_MAGIC = b"OMRPYR1\0"
PYRAMID_HEADER_BYTES = 64
PYRAMID_LEVEL_ALIGN = 4096


def write_pyramid(path, levels, pixel_type, rule=_lib.PYRAMID_MEAN, size=None):
    """Write the pyramid sidecar of an image (layout: include/omr/omr.h).  levels[k-1] is level k
    as a [t][c][z][y][x] array, k = 1..n_levels-1; size = (size_x, size_y) of level 0 (default:
    taken from level 1 when there is one, which fits an even-sized image only, so pass it)."""
    levels = [np.ascontiguousarray(np.asarray(lv).astype(_BE_DTYPES[pixel_type])) for lv in levels]
    for lv in levels:
        assert lv.ndim == 5, "levels must be [t][c][z][y][x]"
    if size is None:
        size = (levels[0].shape[4] * 2, levels[0].shape[3] * 2)
    st, sc, sz = levels[0].shape[:3] if levels else (1, 1, 1)
    hdr = PYRAMID_MAGIC + np.array([1, rule, pixel_type, len(levels) + 1], "<u4").tobytes() + \
        np.array([size[0], size[1], sz, sc, st], "<i4").tobytes()
    with open(path, "wb") as f:
        f.write(hdr.ljust(PYRAMID_HEADER_BYTES, b"\0"))
        for lv in levels:
            f.write(b"\0" * (-f.tell() % PYRAMID_LEVEL_ALIGN))
            f.write(lv.tobytes())


class PixelBuffer:
    def __init__(self, path, size_x, size_y, size_z, size_c, size_t, pixel_type, _handle=None):
        h = ctypes.c_void_p()
        if _handle is not None:           # a level view (PixelBuffer.level)
            h = _handle
        else:
            st = lib.omr_pixel_buffer_open(str(path).encode(), size_x, size_y, size_z, size_c, size_t, pixel_type,
                                           ctypes.byref(h))
            if st != _lib.OK:
                raise _lib.OmrError(st, f"cannot open pixel buffer {path}")
        self.h = h
        self.size_x, self.size_y, self.size_z, self.size_c, self.size_t = size_x, size_y, size_z, size_c, size_t
        self.pixel_type = pixel_type

    def close(self):
        if self.h:
            lib.omr_pixel_buffer_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # PixelBuffer interface the handler uses (ImageRegionRequestHandler.java:446-454): a ROMIO
    # buffer has one resolution level until a pyramid sidecar is attached.
    big_endian = True

    def getResolutionLevels(self):
        return int(lib.omr_pixel_buffer_resolution_levels(self.h))

    def getResolutionDescriptions(self):
        out = (ctypes.c_int32 * (2 * _lib.PYRAMID_MAX_LEVELS))()
        n = lib.omr_pixel_buffer_resolution_descriptions(self.h, out, _lib.PYRAMID_MAX_LEVELS)
        if n < 1:
            raise _lib.OmrError(_lib.INVALID_ARGUMENT, "closed pixel buffer")
        return [[out[2 * k], out[2 * k + 1]] for k in range(n)]

    def build_pyramid(self, ctx, path, rule=_lib.PYRAMID_MEAN, n_levels=0):
        """Build this image's levels on ctx's GPU (K11) and write the sidecar file `path`
        (omr_pixel_buffer_build_pyramid; n_levels <= 0: down to a longest side of 256).  It does
        not attach the file."""
        _lib.check(lib.omr_pixel_buffer_build_pyramid(ctx.h, self.h, int(rule), int(n_levels), str(path).encode()),
                   ctx.h)

    def attach_pyramid(self, path):
        """Serve resolution levels from the sidecar file `path` (omr_pixel_buffer_attach_pyramid)."""
        st = lib.omr_pixel_buffer_attach_pyramid(self.h, str(path).encode())
        if st != _lib.OK:
            raise _lib.OmrError(st, f"cannot attach pyramid {path}")

    def level(self, resolution):
        """Resolution level `resolution` (0 = full size, the index into getResolutionDescriptions)
        as a PixelBuffer of its own; close it like any other, in any order with this one."""
        h = ctypes.c_void_p()
        st = lib.omr_pixel_buffer_level(self.h, int(resolution), ctypes.byref(h))
        if st != _lib.OK:
            raise _lib.OmrError(st, f"no resolution level {resolution}")
        return PixelBuffer(None, self.size_x >> resolution, self.size_y >> resolution, self.size_z, self.size_c,
                           self.size_t, self.pixel_type, _handle=h)

    def getTileSize(self):
        return (min(self.size_x, 256), min(self.size_y, 256))

    def stack_to_device(self, c, t, device):
        """The Z-stack of (c, t) — contiguous in XYZCT order — as a device byte tensor
        (ProjectionService.projectStack reads whole stacks, ProjectionService.java:46-120)."""
        import torch
        host = np.empty((self.size_z, self.size_y, self.size_x), dtype=_BE_DTYPES[self.pixel_type])
        for z in range(self.size_z):
            _lib.check(lib.omr_pixel_buffer_get_tile(self.h, z, c, t, 0, 0, self.size_x, self.size_y,
                                                     host[z].ctypes.data, host[z].nbytes))
        return torch.from_numpy(host.view(np.uint8).reshape(-1)).to(device)

    def histogram(self, ctx, z, c, t, bins=256, range_mode=_lib.HIST_RANGE_TYPE, lo=None, hi=None, region=None):
        """Histogram of plane (z, c, t), or of its region (x, y, w, h), on ctx's GPU
        (omr_pixel_buffer_histogram): (counts[bins] uint32, info, stats) with info = {lo, hi, below,
        above, nan_count} and stats = {min, max, count, nan_count} of the region."""
        from .context import _info_dict, _region
        counts = np.zeros(max(int(bins), 0), dtype=np.uint32)
        info, stats = _lib.HistogramInfo(), _lib.PlaneStats()
        _lib.check(lib.omr_pixel_buffer_histogram(ctx.h, self.h, z, c, t, _region(region), int(range_mode),
                                                  float(lo or 0.0), float(hi or 0.0), int(bins), counts.ctypes.data,
                                                  ctypes.byref(info), ctypes.byref(stats)), ctx.h)
        return counts, _info_dict(info), {"min": stats.min, "max": stats.max, "count": int(stats.count),
                                          "nan_count": int(stats.nan_count)}

    def tiles_png(self, ctx, reqs, w, h, cap=None):
        """Raw tiles as greyscale PNG files (omr_pixel_buffer_tiles_png): reqs = [(z, c, t, x, y)],
        every tile w x h; returns the files as a list of bytes.  When a tile failed (one outside
        the image: INVALID_ARGUMENT) it raises OmrError with .statuses (per tile) and .files (the
        other tiles' bytes, b"" for the failed ones)."""
        n = len(reqs)
        tab = (_lib.RawTileRequest * max(n, 1))()
        for i, r in enumerate(reqs):
            tab[i].z, tab[i].c, tab[i].t, tab[i].x, tab[i].y = [int(v) for v in r]
        if cap is None:
            cap = n * lib.omr_png_gray_batch_max_bytes(max(1, int(w)), max(1, int(h)),
                                                       min(_lib.BYTES_PER_PIXEL[self.pixel_type], 2), 1)
        out = np.empty(max(cap, 1), dtype=np.uint8)
        offs = np.zeros(max(n, 1), np.uint64)
        lens = np.zeros(max(n, 1), np.uint32)
        stat = np.zeros(max(n, 1), np.int32)
        _lib.check(lib.omr_pixel_buffer_tiles_png(ctx.h, self.h, ctypes.addressof(tab), n, int(w), int(h),
                                                  out.ctypes.data, cap, offs.ctypes.data, lens.ctypes.data,
                                                  stat.ctypes.data), ctx.h)
        files = [out[int(offs[i]):int(offs[i]) + int(lens[i])].tobytes() if stat[i] == 0 else b"" for i in range(n)]
        if n and stat[:n].any():
            bad = [i for i in range(n) if stat[i]]
            err = _lib.OmrError(int(stat[bad[0]]), f"raw tiles {bad} failed")
            err.statuses, err.files = [int(s) for s in stat[:n]], files
            raise err
        return files

    def tile_tiff(self, z, c, t, x, y, w, h):
        """The raw tile as a baseline big-endian TIFF in the buffer's pixel type
        (omr_pixel_buffer_tile_tiff)."""
        cap = lib.omr_tiff_raw_max_bytes(int(w), int(h), self.pixel_type)
        out = np.empty(max(cap, 1), dtype=np.uint8)
        n = ctypes.c_size_t(0)
        _lib.check(lib.omr_pixel_buffer_tile_tiff(self.h, z, c, t, x, y, int(w), int(h), out.ctypes.data, cap,
                                                  ctypes.byref(n)))
        return out[:n.value].tobytes()

    def plane_offset(self, z, c, t):
        return lib.omr_pixel_buffer_plane_offset(self.h, z, c, t)

    def get_tile(self, z, c, t, x, y, w, h):
        """PixelBuffer.getTile: [h][w] array in file (big-endian) byte order."""
        if w < 0 or h < 0:   # DimensionsOutOfBoundsException, as the C bounds check
            raise _lib.OmrError(_lib.INVALID_ARGUMENT, f"tile {w}x{h} out of bounds")
        out = np.empty((h, w), dtype=_BE_DTYPES[self.pixel_type])
        _lib.check(lib.omr_pixel_buffer_get_tile(self.h, z, c, t, x, y, w, h, out.ctypes.data, out.nbytes))
        return out
