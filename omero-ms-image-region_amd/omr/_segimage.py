"""What TiffImage and ZarrImage share: an open image handle of libomr.so whose levels are read by
the shared device-read pipeline (omr_segread.cpp).  A subclass opens the image in its __init__
(self.h, self.dtype, self.pixel_type, self.level_sizes) and names its five entry points of `lib`.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import lib


class _SegImage:
    _CLOSE = _GET_TILE = _READ_REGIONS = _RENDER_TILES = None    # names of the subclass's lib functions

    def close(self):
        if self.h:
            getattr(lib, self._CLOSE)(self.h)
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

    def getResolutionLevels(self):
        return len(self.level_sizes)

    def getResolutionDescriptions(self):
        return [list(s) for s in self.level_sizes]

    def get_tile(self, level, z, c, t, x, y, w, h):
        """The host route: [h][w] array in the image's byte order (omr_tiff_image_get_tile,
        omr_zarr_image_get_tile)."""
        if w < 0 or h < 0:
            raise _lib.OmrError(_lib.INVALID_ARGUMENT, f"tile {w}x{h} out of bounds")
        out = np.empty((h, w), dtype=self.dtype)
        _lib.check(getattr(lib, self._GET_TILE)(self.h, int(level), z, c, t, x, y, w, h, out.ctypes.data,
                                                max(out.nbytes, 1)))
        return out

    def read_regions(self, ctx, level, reqs, w, h, out=None, region_stride=None):
        """reqs = [(z, c, t, x, y)], every region w x h of `level`, read and decoded on ctx's GPU
        (omr_tiff_image_read_regions_device, omr_zarr_image_read_regions_device).  Returns a device
        uint8 tensor [n][region_stride] (allocated when out is None; region_stride defaults to the
        region's bytes rounded up to 16): region i is its first w*h*bytes_per_pixel bytes, rows
        packed, the image's byte order."""
        import torch
        n = len(reqs)
        bpp = _lib.BYTES_PER_PIXEL[self.pixel_type]
        if region_stride is None:
            region_stride = (w * h * bpp + 15) // 16 * 16
        if out is None:
            out = torch.zeros((max(n, 1), max(region_stride, 1)), dtype=torch.uint8, device=f"cuda:{ctx.device}")
            ctx.order_after_torch()
        tab = (_lib.RawTileRequest * max(n, 1))()
        for i, r in enumerate(reqs):
            tab[i].z, tab[i].c, tab[i].t, tab[i].x, tab[i].y = [int(v) for v in r]
        _lib.check(getattr(lib, self._READ_REGIONS)(ctx.h, self.h, int(level), ctypes.addressof(tab), n, int(w), int(h),
                                                    out.data_ptr(), int(region_stride)), ctx.h)
        return out[:n]

    def render_tiles(self, ctx, qdef, channels, level, requests, width, height, out=None, flip_h=False,
                     flip_v=False, bindings=None):
        """Context.render_pixel_buffer_tiles for this image's `level` (omr_render_tiff_tiles,
        omr_render_zarr_tiles): requests = [(z, t, x, y)]; out: host numpy [n][h][w] uint32
        (allocated when None) or a device tensor (rendered in place)."""
        from .context import _ptr, make_bindings
        arr, keep = make_bindings(channels) if bindings is None else bindings
        n = len(requests)
        reqs = (_lib.TileRequest * max(n, 1))(*[_lib.TileRequest(*r) for r in requests])
        on_device = out is not None and hasattr(out, "data_ptr")
        if out is None:
            out = np.empty((n, height, width), dtype=np.uint32)
        _lib.check(getattr(lib, self._RENDER_TILES)(ctx.h, self.h, int(level), ctypes.byref(qdef), arr, len(channels), reqs,
                                                    n, int(width), int(height), int(flip_h), int(flip_v), _ptr(out),
                                                    int(on_device)), ctx.h)
        return out
