"""omr — MI355X-native image-region rendering (Python side of the drop-in).

Layers:
  _lib      ctypes binding of libomr.so (the C ABI in include/omr/omr.h)
  context   Context: one per worker thread / GPU (device, stream, workspace)
  renderer  Renderer facade mirroring the omeis Renderer calls the reference makes
            (ImageRegionRequestHandler.java:436-440, :689-741, :559)
  pixbuf    PixelBuffer: ROMIO repository pixel files (getPixelBuffer, :302-309)
  batcher   Batcher: concurrent requests coalesced into GPU batches; Pool: one batcher per GPU
  request   ImageRegionCtx / ShapeMaskCtx parsing and the handler glue
            (ImageRegionCtx.java, ImageRegionRequestHandler.java, ShapeMaskRequestHandler.java)
"""
from . import _lib
from ._lib import OmrError
from .context import Context, pyramid_level_count, pyramid_level_sizes, thumbnail_size
from .pixbuf import PixelBuffer, write_pyramid, write_romio
from .batcher import Batcher, Pool
from .renderer import (ChannelSettings, Renderer, ReverseIntensityContext, create_rendering_def,
                       flip, split_html_color)
from .request import (ImageRegionCtx, ImageRegionRequestHandler, InMemoryPixelBuffer, LutProvider,
                      RequestError, ShapeMaskCtx, ShapeMaskRequestHandler)



def histogram_bin_of(v, lo, hi, bins):
    """The binning rule on the host (omr_histogram_bin_of): bin index, or -1 below the range, -2
    above it, -3 for NaN."""
    return int(_lib.lib.omr_histogram_bin_of(float(v), float(lo), float(hi), int(bins)))


def histogram_json(ctx, pixbuf, z, c, t, bins=256, use_pixels_type_range=True, lo=None, hi=None, region=None):
    """The body of webgateway/histogram_json for plane (z, c, t) of a pixel buffer, as plain Python
    numbers.  Range: an explicit (lo, hi) when both are given, else the pixel-type range
    (usePixelsTypeRange=true) or the plane's own minimum and maximum."""
    if lo is not None and hi is not None:
        mode = _lib.HIST_RANGE_EXPLICIT
    else:
        mode = _lib.HIST_RANGE_TYPE if use_pixels_type_range else _lib.HIST_RANGE_PLANE
    counts, info, _ = pixbuf.histogram(ctx, z, c, t, bins=bins, range_mode=mode, lo=lo, hi=hi, region=region)
    return {"min": float(info["lo"]), "max": float(info["hi"]), "binCount": int(bins),
            "data": [int(v) for v in counts], "leftOutsideCount": int(info["below"]),
            "rightOutsideCount": int(info["above"])}


__all__ = ["_lib", "OmrError", "Context", "Renderer", "histogram_bin_of", "histogram_json", "thumbnail_size", "ChannelSettings", "ReverseIntensityContext",
           "create_rendering_def", "flip", "split_html_color", "ImageRegionCtx",
           "ImageRegionRequestHandler", "InMemoryPixelBuffer", "LutProvider", "RequestError",
           "ShapeMaskCtx", "ShapeMaskRequestHandler", "PixelBuffer", "write_romio", "write_pyramid", "Batcher", "Pool"]
