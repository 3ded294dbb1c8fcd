"""omr — MI355X-native image-region rendering (Python side of the drop-in).

Layers:
  _lib      ctypes binding of libomr.so (the C ABI in include/omr/omr.h)
  context   Context: one per worker thread / GPU (device, stream, workspace)
  renderer  Renderer facade mirroring the omeis Renderer calls the reference makes
            (ImageRegionRequestHandler.java:436-440, :689-741, :559)
  pixbuf    PixelBuffer: ROMIO repository pixel files (getPixelBuffer, :302-309)
  tiffimage TiffImage: tiled TIFF / OME-TIFF pixel files, LZW, Deflate, zstd, JPEG and JPEG 2000 decoded on the GPU; write_tiled_tiff
  j2k       JPEG 2000 codestreams alone, irreversible (9/7) ones included: decode_host, decode_batch_device, stream_forms
  zarrimage ZarrImage: OME-Zarr pyramids, zlib, Blosc (LZ4 or Zstd inside) and zstd chunks decoded on the GPU; write_zarr
  batcher   Batcher: concurrent requests coalesced into GPU batches; Pool: one batcher per GPU
  request   ImageRegionCtx / ShapeMaskCtx parsing and the handler glue
            (ImageRegionCtx.java, ImageRegionRequestHandler.java, ShapeMaskRequestHandler.java)
"""
from . import _lib
from . import j2k
from ._lib import OmrError
from .context import Context, pyramid_level_count, pyramid_level_sizes, thumbnail_size
from .pixbuf import PixelBuffer, write_pyramid, write_romio
from .tiffimage import (TiffImage, j2k_decode_batch_device, j2k_decode_host, j2k_stream_forms, jpeg_decode_batch_device,
                        jpeg_decode_host, jpeg_decode_host_split, jpeg_stream_forms, lzw_decode_host, lzw_encode,
                        write_tiled_tiff)
from .zarrimage import (ZarrImage, blosc_decode_host, blosc_encode, inflate_host, lz4_decode_host, lz4_encode,
                        write_zarr, zstd_decode_host, zstd_encode, zstd_frame_forms)
from .batcher import Batcher, Pool
from .renderer import (ChannelSettings, Renderer, ReverseIntensityContext, create_rendering_def,
                       flip, split_html_color)
from .request import (ImageRegionCtx, ImageRegionRequestHandler, InMemoryPixelBuffer, LutProvider,
                      RequestError, ShapeMaskCtx, ShapeMaskRequestHandler)



def histogram_bin_of(v, lo, hi, bins):
    """The binning rule on the host (omr_histogram_bin_of): bin index, or -1 below the range, -2
    above it, -3 for NaN."""
    return int(_lib.lib.omr_histogram_bin_of(float(v), float(lo), float(hi), int(bins)))


_NP_PIXEL_TYPES = {"int8": _lib.PIXELS_INT8, "uint8": _lib.PIXELS_UINT8, "int16": _lib.PIXELS_INT16,
                   "uint16": _lib.PIXELS_UINT16, "int32": _lib.PIXELS_INT32, "uint32": _lib.PIXELS_UINT32,
                   "float32": _lib.PIXELS_FLOAT, "float64": _lib.PIXELS_DOUBLE}


def encode_tiff_raw(array):
    """A [h][w] numpy array of one of the eight pixel types, in either byte order, as a baseline
    big-endian one-sample TIFF in that type (omr_encode_tiff_raw; host writer, no GPU)."""
    import ctypes
    import numpy as np
    a = np.ascontiguousarray(array)
    if a.ndim != 2 or a.dtype.name not in _NP_PIXEL_TYPES:
        raise OmrError(_lib.INVALID_ARGUMENT, f"not a [h][w] array of a pixel type: {a.dtype} {a.shape}")
    pt = _NP_PIXEL_TYPES[a.dtype.name]
    big = a.dtype.byteorder == ">" or (a.dtype.byteorder == "=" and not np.little_endian) or a.dtype.itemsize == 1
    h, w = a.shape
    cap = _lib.lib.omr_tiff_raw_max_bytes(w, h, pt)
    out = np.empty(max(cap, 1), dtype=np.uint8)
    n = ctypes.c_size_t(0)
    _lib.check(_lib.lib.omr_encode_tiff_raw(a.ctypes.data if a.size else None, pt, int(big), w, h,
                                            out.ctypes.data, cap, ctypes.byref(n)))
    return out[:n.value].tobytes()


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


__all__ = ["_lib", "OmrError", "Context", "Renderer", "histogram_bin_of", "histogram_json", "encode_tiff_raw", "thumbnail_size", "ChannelSettings", "ReverseIntensityContext",
           "create_rendering_def", "flip", "split_html_color", "ImageRegionCtx",
           "ImageRegionRequestHandler", "InMemoryPixelBuffer", "LutProvider", "RequestError",
           "ShapeMaskCtx", "ShapeMaskRequestHandler", "PixelBuffer", "write_romio", "write_pyramid", "Batcher", "Pool",
           "TiffImage", "write_tiled_tiff", "lzw_encode", "lzw_decode_host", "jpeg_decode_host", "jpeg_stream_forms",
           "jpeg_decode_batch_device", "jpeg_decode_host_split", "j2k_decode_host", "j2k_stream_forms",
           "j2k_decode_batch_device",
           "ZarrImage", "write_zarr", "inflate_host", "lz4_encode", "lz4_decode_host", "blosc_encode",
           "blosc_decode_host", "zstd_encode", "zstd_decode_host", "zstd_frame_forms"]
