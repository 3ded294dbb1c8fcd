"""The public surface of omr.tiffimage, omr.zarrimage and the package: the names, and the public
methods of the two image classes with their order and parameter names.  The lists were taken with
`inspect` from the tree before TiffImage and ZarrImage got their common base (omr._segimage); a
refactoring of the wrappers must leave them as they are."""
import inspect
import types

import omr
from omr import tiffimage, zarrimage

ALL = ["_lib", "OmrError", "Context", "Renderer", "histogram_bin_of", "histogram_json", "encode_tiff_raw", "thumbnail_size",
       "ChannelSettings", "ReverseIntensityContext", "create_rendering_def", "flip", "split_html_color", "ImageRegionCtx",
       "ImageRegionRequestHandler", "InMemoryPixelBuffer", "LutProvider", "RequestError", "ShapeMaskCtx",
       "ShapeMaskRequestHandler", "PixelBuffer", "write_romio", "write_pyramid", "Batcher", "Pool", "TiffImage",
       "write_tiled_tiff", "lzw_encode", "lzw_decode_host", "jpeg_decode_host", "jpeg_stream_forms",
       "jpeg_decode_batch_device", "jpeg_decode_host_split", "j2k_decode_host", "j2k_stream_forms", "j2k_decode_batch_device",
       "ZarrImage", "write_zarr", "inflate_host", "lz4_encode", "lz4_decode_host", "blosc_encode", "blosc_decode_host",
       "zstd_encode", "zstd_decode_host", "zstd_frame_forms"]

# the public names that are not imported modules
TIFFIMAGE = ["DIMENSION_ORDERS", "TiffImage", "j2k_decode_batch_device", "j2k_decode_host", "j2k_stream_forms",
             "jpeg_decode_batch_device", "jpeg_decode_host", "jpeg_decode_host_split", "jpeg_stream_forms", "lib",
             "lzw_decode_host", "lzw_encode", "write_tiled_tiff"]
ZARRIMAGE = ["ZSTD_BLOCK_MAX", "ZarrImage", "blosc_decode_host", "blosc_encode", "inflate_host", "lib", "lz4_decode_host",
             "lz4_encode", "write_zarr", "xxh64", "zstd_block", "zstd_decode_host", "zstd_encode", "zstd_frame_forms",
             "zstd_frame_header", "zstd_sequences_block"]

SHARED_METHODS = [
    ("close", ["self"]),
    ("__del__", ["self"]),
    ("__enter__", ["self"]),
    ("__exit__", ["self", "exc"]),
    ("getResolutionLevels", ["self"]),
    ("getResolutionDescriptions", ["self"]),
    ("get_tile", ["self", "level", "z", "c", "t", "x", "y", "w", "h"]),
    ("read_regions", ["self", "ctx", "level", "reqs", "w", "h", "out", "region_stride"]),
    ("render_tiles", ["self", "ctx", "qdef", "channels", "level", "requests", "width", "height", "out", "flip_h", "flip_v",
                      "bindings"]),
]
TIFF_METHODS = [("__init__", ["self", "path", "size_z", "size_c", "size_t", "dimension_order", "accept"])] + SHARED_METHODS
ZARR_METHODS = [("__init__", ["self", "path", "codecs"])] + SHARED_METHODS

FUNCTIONS = {
    tiffimage: {
        "lzw_decode_host": ["stream", "expected"],
        "jpeg_decode_host": ["stream", "width", "height", "samples", "ycbcr", "tables"],
        "jpeg_decode_host_split": ["stream", "width", "height", "samples", "ycbcr", "tables", "subsequence_bits", "lanes"],
        "jpeg_stream_forms": ["stream", "tables"],
        "j2k_decode_host": ["stream", "width", "height", "samples", "bits"],
        "j2k_stream_forms": ["stream"],
        "j2k_decode_batch_device": ["ctx", "streams", "sizes", "samples", "bits"],
        "jpeg_decode_batch_device": ["ctx", "streams", "sizes", "samples", "ycbcr", "tables"],
    },
    zarrimage: {
        "inflate_host": ["stream", "expected"],
        "lz4_decode_host": ["stream", "expected"],
        "blosc_decode_host": ["chunk", "expected", "inner"],
        "zstd_decode_host": ["frame", "expected"],
        "zstd_frame_forms": ["frame"],
    },
}


def _public(module):
    return sorted(n for n, v in vars(module).items() if not n.startswith("_") and not isinstance(v, types.ModuleType))


def _methods(cls):
    """(name, parameter names) of the public and the four special methods, in definition order: the
    class's own first, then those of its bases."""
    keep = ("__init__", "__del__", "__enter__", "__exit__")
    seen, out = set(), []
    for klass in cls.__mro__[:-1]:
        for name, v in vars(klass).items():
            if callable(v) and (not name.startswith("_") or name in keep) and name not in seen:
                seen.add(name)
                out.append((name, list(inspect.signature(getattr(cls, name)).parameters)))
    return out


def test_package_exports():
    assert list(omr.__all__) == ALL
    for name in ALL:
        assert hasattr(omr, name), name


def test_module_names():
    assert _public(tiffimage) == TIFFIMAGE
    assert _public(zarrimage) == ZARRIMAGE
    assert tiffimage.TiffImage.__module__ == "omr.tiffimage" and zarrimage.ZarrImage.__module__ == "omr.zarrimage"
    assert omr.TiffImage is tiffimage.TiffImage and omr.ZarrImage is zarrimage.ZarrImage


def test_image_class_methods():
    assert _methods(tiffimage.TiffImage) == TIFF_METHODS
    assert _methods(zarrimage.ZarrImage) == ZARR_METHODS
    for cls in (tiffimage.TiffImage, zarrimage.ZarrImage):
        assert cls.__doc__ and cls.__init__.__doc__
        for name, _ in SHARED_METHODS[6:]:
            assert getattr(cls, name).__doc__, name


def test_function_parameters():
    for module, functions in FUNCTIONS.items():
        for name, params in functions.items():
            assert list(inspect.signature(getattr(module, name)).parameters) == params, name
