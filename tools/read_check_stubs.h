// read_check_stubs.h — what the readers' host halves (omr_tiffread.cpp, omr_zarr.cpp) take from the
// rest of the library, for the stand-alone sanitizer programs that link them without it
// (tiff_read_check, zarr_read_check, blosc_read_check, zstd_read_check): the sample width, the
// error message sink and the two entry points of the device route (omr_segread.cpp), which is not
// run there.  Include it in exactly one translation unit of a program.
#pragma once

#include "omr_segread.h"

namespace omr {
int bytes_per_pixel(int32_t t) {
    switch (t) {
    case OMR_PIXELS_INT8: case OMR_PIXELS_UINT8: return 1;
    case OMR_PIXELS_INT16: case OMR_PIXELS_UINT16: return 2;
    case OMR_PIXELS_INT32: case OMR_PIXELS_UINT32: case OMR_PIXELS_FLOAT: return 4;
    case OMR_PIXELS_DOUBLE: return 8;
    default: return 0;
    }
}
omr_status fail(Ctx*, omr_status s, const std::string&) { return s; }
omr_status read_regions_checked(Ctx*, SegSource&, const SegImageDims&, const omr_raw_tile_request*, int32_t, int32_t, int32_t,
                                void*, int64_t) {
    return OMR_DEVICE;
}
omr_status render_tiles_checked(omr_ctx*, SegSource&, const SegImageDims&, const omr_quantum_def*, const omr_channel_binding*,
                                int32_t, const omr_tile_request*, int32_t, int32_t, int32_t, int32_t, int32_t, uint32_t*, int32_t) {
    return OMR_DEVICE;
}
}  // namespace omr
