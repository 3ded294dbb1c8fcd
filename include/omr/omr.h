/*
 * omr.h — C ABI of the MI355X-native image-region rendering path.
 *
 * This is the drop-in boundary between the reference's Java host code
 * (omero-ms-image-region's ImageRegionRequestHandler / ShapeMaskRequestHandler)
 * and hand-written gfx950 HIP kernels.  Every entry point names the reference
 * call site it replaces.  Paths are relative to
 *   src/main/java/com/glencoesoftware/omero/ms/image/region/
 * of the reference.  Plain pointers and sizes only; no torch or HIP types.
 *
 * Status codes map onto the reference's HTTP outcomes
 * (ImageRegionVerticle.java:163-186, ImageRegionMicroserviceVerticle.java:301-304):
 *   OMR_INVALID_ARGUMENT -> 400 (IllegalArgumentException / ValidationException)
 *   OMR_NOT_FOUND        -> 404 (handler returned null, e.g. unknown format)
 *   OMR_QUANTIZATION     -> 500 (QuantizationException, ImageRegionRequestHandler.java:479)
 *   OMR_DEVICE / OMR_OOM -> 500
 *   OMR_INTERNAL         -> 500 (unchecked exceptions the reference would throw: NPE, CCE, ...)
 *
 * Threading: one omr_ctx per worker thread.  Calls on distinct contexts may run
 * concurrently; one context must not be called concurrently.  All buffers are
 * caller-owned.  Unlike the reference (global mutable compression level,
 * ImageRegionRequestHandler.java:457-460 on a Spring singleton), JPEG quality is
 * a per-call argument.
 */
#ifndef OMR_OMR_H
#define OMR_OMR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OMR_ABI_VERSION 2   /* 2 (round 4): omr_tile_job gained the projection fields */

typedef int32_t omr_status;
enum {
    OMR_OK = 0,
    OMR_INVALID_ARGUMENT = 1,
    OMR_NOT_FOUND = 2,
    OMR_QUANTIZATION = 3,
    OMR_DEVICE = 4,
    OMR_OOM = 5,
    OMR_BUFFER_TOO_SMALL = 6,
    OMR_INTERNAL = 7          /* NPE / ClassCastException / IndexOutOfBounds in the reference -> 500 */
};

/* ome.model.enums.PixelsType values the path supports. */
enum {
    OMR_PIXELS_INT8 = 0,
    OMR_PIXELS_UINT8 = 1,
    OMR_PIXELS_INT16 = 2,
    OMR_PIXELS_UINT16 = 3,
    OMR_PIXELS_INT32 = 4,
    OMR_PIXELS_UINT32 = 5,
    OMR_PIXELS_FLOAT = 6,
    OMR_PIXELS_DOUBLE = 7
};

/* ome.model.enums.Family (ImageRegionVerticle.java:72-76 lists the families). */
enum {
    OMR_FAMILY_LINEAR = 0,
    OMR_FAMILY_POLYNOMIAL = 1,
    OMR_FAMILY_LOGARITHMIC = 2,
    OMR_FAMILY_EXPONENTIAL = 3
};

/* RenderingModel: Renderer.MODEL_GREYSCALE / MODEL_RGB (ImageRegionCtx.java:333-341). */
enum { OMR_MODEL_GREYSCALE = 0, OMR_MODEL_RGB = 1 };

/* IProjection constants used by ProjectionService.java:75-91. */
enum { OMR_PROJECTION_MAX = 0, OMR_PROJECTION_MEAN = 1, OMR_PROJECTION_SUM = 2 };

/* QuantumDef + RenderingDef model (ImageRegionRequestHandler.java:262-277). */
typedef struct omr_quantum_def {
    int32_t cd_start;        /* 0 */
    int32_t cd_end;          /* 255 (QuantumFactory.DEPTH_8BIT) */
    int32_t bit_resolution;  /* 255 */
    int32_t model;           /* OMR_MODEL_* */
} omr_quantum_def;

/*
 * One ChannelBinding as the Renderer sees it after updateSettings
 * (ImageRegionRequestHandler.java:281-298 defaults, :689-741 request settings).
 */
typedef struct omr_channel_binding {
    int32_t active;           /* Renderer.setActive (:696) */
    int32_t family;           /* OMR_FAMILY_*; HTTP path is always linear (:285) */
    double coefficient;       /* curve coefficient k; HTTP path 1.0 (:286) */
    int32_t noise_reduction;  /* HTTP path false (:287) */
    int32_t reverse;          /* ReverseIntensityContext in the codomain chain (:725-726) */
    double input_start;       /* Renderer.setChannelWindow start (:703), float-rounded by ImageRegionCtx.java:313 */
    double input_end;         /* window end */
    double global_min;        /* LUT domain = StatsInfo/type range (StatsFactory.initPixelsRange, :290-291) */
    double global_max;
    uint8_t rgba[4];          /* Renderer.setRGBA (:712) */
    const uint8_t* lut;       /* setChannelLookupTable (:708): 768 bytes R[256] G[256] B[256]; NULL = use rgba */
} omr_channel_binding;

/* RegionDef (omeis.providers.re.data.RegionDef). */
typedef struct omr_region {
    int32_t x, y, width, height;
} omr_region;

typedef struct omr_ctx omr_ctx;

/* ---- context --------------------------------------------------------- */
int32_t     omr_abi_version(void);
omr_status  omr_ctx_create(int32_t device_ordinal, omr_ctx** out);
void        omr_ctx_destroy(omr_ctx* ctx);
const char* omr_last_error(const omr_ctx* ctx);
omr_status  omr_ctx_synchronize(omr_ctx* ctx);
/* Run subsequent device-side calls on a caller-owned hipStream_t (NULL = ctx's own).  A change of
 * stream waits for the work queued on the previous one when the context holds cached render
 * settings (their tables are ordered by the stream), so the previous stream must still exist. */
omr_status  omr_ctx_set_stream(omr_ctx* ctx, void* hip_stream);
void*       omr_ctx_get_stream(omr_ctx* ctx);
/*
 * Kernel timing (perf4j StopWatch analogue, ImageRegionRequestHandler.java:502): when enabled,
 * every hot-kernel launch (K2 render, K3 projection, K4 JPEG) is bracketed by HIP events on
 * the stream it is launched on.  omr_ctx_kernel_timings synchronises, writes up to `cap`
 * per-launch durations in ms (launch order) and clears the record; returns the count.
 * kind_out (optional) receives 2 = render, 3 = projection, 4 = jpeg per entry (10 = fused scaled
 * render, 11 = ARGB scaler: omr_render_scaled_batch_device; 12 = pyramid levels:
 * omr_pyramid_build_device; 20..26 = the batched PNG stages and 27 = the grey wave filter:
 * omr_encode_png_gray_batch_device; 30 = LZW decode and 31 = TIFF place:
 * omr_tiff_image_read_regions_device; 32 = zlib inflate: omr_inflate_batch_device and, with 31,
 * omr_zarr_image_read_regions_device; 33 = LZ4 decode: omr_lz4_decode_batch_device and, with 34 =
 * Blosc place, omr_zarr_image_read_regions_device on a Blosc image; 35 = Zstandard decode:
 * omr_zstd_decode_batch_device and, with 34 or 31, omr_zarr_image_read_regions_device on a
 * Blosc-Zstd or zstd image; 36 = JPEG entropy decode, 37 = JPEG IDCT and 38 = JPEG upsample /
 * colour / store: omr_jpeg_decode_batch_device and, in front of 31,
 * omr_tiff_image_read_regions_device on a JPEG image; 39 = split JPEG entropy decode and 40 = its
 * DC sums, in place of or beside 36 after omr_ctx_set_jpeg_split; 41 = JPEG 2000 code-block
 * decode, 42 = one level of the inverse 5/3 transform and 43 = JPEG 2000 colour / level shift /
 * store: omr_j2k_decode_batch_device and, in front of 31, omr_tiff_image_read_regions_device on a
 * JPEG 2000 image; 44 = one level of the inverse 9/7 transform, in place of or beside 42 for
 * irreversible streams).
 */
omr_status  omr_ctx_enable_kernel_timing(omr_ctx* ctx, int32_t enable);
int32_t     omr_ctx_kernel_timings(omr_ctx* ctx, float* ms_out, int32_t* kind_out, int32_t cap);
/* Pinned host staging (PixelBuffer tile reads land here). */
void*       omr_pinned_alloc(omr_ctx* ctx, size_t bytes);
void        omr_pinned_free(omr_ctx* ctx, void* p);

/*
 * Un-vendored upstream semantics.  The quantization, compositing and
 * JPEG-table arithmetic lives in omero:server 5.4.10 jars that are absent here, so every choice
 * that could not be pinned is a named switch; 0 (all off) is the restatement the repo defaults
 * to (DESIGN.md §2 gives the reasoning per switch).  The CPU restatement (oracle/) implements the
 * same switches, and the GPU tests cover each one against it.
 */
enum {
    /* Quantization_8_16_bit LUT window ends as Java (int) casts of the double window
     * (x < (int)start -> cdStart, x >= (int)end -> cdEnd) instead of double compares
     * (x < start, x >= end).  Integer pixel types (the LUT path) only. */
    OMR_SEM_WINDOW_INT_BOUNDS = 1u << 0,
    /* Channel colour scaling in two truncating steps, colour then alpha,
     * (int)((int)(c/255f * v) * (a/255f)), instead of (int)((c/255f * a/255f) * v).  (The
     * one-step order (int)((c/255f * v) * (a/255f)) needs no switch: it equals the default for
     * every c, a, v in 0..255, tests/test_semantics.py.) */
    OMR_SEM_ALPHA_SEPARATE = 1u << 1,
    /* Greyscale model: a .lut channel renders (R[v],G[v],B[v]) instead of ignoring the LUT. */
    OMR_SEM_GREYSCALE_LUT = 1u << 2,
    /* JPEG chroma base table K2Div2Chrominance (Annex K chroma halved, JPEGQTable) scaled by the
     * quality instead of K2Chrominance. */
    OMR_SEM_JPEG_CHROMA_DIV2 = 1u << 3,
    /* Projection glue: render every active channel.  By default
     * omr_render_projected_device reproduces the reference, whose InMemoryPlanarPixelBuffer is
     * sized sizeC = #active channels (ImageRegionRequestHandler.java:538-555) but read at the
     * original channel index (:525, :549): a rendered channel whose index is >= #active fails its
     * bounds check (DimensionsOutOfBoundsException -> 500, here OMR_INTERNAL). */
    OMR_SEM_PROJECTION_ALL_ACTIVE = 1u << 4,
    /* S2 logarithmic map without the x <= 0 guard: f(x) = Math.log(x) for every x (NaN below 0,
     * -Infinity at 0, propagated through both rounding stages as Java does: Math.round(NaN) = 0).
     * By default f(x) = x > 0 ? log(x) : 0. */
    OMR_SEM_LOG_UNGUARDED = 1u << 5,
    /* S4 noise reduction off: a channel's noiseReduction flag has no effect.  By default the first
     * and last decile of the window clip to cdStart / cdEnd. */
    OMR_SEM_NOISE_REDUCTION_OFF = 1u << 6,
    /* Exponential map on the window-normalised input (Appendix C): f(x) = exp(pow((x - start) /
     * (end - start), k)).  By default f(x) = exp(pow(x, k)), which overflows to +Infinity above
     * x ~ 709 for k = 1 (a 16-bit window then renders cdStart below its end). */
    OMR_SEM_EXP_NORMALIZED = 1u << 7,
    /* Shape mask, width % 8 == 0 with a flip: flip at pixel level (the evident intent).  By default
     * the reference is reproduced: it flips the still bit-packed buffer as if it held one byte per
     * pixel (ShapeMaskRequestHandler.java:175-181, :145-150), which indexes past the array
     * (ArrayIndexOutOfBoundsException -> the future fails -> 404, ShapeMaskVerticle.java:119-128,
     * here OMR_NOT_FOUND) unless the buffer holds >= width*height bytes, when the byte-flipped
     * buffer is rendered as packed bits. */
    OMR_SEM_MASK_PIXEL_FLIP = 1u << 8,
    OMR_SEM_ALL = 0x1FFu
};
/* Semantics of every later call on this context (renders, projections' renders, JPEG). */
omr_status omr_ctx_set_semantics(omr_ctx* ctx, uint32_t flags);
uint32_t   omr_ctx_get_semantics(const omr_ctx* ctx);
/*
 * Debug / test hook: lookups of the context's device cache of staged render settings that found
 * their setting (hits: no table-building launch in front of the render kernel) and that did not
 * (misses) since the context was created.  Both stay 0 with OMR_PLAN_CACHE=0.
 */
omr_status omr_debug_plan_cache_stats(omr_ctx* ctx, uint64_t* hits, uint64_t* misses);

/* ---- pixel buffer: ROMIO repository file -> pinned staging -> HBM ---------- */
/*
 * Replaces pixelsService.getPixelBuffer(pixels, false) (ImageRegionRequestHandler.java:302-309)
 * for repository-backed images (upstream ome.io.nio.RomioPixelBuffer):
 * one file of big-endian planes in XYZCT order, plane (z, c, t) at
 * ((t*sizeC + c)*sizeZ + z) * sizeX*sizeY*bytesPerPixel.  Read-only; safe to share between
 * contexts and threads (pread).  open: OMR_NOT_FOUND when the file does not exist,
 * OMR_INVALID_ARGUMENT when it is shorter than the dimensions say.
 */
typedef struct omr_pixel_buffer omr_pixel_buffer;
omr_status omr_pixel_buffer_open(const char* path, int32_t size_x, int32_t size_y, int32_t size_z,
                                 int32_t size_c, int32_t size_t_, int32_t pixel_type,
                                 omr_pixel_buffer** out);
void       omr_pixel_buffer_close(omr_pixel_buffer* pb);
/* RomioPixelBuffer.getPlaneOffset(z, c, t) in bytes; -1 when out of range. */
int64_t    omr_pixel_buffer_plane_offset(const omr_pixel_buffer* pb, int32_t z, int32_t c, int32_t t);
/* PixelBuffer.getTile(z, c, t, x, y, w, h): w*h pixels, rows packed, file (big-endian) byte order.
 * OMR_INVALID_ARGUMENT outside the image (DimensionsOutOfBoundsException). */
omr_status omr_pixel_buffer_get_tile(const omr_pixel_buffer* pb, int32_t z, int32_t c, int32_t t,
                                     int32_t x, int32_t y, int32_t w, int32_t h, void* dst, size_t cap);
typedef struct omr_tile_request { int32_t z, t, x, y; } omr_tile_request;
/*
 * n render_image_region tile requests (ImageRegionRequestHandler.java:430-600: getPixelBuffer ->
 * renderAsPackedInt -> flip) of one image at one rendering setting, all width x height: reader
 * threads pread each group of tiles straight into pinned memory while the previous group is
 * copied to HBM (own copy stream), rendered (K1+K2) and copied back.  argb_out: n*height*width
 * uint32 in host memory (out_on_device 0; pinned memory from omr_pinned_alloc skips a bounce
 * copy) or in device memory (1: e.g. for omr_encode_jpeg_batch_device).  Synchronous.
 */
/* Tile rows DMA'd straight from the registered file mapping (1, default) or copied by reader
 * threads into pinned staging first (0).  The DMA path falls back to staging on its own when the
 * driver refuses to register the mapping. */
omr_status omr_ctx_set_pixel_buffer_dma(omr_ctx* ctx, int32_t enable);
omr_status omr_render_pixel_buffer_tiles(omr_ctx* ctx, const omr_pixel_buffer* pb,
                                         const omr_quantum_def* qdef,
                                         const omr_channel_binding* channels, int32_t size_c,
                                         const omr_tile_request* reqs, int32_t n, int32_t width,
                                         int32_t height, int32_t flip_h, int32_t flip_v,
                                         uint32_t* argb_out, int32_t out_on_device);

/* ---- plane statistics and histograms (K9) ---------------------------------- */
/*
 * What webgateway/histogram_json serves, and what fills omr_channel_binding.global_min /
 * global_max (OMERO's StatsInfo) when the caller has none.  The reference snapshot predates the
 * endpoint, so the rule is this library's own, modelled on RawPixelsStore.getHistogram.
 *
 * A plane is width x height pixels of one OMR_PIXELS_* type, big-endian (file order) or native,
 * row_stride_px pixels between row starts (0 = width); region NULL = the whole plane.  Every
 * pixel v is taken as a double (exact for every type).
 *   statistics  nan_count = NaN pixels; count = w*h - nan_count; min / max over the others
 *               (+-Infinity take part); min = +Infinity, max = -Infinity when count is 0.
 *   histogram   NaN -> nan_count; v < lo -> below; v > hi -> above; else, in IEEE double with one
 *               rounding per operation,
 *                   range = hi - lo + 1.0;  bin_range = range / (double)bin_count;
 *                   bin   = min((int64)((v - lo) / bin_range), bin_count - 1)
 *               (the + 1.0 for every type, float included: OMERO's rule).
 *               sum(counts) + below + above + nan_count == w*h.
 * OMR_INVALID_ARGUMENT, decided before any launch (the context stays usable): a NULL pointer, an
 * unknown pixel type, n_planes outside 1..32, bin_count outside 1..OMR_HIST_MAX_BINS, lo, hi or
 * hi - lo not finite, lo > hi, width, height or a region side <= 0, a region that leaves the
 * plane, 0 < row_stride_px < width, a region of 2^32 pixels or more, a plane pointer that is not
 * a multiple of the pixel size.
 */
typedef struct omr_plane_stats { double min, max; uint64_t count, nan_count; } omr_plane_stats;
typedef struct omr_histogram_info { double lo, hi; uint64_t below, above, nan_count; } omr_histogram_info;
enum {
    OMR_HIST_RANGE_TYPE = 0,      /* the pixel-type range of omr_create_rendering_def (usePixelsTypeRange) */
    OMR_HIST_RANGE_PLANE = 1,     /* the region's own min / max; no non-NaN pixel: every count 0, OMR_OK */
    OMR_HIST_RANGE_EXPLICIT = 2   /* the caller's lo / hi (e.g. StatsInfo) */
};
enum { OMR_HIST_MAX_BINS = 4096 };

/* The rule, on the host: bin index, or -1 below, -2 above, -3 NaN. */
int32_t    omr_histogram_bin_of(double v, double lo, double hi, int32_t bin_count);

/* d_planes: HOST array of n_planes device pointers; results in HOST memory; synchronous, on the
 * context's stream. */
omr_status omr_plane_stats_device(omr_ctx* ctx, const void* const* d_planes, int32_t n_planes,
                                  int32_t pixel_type, int32_t big_endian, int32_t width, int32_t height,
                                  int64_t row_stride_px, const omr_region* region,
                                  omr_plane_stats* stats_out /* [n_planes] */);
omr_status omr_histogram_device(omr_ctx* ctx, const void* const* d_planes, int32_t n_planes,
                                int32_t pixel_type, int32_t big_endian, int32_t width, int32_t height,
                                int64_t row_stride_px, const omr_region* region,
                                const double* lo, const double* hi /* [n_planes] */, int32_t bin_count,
                                uint32_t* counts_out /* [n_planes][bin_count] */,
                                omr_histogram_info* info_out /* [n_planes] */);
/* One host plane (rows packed): upload, statistics pass when range_mode or stats_out (may be
 * NULL) needs it, histogram.  lo / hi are read in OMR_HIST_RANGE_EXPLICIT only. */
omr_status omr_histogram(omr_ctx* ctx, const void* plane, int32_t pixel_type, int32_t big_endian,
                         int32_t width, int32_t height, const omr_region* region, int32_t range_mode,
                         double lo, double hi, int32_t bin_count, uint32_t* counts_out,
                         omr_histogram_info* info_out, omr_plane_stats* stats_out);
/* histogram_json for plane (z, c, t) of a ROMIO buffer: only the region's rows are read (the tile
 * read, into pinned memory), copied on the copy stream and counted on the context's.
 * OMR_INVALID_ARGUMENT for z, c or t outside the image, as omr_pixel_buffer_get_tile. */
omr_status omr_pixel_buffer_histogram(omr_ctx* ctx, const omr_pixel_buffer* pb, int32_t z, int32_t c,
                                      int32_t t, const omr_region* region, int32_t range_mode,
                                      double lo, double hi, int32_t bin_count, uint32_t* counts_out,
                                      omr_histogram_info* info_out, omr_plane_stats* stats_out);

/* ---- resolution pyramids (K11) ---------------------------------------------- */
/*
 * The levels behind tile=res,x,y[,w,h] (getResolutionLevels / getResolutionDescriptions,
 * ImageRegionRequestHandler.java:446-454, :792-795, :840-853).  The reference snapshot has no
 * pyramid writer (OMERO's PixelsService.makePyramid is not vendored), so the rule below is the
 * library's own, as for K9 and K10.
 *
 * Level sizes.  Level k (0 = full size) is floor(W / 2^k) x floor(H / 2^k); n_levels counts
 * level 0.  A valid pyramid has 1 <= n_levels <= OMR_PYRAMID_MAX_LEVELS and
 * n_levels <= 1 + floor(log2(min(W, H))): every level then has both sides >= 1 and every 2x2 box
 * lies inside its source.  A trailing odd row or column of a level contributes nothing to the next.
 *
 * Downsampling.  Both rules cascade: level k is made from the stored level k-1.
 *   OMR_PYRAMID_SUBSAMPLE  L_k[j][i] = L_{k-1}[2j][2i], i.e. level-0 pixel (i*2^k, j*2^k); the
 *                          bytes are copied verbatim (NaN payloads survive).
 *   OMR_PYRAMID_MEAN       with a, b, c, d = L_{k-1}[2j][2i], [2j][2i+1], [2j+1][2i], [2j+1][2i+1]:
 *                          8-, 16- and 32-bit integers, signed and unsigned:
 *                              floor((a + b + c + d + 2) / 4) in int64 (half rounds towards
 *                              +infinity, an arithmetic shift for negatives; always fits the type);
 *                          float:  (float)((((double)a + (double)b) + ((double)c + (double)d)) * 0.25);
 *                          double: ((a + b) + (c + d)) * 0.25;
 *                          one IEEE rounding per operation (no fused multiply-add); NaN propagates.
 * Levels keep the byte order of level 0; output planes are packed (row stride = level width).
 */
enum { OMR_PYRAMID_SUBSAMPLE = 0, OMR_PYRAMID_MEAN = 1 };
#define OMR_PYRAMID_MAX_LEVELS 16
#define OMR_PYRAMID_DEFAULT_MIN_SIDE 256   /* OMERO's tile side */
/* The smallest n >= 1 with max(size_x >> (n-1), size_y >> (n-1)) <= min_side, capped by the bounds
 * above; negative (-OMR_INVALID_ARGUMENT) for min_side < 1 or a non-positive size.  Host only. */
int32_t    omr_pyramid_level_count(int32_t size_x, int32_t size_y, int32_t min_side);
/* (w, h) pairs of levels 0..n_levels-1 into sizes_out[2*n_levels], largest first: the order of
 * getResolutionDescriptions and of omr_get_region_def's level_sizes.  OMR_INVALID_ARGUMENT for an
 * n_levels outside the bounds above.  Host only. */
omr_status omr_pyramid_level_sizes(int32_t size_x, int32_t size_y, int32_t n_levels, int32_t* sizes_out);
/*
 * K11: levels 1..n_levels-1 of n_planes (1..32) planes already in HBM.  d_planes is a HOST array
 * of n_planes device pointers (rows row_stride_px pixels apart, 0 = width); d_levels_out is a HOST
 * array of n_levels-1 device bases: plane p of level k goes to d_levels_out[k-1] + p * w_k*h_k*bpp.
 * All eight pixel types.  Level 0 is read once: one launch writes up to four levels (three for 32-
 * and 64-bit pixels) from registers and further levels come from re-running the kernel on the last
 * level written; omr_ctx_kernel_timings reports kind 12 per launch.  No atomics: two calls give
 * identical bytes.  Planes, strides or widths off the 16-byte grid take a per-pixel form of the
 * same rule; no shape is refused.  OMR_INVALID_ARGUMENT, decided before any launch (the context
 * stays usable): a NULL pointer, an unknown type or rule, n_planes outside 1..32, n_levels outside
 * the bounds above, 0 < row_stride_px < width, width*height >= 2^31, a plane or level pointer that
 * is not a multiple of the pixel size.  n_levels == 1 is OMR_OK and launches nothing.
 * Asynchronous on the context stream.
 */
omr_status omr_pyramid_build_device(omr_ctx* ctx, const void* const* d_planes, int32_t n_planes,
                                    int32_t pixel_type, int32_t big_endian, int32_t width, int32_t height,
                                    int64_t row_stride_px, int32_t rule, int32_t n_levels,
                                    void* const* d_levels_out);
/*
 * Pyramid sidecar file of a ROMIO pixel buffer.  A 64-byte little-endian header:
 *     bytes  0..7   magic "OMRPYR1\0"
 *     uint32 version (1), rule (OMR_PYRAMID_*), pixel_type, n_levels            (bytes  8..23)
 *     int32  size_x, size_y, size_z, size_c, size_t of level 0                  (bytes 24..43)
 *     zero padding                                                              (bytes 44..63)
 * then levels 1..n_levels-1, each in ROMIO layout (big-endian planes in XYZCT order at the
 * level's size), each starting at the next multiple of 4096 bytes; gaps are zero and the file
 * ends with the last level's last byte.  The same input and rule give identical bytes.
 *
 * build_pyramid: reads pb's planes, runs K11 on groups of up to 32 planes (the next group's copy
 * overlaps the current group's kernel), copies the levels back and writes sidecar_path + ".tmp",
 * then renames it to sidecar_path.  n_levels <= 0: omr_pyramid_level_count(size_x, size_y, 256).
 * Synchronous.  An I/O failure is OMR_INTERNAL with the errno text in omr_last_error.  It does not
 * attach the file.
 */
omr_status omr_pixel_buffer_build_pyramid(omr_ctx* ctx, const omr_pixel_buffer* pb, int32_t rule,
                                          int32_t n_levels, const char* sidecar_path);
/* Attach a sidecar (host only: no context, no GPU): magic, version, pixel type, the five
 * dimensions, the n_levels bounds and the file length are validated.  OMR_NOT_FOUND for a missing
 * file, OMR_INVALID_ARGUMENT for anything else; a second attach replaces the first.  Not to be
 * called while another thread uses pb (views taken before stay valid). */
omr_status omr_pixel_buffer_attach_pyramid(omr_pixel_buffer* pb, const char* sidecar_path);
/* getResolutionLevels: n_levels of the attached pyramid, 1 without one (0 for NULL). */
int32_t    omr_pixel_buffer_resolution_levels(const omr_pixel_buffer* pb);
/* getResolutionDescriptions: up to cap_pairs (w, h) pairs, largest first; returns the level count
 * (negative -OMR_INVALID_ARGUMENT for a NULL argument). */
int32_t    omr_pixel_buffer_resolution_descriptions(const omr_pixel_buffer* pb, int32_t* sizes_out,
                                                    int32_t cap_pairs);
/*
 * A resolution level as a pixel buffer of its own.  resolution is the request's index (0 = full
 * size), i.e. the index into the descriptions (omr_resolution_level gives the omeis number).  The
 * view has the level's size_x / size_y, the parent's z, c, t and pixel type and its own identity
 * for the batcher's caches, works with every call that takes an omr_pixel_buffer (get_tile,
 * plane_offset, omr_render_pixel_buffer_tiles, histogram, batcher and pool jobs, projections) and
 * is closed with omr_pixel_buffer_close; views and parent share the file mappings by reference
 * count, so the closing order does not matter.  A view itself reports one level.
 * OMR_INVALID_ARGUMENT for a resolution outside 0..n_levels-1.
 */
omr_status omr_pixel_buffer_level(const omr_pixel_buffer* pb, int32_t resolution, omr_pixel_buffer** view);

/* ---- request batching ------------------------------ */
/*
 * Concurrent render_image_region requests coalesced into GPU batches.  The reference runs each
 * request on its own worker thread (ImageRegionMicroserviceVerticle.java:149-165) with its own
 * Renderer (ImageRegionRequestHandler.java:436-440) and caches finished regions in Redis under
 * ImageRegionCtx.cacheKey (ImageRegionCtx.java:165-177).  A batcher owns one GPU context and a
 * dispatcher thread: submitted jobs are grouped by image + rendering settings + tile size + flip +
 * format, each group is rendered by one omr_render_pixel_buffer_tiles call and encoded by one
 * batched JPEG / PNG launch, and identical tiles in flight together are rendered once.
 * Projection requests (p=intmax|intmean|intsum, :506-558) are jobs with has_projection set: the
 * active channels' Z-stacks at t go to HBM by DMA, K3 + K2 (or K3R) project and render the full
 * plane, and the group's planes are encoded in one batch; jobs with the same image, settings,
 * projection and t are rendered once.  Shape masks (render_shape_mask,
 * ShapeMaskRequestHandler.java:165-207, one per worker at ShapeMaskVerticle.java:121-149) are
 * jobs of their own (omr_batcher_submit_mask): every mask of a dispatch round is encoded by one
 * omr_render_shape_mask_png_batch call.  A failing job (OMR_QUANTIZATION, the quirk-3 OMR_INTERNAL
 * of the projection glue, a mask's 404) fails alone.
 * submit/wait are thread-safe; the pixel buffer must outlive its jobs.
 */
enum { OMR_FORMAT_JPEG = 0, OMR_FORMAT_PNG = 1, OMR_FORMAT_ARGB = 2 /* packed int[] */,
       OMR_FORMAT_TIFF = 3 /* TIFFImageWriter branch, :583-596 */ };
typedef struct omr_tile_job {
    const omr_pixel_buffer* pb;
    const struct omr_quantum_def* qdef;            /* copied at submit */
    const struct omr_channel_binding* channels;    /* size_c entries, copied (LUTs too) */
    int32_t size_c;
    int32_t z, t, x, y, width, height;
    int32_t flip_h, flip_v;
    int32_t format;                                /* OMR_FORMAT_*; others -> OMR_NOT_FOUND (404) */
    float quality;                                 /* JPEG */
    /* p=intmax|intmean|intsum[|start:end] (ImageRegionCtx.projection, ImageRegionRequestHandler.java
     * :506-558): with has_projection != 0 every active channel is projected (OMR_PROJECTION_*) over
     * z in [projection_start, projection_end] at t -- a negative bound takes the reference's default,
     * 0 / sizeZ - 1 (:510-515) -- and the full projected plane is rendered: z, x, y, width and height
     * are ignored, as the glue replaces the plane definition (:550-552).  Zero-initialised: none. */
    int32_t has_projection, projection, projection_start, projection_end;
} omr_tile_job;
struct omr_mask_job;   /* shape-mask job, declared with omr_render_shape_mask_png_batch below */
typedef struct omr_batcher omr_batcher;
omr_status omr_batcher_create(int32_t device_ordinal, int32_t max_batch, int32_t max_wait_us,
                              omr_batcher** out);
void       omr_batcher_destroy(omr_batcher* b);
omr_status omr_batcher_submit(omr_batcher* b, const omr_tile_job* job, uint64_t* ticket);
/* A render_shape_mask job (the mask bytes are copied at submit); its result is the PNG file. */
omr_status omr_batcher_submit_mask(omr_batcher* b, const struct omr_mask_job* job, uint64_t* ticket);
/* Blocks until the job is done; copies its encoded bytes.  OMR_BUFFER_TOO_SMALL sets *len and
 * keeps the result for a retry with a larger buffer. */
omr_status omr_batcher_wait(omr_batcher* b, uint64_t ticket, uint8_t* out, size_t cap, size_t* len);
/* jobs submitted, dispatch rounds, tiles rendered (distinct renders: tiles, projected planes and
 * masks), duplicate jobs served from a sibling job's result */
omr_status omr_batcher_stats(omr_batcher* b, uint64_t stats_out[4]);
/* OMR_SEM_* flags for jobs submitted after this call (each job keeps the flags it was submitted
 * under; jobs with different flags never share a render). */
omr_status omr_batcher_set_semantics(omr_batcher* b, uint32_t flags);
/* HBM stack cache of the projection jobs: the (pixel buffer, c, t) Z-stacks stay resident (least
 * recently used evicted) up to max_bytes (default 4 GiB, env OMR_STACK_CACHE_MB; 0 disables), so
 * repeated p= requests on an image skip the PCIe upload.  stats: hits, misses, resident bytes. */
omr_status omr_batcher_set_stack_cache(omr_batcher* b, int64_t max_bytes);
omr_status omr_batcher_stack_cache_stats(omr_batcher* b, uint64_t stats_out[3]);

/* ---- node-level serving pool: the request batches of all worker threads over the node's GPUs ---- */
/*
 * The reference's only parallelism is N worker-verticle instances over one worker pool
 * (ImageRegionMicroserviceVerticle.java:84-85, :149-165).  A pool holds one batcher per entry of
 * devices[] (its own context, stream, dispatcher thread and plan / LUT replicas in that GPU's
 * HBM; an ordinal may repeat, e.g. two batchers on one card) and sends each submitted job to the
 * batcher with the fewest jobs queued or in flight.  Tiles are independent, so nothing crosses
 * between GPUs: no collective, no peer copies.  submit / wait are thread-safe and keep the
 * batcher's per-tile statuses (OMR_QUANTIZATION fails only its own tile).  At most 256 devices.
 */
typedef struct omr_pool omr_pool;
omr_status omr_pool_create(const int32_t* devices, int32_t n_devices, int32_t max_batch, int32_t max_wait_us,
                           omr_pool** out);
void       omr_pool_destroy(omr_pool* p);
int32_t    omr_pool_size(const omr_pool* p);
omr_status omr_pool_submit(omr_pool* p, const omr_tile_job* job, uint64_t* ticket);
omr_status omr_pool_submit_mask(omr_pool* p, const struct omr_mask_job* job, uint64_t* ticket);
/* omr_batcher_wait of the batcher holding the ticket. */
omr_status omr_pool_wait(omr_pool* p, uint64_t ticket, uint8_t* out, size_t cap, size_t* len);
/* Index into devices[] of the batcher a ticket went to (-1: not a ticket of this pool). */
int32_t    omr_pool_device_index(const omr_pool* p, uint64_t ticket);
omr_status omr_pool_set_semantics(omr_pool* p, uint32_t flags);
omr_status omr_pool_set_stack_cache(omr_pool* p, int64_t max_bytes_per_device);
/* stats_out[4*i .. 4*i+3] = omr_batcher_stats of device i; n_entries >= omr_pool_size. */
omr_status omr_pool_stats(omr_pool* p, uint64_t* stats_out, int32_t n_entries);

/* ---- render (quantize + codomain + composite + flip) ------------------ */
/*
 * Replaces renderer.renderAsPackedInt(planeDef, null)  (ImageRegionRequestHandler.java:559)
 * followed by flip(buf, sizeX, sizeY, flipH, flipV)      (ImageRegionRequestHandler.java:574-575, :616-642).
 * planes[c] points at the region of channel c (size_c pointers; NULL allowed for inactive
 * channels); row_stride is in pixels (0 = width).  big_endian: ROMIO planes are big-endian.
 * Host memory in and out; synchronous.
 */
omr_status omr_render_packed_int(omr_ctx* ctx, const omr_quantum_def* qdef,
                                 const omr_channel_binding* channels, int32_t size_c,
                                 const void* const* planes, int64_t row_stride,
                                 int32_t pixel_type, int32_t big_endian,
                                 int32_t width, int32_t height,
                                 int32_t flip_h, int32_t flip_v,
                                 uint32_t* argb_out);

/* Same, device pointers, asynchronous on the context stream. */
omr_status omr_render_packed_int_device(omr_ctx* ctx, const omr_quantum_def* qdef,
                                        const omr_channel_binding* channels, int32_t size_c,
                                        const void* const* d_planes, int64_t row_stride,
                                        int32_t pixel_type, int32_t big_endian,
                                        int32_t width, int32_t height,
                                        int32_t flip_h, int32_t flip_v,
                                        uint32_t* d_argb_out);

/*
 * Batch of n_tiles same-settings tile requests (one viewer's tiles; the request-level
 * parallelism of ImageRegionMicroserviceVerticle.java:149-165 coalesced into one launch).
 * d_plane_ptrs: DEVICE array of n_tiles*size_c device pointers ([tile][channel]); each plane
 * must start 16-byte aligned when width and row_stride are multiples of 16 bytes' worth of pixels
 * (the vector path: 16-B loads), which the library cannot check on the host.
 * d_argb_out: device [n_tiles][height][width].  d_status (optional, device int32[n_tiles]):
 * per-tile OMR_OK / OMR_QUANTIZATION.  Asynchronous on the context stream.
 */
omr_status omr_render_batch_device(omr_ctx* ctx, const omr_quantum_def* qdef,
                                   const omr_channel_binding* channels, int32_t size_c,
                                   const void* const* d_plane_ptrs, int32_t n_tiles,
                                   int64_t row_stride, int32_t pixel_type, int32_t big_endian,
                                   int32_t width, int32_t height,
                                   int32_t flip_h, int32_t flip_v,
                                   uint32_t* d_argb_out, int32_t* d_status);

/*
 * Same batch with the planes laid out regularly in device memory (e.g. a pyramid level kept
 * resident as [tile][channel][y][x]): plane(t, c) = d_base + t*tile_stride_bytes +
 * c*channel_stride_bytes.  No pointer table; otherwise identical to omr_render_batch_device.
 */
omr_status omr_render_batch_strided_device(omr_ctx* ctx, const omr_quantum_def* qdef,
                                           const omr_channel_binding* channels, int32_t size_c,
                                           const void* d_base, int64_t tile_stride_bytes,
                                           int64_t channel_stride_bytes, int32_t n_tiles,
                                           int64_t row_stride, int32_t pixel_type, int32_t big_endian,
                                           int32_t width, int32_t height,
                                           int32_t flip_h, int32_t flip_v,
                                           uint32_t* d_argb_out, int32_t* d_status);

/* ---- scaled rendering: thumbnails and bird's-eye views (K10) ------------- */
/*
 * The scaling rule (the library's own; the reference snapshot has no thumbnail code): an exact
 * area-weighted mean, rounded half up.  Source W x H, output tw x th with 1 <= tw <= W and
 * 1 <= th <= H (downscale or identity; anything else is OMR_INVALID_ARGUMENT), W*H < 2^31.
 * In units of 1/tw source column x covers [x*tw, (x+1)*tw) and output column i covers
 * [i*W, (i+1)*W); wx[i][x] is the length of their overlap, an integer in 0..tw with
 * sum_x wx[i][x] = W.  wy[j][y] is the same from H and th.  For each of the four bytes b of the
 * packed ARGB, in non-negative integers with floor division:
 *
 *     out[j][i].b = (sum_y sum_x wy[j][y] * wx[i][x] * src[y][x].b + (W*H)/2) / (W*H)
 *
 * The alpha byte goes through the same formula (a render writes 0xFF, which stays 0xFF); the
 * identity size returns the source.  Flips apply to the full-size render first, as in
 * omr_render_*, which for this rule equals flipping the small image.  The sums are integers and
 * order-free: two calls return identical bytes, and the result is exact at every size (sums are
 * 64-bit once 255*W*H + W*H/2 no longer fits 32 bits, from about 4100 x 4100).
 *
 * omr_scale_argb_device: the rule on n ARGB images already in HBM, image k at
 * d_src + k*src_image_stride_px with rows src_row_stride_px apart (0 = packed), into
 * d_dst [n][dst_h][dst_w].  Asynchronous on the context stream.
 */
omr_status omr_scale_argb_device(omr_ctx* ctx, const uint32_t* d_src, int32_t n, int32_t src_w, int32_t src_h,
                                 int64_t src_row_stride_px, int64_t src_image_stride_px, uint32_t* d_dst,
                                 int32_t dst_w, int32_t dst_h);
/*
 * render_thumbnail / render_birds_eye_view: omr_render_batch_device followed by the rule, i.e.
 * n_tiles whole planes rendered with one setting and handed back out_w x out_h each
 * (d_argb_out: device [n_tiles][out_h][out_w]; one image is n_tiles = 1, which must be >= 1).
 * d_status (optional, device int32[n_tiles]): per-image OMR_OK / OMR_QUANTIZATION.
 * 8/16-bit integer pixels with 1..4 active channels go through one kernel that quantizes,
 * composites and reduces (the full-size ARGB never reaches HBM) when width is a multiple of 8
 * pixels and every plane and row starts on an 8-pixel boundary, i.e. 16-byte aligned for 16-bit and
 * 8-byte aligned for 8-bit pixels (pointer-table planes: the caller's contract, as for
 * omr_render_batch_device), out_w <= 1024 and width*out_w < 2^31.  Everything
 * else, and every call of a context created with OMR_SCALE_FUSED=0 in the environment, renders
 * full size into a context buffer and scales that: identical bytes either way.
 * omr_ctx_kernel_timings reports kind 10 for the fused kernel and kind 11 for the ARGB scaler
 * (behind a kind-2 render on the unfused route).  Asynchronous on the context stream.
 */
omr_status omr_render_scaled_batch_device(omr_ctx* ctx, const omr_quantum_def* qdef,
                                          const omr_channel_binding* channels, int32_t size_c,
                                          const void* const* d_plane_ptrs, int32_t n_tiles,
                                          int64_t row_stride, int32_t pixel_type, int32_t big_endian,
                                          int32_t width, int32_t height,
                                          int32_t flip_h, int32_t flip_v,
                                          uint32_t* d_argb_out, int32_t* d_status,
                                          int32_t out_w, int32_t out_h);
/* Same with the strided plane layout of omr_render_batch_strided_device. */
omr_status omr_render_scaled_batch_strided_device(omr_ctx* ctx, const omr_quantum_def* qdef,
                                                  const omr_channel_binding* channels, int32_t size_c,
                                                  const void* d_base, int64_t tile_stride_bytes,
                                                  int64_t channel_stride_bytes, int32_t n_tiles,
                                                  int64_t row_stride, int32_t pixel_type, int32_t big_endian,
                                                  int32_t width, int32_t height,
                                                  int32_t flip_h, int32_t flip_v,
                                                  uint32_t* d_argb_out, int32_t* d_status,
                                                  int32_t out_w, int32_t out_h);
/*
 * Thumbnail size by OMERO's longest-side rule, host only.  big = max(size_x, size_y): when
 * big <= longest_side the image keeps its own size (no upscaling, unlike OMERO); otherwise the
 * long side becomes longest_side and the short side max(1, short*longest_side / big) (int64
 * floor division).  longest_side < 1 or a non-positive size is OMR_INVALID_ARGUMENT.
 */
omr_status omr_thumbnail_size(int32_t size_x, int32_t size_y, int32_t longest_side, int32_t* out_w, int32_t* out_h);

/*
 * Standalone output flip of an already-rendered ARGB buffer on the device
 * (ImageRegionRequestHandler.flip, :616-642).  src and dest must not alias.
 * Identity (no flip) copies.
 */
omr_status omr_flip_argb_device(omr_ctx* ctx, const uint32_t* d_src, uint32_t* d_dest,
                                int32_t size_x, int32_t size_y, int32_t flip_h, int32_t flip_v);
/* ShapeMaskRequestHandler.flip(byte[]...) (:128-154), byte-per-pixel. */
omr_status omr_flip_mask_device(omr_ctx* ctx, const uint8_t* d_src, uint8_t* d_dest,
                                int32_t size_x, int32_t size_y, int32_t flip_h, int32_t flip_v);

/* ---- Z-projection ------------------------------------------------------ */
/*
 * ProjectionService.projectStack(pixels, buf, alg, t, c, stepping, start, end)
 * (ProjectionService.java:46-120): one channel's stack [size_z][size_y][size_x] -> one plane
 * of the same pixel type.  Max over z in [start,end] inclusive; mean/sum over [start,end)
 * (ProjectionService.java:184 vs :271).  Host memory; synchronous.
 *
 * Stepping: the planes read are z = start + i * stepping for i < omr_projection_plane_count(),
 * counted in 64 bits, so a stepping up to INT32_MAX is valid while start + stepping <= INT32_MAX
 * (start = 0, stepping = INT32_MAX projects plane 0).  Every projection call answers
 * OMR_INVALID_ARGUMENT when the loop runs at least once (start <= end for max, start < end for
 * mean and sum) and (int64)start + stepping > INT32_MAX -- in general, when z after the last
 * plane read would pass INT32_MAX: there the reference's int z wraps negative, its loop goes
 * on and the plane read throws.
 */
/* The number of planes a projection reads (0 for an empty range), or the rejection above.  Also
 * OMR_INVALID_ARGUMENT for a negative bound, stepping <= 0 or an unknown algorithm.  No context. */
omr_status omr_projection_plane_count(int32_t algorithm, int32_t start, int32_t end, int32_t stepping,
                                      int64_t* count);
omr_status omr_project_stack(omr_ctx* ctx, const void* stack, int32_t pixel_type,
                             int32_t big_endian_in, int32_t size_x, int32_t size_y, int32_t size_z,
                             int32_t algorithm, int32_t start, int32_t end, int32_t stepping,
                             void* plane_out, int32_t big_endian_out);
omr_status omr_project_stack_device(omr_ctx* ctx, const void* d_stack, int32_t pixel_type,
                                    int32_t big_endian_in, int32_t size_x, int32_t size_y,
                                    int32_t size_z, int32_t algorithm, int32_t start, int32_t end,
                                    int32_t stepping, void* d_plane_out, int32_t big_endian_out);
/*
 * n_stacks same-geometry stacks (e.g. every active channel of one p= request, the glue's
 * projectStack loop at ImageRegionRequestHandler.java:516-533) projected in one launch.
 * d_stacks / d_planes_out: HOST arrays of n_stacks device pointers; n_stacks <= 32.
 * Asynchronous on the context stream.
 */
omr_status omr_project_stacks_device(omr_ctx* ctx, const void* const* d_stacks, int32_t n_stacks,
                                     int32_t pixel_type, int32_t big_endian_in, int32_t size_x,
                                     int32_t size_y, int32_t size_z, int32_t algorithm, int32_t start,
                                     int32_t end, int32_t stepping, void* const* d_planes_out,
                                     int32_t big_endian_out);
/*
 * Projection glue + render (ImageRegionRequestHandler.java:506-559): project every active
 * channel's stack (d_stacks[c], NULL for inactive) and render the full projected plane.
 * Projected planes stay in HBM (native byte order); output device [size_y][size_x].
 */
omr_status omr_render_projected_device(omr_ctx* ctx, const omr_quantum_def* qdef,
                                       const omr_channel_binding* channels, int32_t size_c,
                                       const void* const* d_stacks, int32_t pixel_type,
                                       int32_t big_endian, int32_t size_x, int32_t size_y,
                                       int32_t size_z, int32_t algorithm, int32_t start,
                                       int32_t end, int32_t stepping, int32_t flip_h,
                                       int32_t flip_v, uint32_t* d_argb_out);

/* ---- encode --------------------------------------------------------------- */
/* Upper bound of the encoded size (callers size `out` with it). */
size_t omr_jpeg_max_bytes(int32_t width, int32_t height);
size_t omr_png_max_bytes(int32_t width, int32_t height, int32_t channels);
/*
 * JPEG baseline (JFIF, YCbCr 4:2:0, IJG islow FDCT, Java ImageIO quality scaling,
 * standard Huffman tables) of the 24-bit RGB view of ARGB pixels
 * (ImageUtil.createBufferedImage + compressionService.compressToStream,
 *  ImageRegionRequestHandler.java:576-582).  Quality is per call.
 * Host ARGB in, host bytes out.  *out_len always receives the file length; a NULL `out` or
 * cap < length returns OMR_BUFFER_TOO_SMALL (query, then call again).  Tiles up to 4096 px
 * run the batched pipeline below with one tile; larger images the single-tile kernels.
 */
omr_status omr_encode_jpeg(omr_ctx* ctx, const uint32_t* argb, int32_t width, int32_t height,
                           float quality, uint8_t* out, size_t cap, size_t* out_len);
/* Device ARGB in (e.g. straight from omr_render_*_device), host bytes out. */
omr_status omr_encode_jpeg_device(omr_ctx* ctx, const uint32_t* d_argb, int32_t width,
                                  int32_t height, float quality, uint8_t* out, size_t cap,
                                  size_t* out_len);
/*
 * Batched JPEG (same encoder, byte-identical per tile) of n_tiles device ARGB tiles
 * (tile i at d_argb + i*tile_stride_px; 0 = width*height), e.g. the output of
 * omr_render_batch_*_device.  Complete JFIF files are packed back to back in d_out
 * (capacity out_cap bytes): file i at d_out + d_offsets[i], d_lengths[i] bytes (0 and
 * d_status[i] = OMR_BUFFER_TOO_SMALL when it did not fit; d_status optional).
 * Asynchronous on the context stream; width, height <= 4096.  This is the batch form of the
 * per-request compressToStream calls (ImageRegionRequestHandler.java:580-582).
 */
omr_status omr_encode_jpeg_batch_device(omr_ctx* ctx, const uint32_t* d_argb, int64_t tile_stride_px,
                                        int32_t n_tiles, int32_t width, int32_t height, float quality,
                                        uint8_t* d_out, size_t out_cap, uint64_t* d_offsets,
                                        uint32_t* d_lengths, int32_t* d_status);
/*
 * render_image_region's default response for a batch of tiles in one call: render (quantize,
 * codomain, composite, flip: renderAsPackedInt + flip, :559, :574-575) and JPEG-encode
 * (createBufferedImage + compressToStream, :576-582) n_tiles same-settings tiles whose planes
 * are already in HBM.  Output exactly as omr_encode_jpeg_batch_device (byte-identical files);
 * d_status[i] (optional) also reports OMR_QUANTIZATION for a tile with a pixel outside its LUT
 * domain.  8/16-bit integer pixels with 1..4 active channels on tiles whose sides are multiples
 * of 16 render inside the encoder's first kernel (the ARGB tile never reaches HBM); other
 * requests render with K2 first.  Plane rows must start 4-byte aligned (16-bit) / 2-byte
 * aligned (8-bit) for the fused path.  Asynchronous on the context stream.
 */
omr_status omr_render_jpeg_batch_strided_device(omr_ctx* ctx, const omr_quantum_def* qdef,
                                                const omr_channel_binding* channels, int32_t size_c,
                                                const void* d_base, int64_t tile_stride_bytes,
                                                int64_t channel_stride_bytes, int32_t n_tiles, int64_t row_stride,
                                                int32_t pixel_type, int32_t big_endian, int32_t width, int32_t height,
                                                int32_t flip_h, int32_t flip_v, float quality, uint8_t* d_out,
                                                size_t out_cap, uint64_t* d_offsets, uint32_t* d_lengths,
                                                int32_t* d_status);
/*
 * One render_image_region request in its default format (format=jpeg, ImageRegionCtx.java:146):
 * renderAsPackedInt + flip + createBufferedImage + compressToStream
 * (ImageRegionRequestHandler.java:559-582) of one tile whose planes are already in HBM, the JPEG
 * file landing in `out` (host memory).  d_planes is a HOST array of size_c device pointers, one per
 * channel (an inactive channel's may be null).  Same files as omr_render_packed_int_device +
 * omr_encode_jpeg_device, in one call with one stream sync (K2's small-launch render + the one-tile
 * JPEG pipeline: measured faster for a single tile than the fused kernel).  Synchronous; a pixel outside its LUT
 * domain returns OMR_QUANTIZATION (-> 500); *out_len is set whenever the length is known
 * (OMR_BUFFER_TOO_SMALL when cap is short).  Tiles up to 4096 x 4096.
 */
omr_status omr_render_jpeg(omr_ctx* ctx, const omr_quantum_def* qdef, const omr_channel_binding* channels,
                           int32_t size_c, const void* const* d_planes, int64_t row_stride, int32_t pixel_type,
                           int32_t big_endian, int32_t width, int32_t height, int32_t flip_h, int32_t flip_v,
                           float quality, uint8_t* out, size_t cap, size_t* out_len);
/* Same with a device plane-pointer table [tile][channel] (omr_render_batch_device's layout). */
omr_status omr_render_jpeg_batch_device(omr_ctx* ctx, const omr_quantum_def* qdef,
                                        const omr_channel_binding* channels, int32_t size_c,
                                        const void* const* d_plane_ptrs, int32_t n_tiles, int64_t row_stride,
                                        int32_t pixel_type, int32_t big_endian, int32_t width, int32_t height,
                                        int32_t flip_h, int32_t flip_v, float quality, uint8_t* d_out,
                                        size_t out_cap, uint64_t* d_offsets, uint32_t* d_lengths,
                                        int32_t* d_status);
/*
 * Thumbnails as JPEG files: omr_render_scaled_batch_device into a context buffer, then
 * omr_encode_jpeg_batch_device's pipeline on the n_tiles out_w x out_h images (out_w, out_h <=
 * 4096).  Files, offsets, lengths and statuses exactly as omr_render_jpeg_batch_device.
 * Asynchronous on the context stream.
 */
omr_status omr_render_thumbnail_jpeg_batch_device(omr_ctx* ctx, const omr_quantum_def* qdef,
                                                  const omr_channel_binding* channels, int32_t size_c,
                                                  const void* const* d_plane_ptrs, int32_t n_tiles,
                                                  int64_t row_stride, int32_t pixel_type, int32_t big_endian,
                                                  int32_t width, int32_t height, int32_t flip_h, int32_t flip_v,
                                                  int32_t out_w, int32_t out_h, float quality, uint8_t* d_out,
                                                  size_t out_cap, uint64_t* d_offsets, uint32_t* d_lengths,
                                                  int32_t* d_status);
/* Same, host output: files packed in out (cap bytes), offsets/lengths host arrays; synchronous. */
omr_status omr_encode_jpeg_batch(omr_ctx* ctx, const uint32_t* d_argb, int64_t tile_stride_px,
                                 int32_t n_tiles, int32_t width, int32_t height, float quality,
                                 uint8_t* out, size_t cap, uint64_t* offsets, uint32_t* lengths);
/* Java ImageIO quality -> quantisation tables (natural order), JPEGQTable.getScaledInstance. */
omr_status omr_jpeg_quant_tables(float quality, uint8_t luma[64], uint8_t chroma[64]);
/* Same under OMR_SEM_* flags (OMR_SEM_JPEG_CHROMA_DIV2 selects the chroma base table). */
omr_status omr_jpeg_quant_tables_sem(float quality, uint32_t semantics, uint8_t luma[64], uint8_t chroma[64]);

/* PNG RGB8 of ARGB pixels (ImageIO.write(image, "png"), ImageRegionRequestHandler.java:598). */
omr_status omr_encode_png(omr_ctx* ctx, const uint32_t* argb, int32_t width, int32_t height,
                          uint8_t* out, size_t cap, size_t* out_len);
omr_status omr_encode_png_device(omr_ctx* ctx, const uint32_t* d_argb, int32_t width,
                                 int32_t height, uint8_t* out, size_t cap, size_t* out_len);
/*
 * Batched PNG (same encoder family, decoded pixels identical per tile) of n_tiles device ARGB
 * tiles (tile i at d_argb + i*tile_stride_px; 0 = width*height): the batch form of the
 * per-request ImageIO.write(image, "png", ...) calls (ImageRegionRequestHandler.java:597-599).
 * Complete PNG files in d_out (capacity out_cap bytes): file i at d_out + d_offsets[i] (16-byte
 * aligned slots, in tile order), d_lengths[i] bytes; 0 and d_status[i] = OMR_BUFFER_TOO_SMALL when
 * it did not fit (d_offsets / d_lengths / d_status optional).  Every stage is one launch over all
 * tiles; no host sync (asynchronous on the context stream).  width, height <= 4096.
 */
omr_status omr_encode_png_batch_device(omr_ctx* ctx, const uint32_t* d_argb, int64_t tile_stride_px,
                                       int32_t n_tiles, int32_t width, int32_t height, uint8_t* d_out,
                                       size_t out_cap, uint64_t* d_offsets, uint32_t* d_lengths,
                                       int32_t* d_status);
/* Output capacity that always holds n batched PNG files of width x height (channels 3: RGB
 * tiles, 1: masks), 16-byte slots included. */
size_t omr_png_batch_max_bytes(int32_t width, int32_t height, int32_t channels, int32_t n);

/* ---- raw pixel tiles (K12) ---------------------------------------------------- */
/*
 * The pixel values themselves, not a rendering: the /tile/<image>/<z>/<c>/<t>?x=&y=&w=&h=&
 * resolution=&format=png|tif request of the OMERO pixel-buffer microservice.  The rules are this
 * library's own:
 *  - PNG: greyscale (colour type 0), bit depth 8 for OMR_PIXELS_INT8 / UINT8 and 16 for INT16 /
 *    UINT16, samples big-endian as PNG demands (a native-order plane is swapped on the device).
 *    Signed types keep their bit patterns: the file of an int16 plane holds the same bytes as the
 *    file of the uint16 plane with those bits, which is what a Java TYPE_USHORT_GRAY raster of the
 *    same bytes holds; a client that knows the pixel type reinterprets them.  PNG has no 32-bit
 *    integer, float or double sample: those types are OMR_INVALID_ARGUMENT here, TIFF carries them.
 *  - The encoder is the batched PNG pipeline (same filter heuristic, deflate and file layout as
 *    omr_encode_png_batch_device); the filter stage reads the region's rows in place from the
 *    plane with the plane's pitch, so a row band or a level view needs no repacking.
 *  - Two calls with the same input return identical bytes.
 *
 * omr_encode_png_gray_batch_device: tile i is the width x height region at (x, y) of the device
 * plane d_plane (its first pixel; rows pitch_px pixels apart, pitch_px >= x + width; a 16-bit
 * plane at an even address).  n files packed in d_out as omr_encode_png_batch_device packs them
 * (16-byte slots in tile order, d_offsets / d_lengths / d_status optional, OMR_BUFFER_TOO_SMALL
 * and length 0 for a file that did not fit).  Asynchronous on the context stream, no host sync.
 * OMR_INVALID_ARGUMENT (nothing launched): a pixel type PNG cannot hold, width / height outside
 * 1..4096, n < 0, a null table or plane, pitch_px < x + width, a negative x or y, an odd 16-bit
 * plane address.  n == 0 is OMR_OK and launches nothing.
 * A context created with OMR_PNG_GRAY_WAVE=0 in the environment filters every batch with the
 * workgroup kernel (the reference route of the tests); by default a uniform batch of whole-dword
 * rows of at most 4096 bytes that all start on 16-byte boundaries takes the wave kernel, which
 * omr_ctx_kernel_timings reports as kind 27 (the other PNG stages: 20 filter, 21 parse, 22 tables,
 * 23 encode, 24 meta + offsets, 25 emit, 26 CRC).  Both give the same bytes.
 */
typedef struct omr_raw_tile {
    const void* d_plane;
    int64_t pitch_px;
    int32_t x, y;
} omr_raw_tile;
/* Output capacity that always holds n grey PNG files of width x height (stored blocks, chunks and
 * the 16-byte slots included); 0 for n <= 0 or a size / sample width no file has. */
size_t omr_png_gray_batch_max_bytes(int32_t width, int32_t height, int32_t bytes_per_sample, int32_t n);
omr_status omr_encode_png_gray_batch_device(omr_ctx* ctx, const omr_raw_tile* tiles, int32_t n,
                                            int32_t pixel_type, int32_t big_endian, int32_t width,
                                            int32_t height, uint8_t* d_out, size_t out_cap,
                                            uint64_t* d_offsets, uint32_t* d_lengths, int32_t* d_status);
/*
 * Host-fed: n tiles (z, c, t, x, y) of one pixel buffer or level view, all width x height, read
 * through the pixel-buffer staging (the registered mapping's DMA, or pinned slots) and encoded in
 * one batch.  Host out, synchronous: file i at out + offsets[i], lengths[i] bytes, status[i].  A
 * tile outside the image (the omr_pixel_buffer_get_tile rule) fails alone with
 * OMR_INVALID_ARGUMENT in status[i] and length 0; the call still returns OMR_OK.
 * n * omr_png_gray_batch_max_bytes(width, height, bytes per sample, 1) always suffices.
 */
typedef struct omr_raw_tile_request {
    int32_t z, c, t, x, y;
} omr_raw_tile_request;
omr_status omr_pixel_buffer_tiles_png(omr_ctx* ctx, const omr_pixel_buffer* pb,
                                      const omr_raw_tile_request* reqs, int32_t n, int32_t width,
                                      int32_t height, uint8_t* out, size_t cap, uint64_t* offsets,
                                      uint32_t* lengths, int32_t* status);

/*
 * TIFF of the 24-bit RGB view (TIFFImageWriter branch, ImageRegionRequestHandler.java:584-596):
 * baseline uncompressed big-endian RGB, 8-bit samples, >= 8 KiB strips.  Host writer.
 */
size_t omr_tiff_max_bytes(int32_t width, int32_t height);
omr_status omr_encode_tiff(omr_ctx* ctx, const uint32_t* argb, int32_t width, int32_t height,
                           uint8_t* out, size_t cap, size_t* out_len);
omr_status omr_encode_tiff_device(omr_ctx* ctx, const uint32_t* d_argb, int32_t width,
                                  int32_t height, uint8_t* out, size_t cap, size_t* out_len);
/*
 * Raw TIFF (K12, host writer): the pixels of one plane region in their own type -- baseline,
 * uncompressed, big-endian ("MM"), one sample per pixel, BitsPerSample 8 / 16 / 32 / 64,
 * SampleFormat 1 (unsigned) / 2 (signed) / 3 (IEEE), PhotometricInterpretation BlackIsZero, whole
 * rows per strip and every strip but the last at least 8 KiB.  All eight OMR_PIXELS_* types;
 * native-order input (big_endian = 0) is swapped.  width, height <= 65535 and a file below 4 GiB,
 * else OMR_INVALID_ARGUMENT (omr_tiff_raw_max_bytes: 0).  *out_len receives the file's length also
 * with OMR_BUFFER_TOO_SMALL.  omr_pixel_buffer_tile_tiff reads the tile as
 * omr_pixel_buffer_get_tile does (same bounds rule; w, h >= 1) and writes it.
 */
size_t omr_tiff_raw_max_bytes(int32_t width, int32_t height, int32_t pixel_type);
omr_status omr_encode_tiff_raw(const void* pixels, int32_t pixel_type, int32_t big_endian,
                               int32_t width, int32_t height, uint8_t* out, size_t cap, size_t* out_len);
omr_status omr_pixel_buffer_tile_tiff(const omr_pixel_buffer* pb, int32_t z, int32_t c, int32_t t,
                                      int32_t x, int32_t y, int32_t w, int32_t h, uint8_t* out,
                                      size_t cap, size_t* out_len);

/* ---- shape mask ------------------------------------------------------------- */
/*
 * ShapeMaskRequestHandler.renderShapeMask(Color, byte[], w, h) (:165-207): MSB-first bit mask
 * (no row padding) -> flip -> 2-entry palette PNG (index 0 transparent, index 1 = rgba).
 * width % 8 == 0 with a flip follows the reference's packed-buffer flip unless the context has
 * OMR_SEM_MASK_PIXEL_FLIP (see there).  Every exception the reference raises inside
 * renderShapeMask (a null or short mask, a zero size, the packed-buffer flip's
 * ArrayIndexOutOfBoundsException, width*height past Java int) completes its future exceptionally,
 * which ShapeMaskVerticle.java:119-128 answers with 404: OMR_NOT_FOUND.  A null rgba or out is
 * OMR_INVALID_ARGUMENT.  Host in/out.
 */
omr_status omr_render_shape_mask_png(omr_ctx* ctx, const uint8_t* bits, size_t n_bytes,
                                     int32_t width, int32_t height, const uint8_t rgba[4],
                                     int32_t flip_h, int32_t flip_v,
                                     uint8_t* out, size_t cap, size_t* out_len);
/*
 * N render_shape_mask requests in one call (the per-worker renderShapeMask calls of
 * ShapeMaskVerticle.java:121-149 coalesced): the masks may differ in size, colour and flips, and
 * are encoded by the batched PNG pipeline (one launch per stage for all of them).  Host in/out,
 * synchronous.  File i lands at out + offsets[i] (16-byte aligned slots), lengths[i] bytes;
 * status[i] is OMR_OK, OMR_NOT_FOUND for every case the single call answers with 404 (the same
 * checks and the same packed-buffer flip), or OMR_BUFFER_TOO_SMALL when cap ran out
 * (omr_png_batch_max_bytes(w, h, 1, 1) per mask always suffices).  Returns OMR_OK when the call
 * ran; per-mask outcomes are in status.
 */
typedef struct omr_mask_job {
    const uint8_t* bits;        /* MSB-first mask bits (byte[] of the Mask) */
    size_t n_bytes;
    int32_t width, height;
    uint8_t rgba[4];            /* fill colour (omr_shape_mask_fill_color) */
    int32_t flip_h, flip_v;
} omr_mask_job;
omr_status omr_render_shape_mask_png_batch(omr_ctx* ctx, const omr_mask_job* jobs, int32_t n,
                                           uint8_t* out, size_t cap, uint64_t* offsets,
                                           uint32_t* lengths, int32_t* status);

/* ---- host-side request helpers (no device work) ---------------------------------- */
/* ImageRegionRequestHandler.splitHTMLColor (:865-890), bug-compatible; OMR_INVALID_ARGUMENT = null. */
omr_status omr_split_html_color(const char* color, int32_t rgba_out[4]);
/* ShapeMaskRequestHandler.renderShapeMask(Mask) fill colour (:97-106).  OMR_INVALID_ARGUMENT where the
 * reference throws (NPE on an unparsable colour, Color's IAE); inside renderShapeMask that fails the
 * future, which the verticle answers with 404 (ShapeMaskVerticle.java:119-128). */
omr_status omr_shape_mask_fill_color(int32_t has_mask_fill, int32_t mask_fill_color,
                                     const char* request_color, uint8_t rgba_out[4]);
/*
 * getRegionDef + truncateRegionDef + flipRegionDef (ImageRegionRequestHandler.java:789-832,
 * :751-758, :770-780).  mode: 0 = tile (tile.x/y in tile units, width/height 0 = use
 * tile_size_*), 1 = region (pixels), 2 = neither (full plane).  level_sizes holds
 * n_levels (sizeX,sizeY) pairs; resolution < 0 means "not given" (0).
 */
omr_status omr_get_region_def(int32_t mode, const omr_region* request, int32_t resolution,
                              const int32_t* level_sizes, int32_t n_levels,
                              int32_t tile_size_x, int32_t tile_size_y, int32_t max_tile_length,
                              int32_t flip_h, int32_t flip_v, omr_region* out);
/* setResolutionLevel (:840-853): Renderer level = nLevels - resolution - 1. */
int32_t omr_resolution_level(int32_t n_levels, int32_t resolution);
/* checkPlaneDef (:651-681): truncate region to the level size. */
omr_status omr_check_plane_def(omr_region* region, int32_t size_x, int32_t size_y);
/* LutReader: parse an ImageJ .lut file image (768 B binary, 800 B with header, or text). */
omr_status omr_parse_lut(const uint8_t* data, size_t n, uint8_t lut_out[768]);

/* ---- request decode + renderer settings (omr_request.cpp; host only) -------------------- */
#define OMR_MAX_REQUEST_CHANNELS 64
/* per-channel entry of omr_image_region_ctx.map_reverse (the `maps` JSON list) */
enum { OMR_MAP_NONE = 0, OMR_MAP_REVERSE = 1, OMR_MAP_NULL = 2, OMR_MAP_BAD = 3 };

/*
 * ImageRegionCtx (ImageRegionCtx.java:44-109) after assignParams (:127-153).  has_* / -1 encode
 * Java nulls.  windows are the Float values (:313-314); colors[i] is the raw `$...` string
 * (HTML colour or a *.lut name).
 */
typedef struct omr_image_region_ctx {
    int64_t image_id;
    int32_t z, t;
    int32_t has_tile;          /* tile: x/y in tile units, width/height 0 for the short form */
    omr_region tile;
    int32_t has_resolution, resolution;
    int32_t has_region;
    omr_region region;
    int32_t n_channels;        /* -1: no 'c' parameter (channels == null) */
    int32_t channels[OMR_MAX_REQUEST_CHANNELS];      /* signed 1-based, negative = inactive */
    int32_t window_set[OMR_MAX_REQUEST_CHANNELS];    /* 0: Float[2]{null,null} */
    float windows[OMR_MAX_REQUEST_CHANNELS][2];
    int32_t color_set[OMR_MAX_REQUEST_CHANNELS];     /* 0: colour null */
    char colors[OMR_MAX_REQUEST_CHANNELS][64];
    int32_t model;             /* -1 null, OMR_MODEL_GREYSCALE ("g"), OMR_MODEL_RGB ("c") */
    int32_t has_quality;
    float quality;
    int32_t inverted_axis;     /* -1 null, 0/1 (parsed, unused, :93-97) */
    int32_t projection;        /* -1 null, OMR_PROJECTION_* */
    int32_t has_projection_start, projection_start;
    int32_t has_projection_end, projection_end;
    int32_t n_maps;            /* -1: no `maps` parameter */
    int32_t map_reverse[OMR_MAX_REQUEST_CHANNELS];   /* OMR_MAP_* per list element */
    int32_t flip_h, flip_v;
    char format[16];           /* default "jpeg" */
    char cache_key[17];        /* Guava sipHash24 hex of the sorted parameters (:165-177) */
} omr_image_region_ctx;

/* ShapeMaskCtx (ShapeMaskCtx.java:38-81). */
typedef struct omr_shape_mask_ctx {
    int64_t shape_id;
    int32_t has_color;
    char color[64];
    int32_t flip_h, flip_v;
    char cache_key[128];       /* "ome.model.roi.Mask:<id>:<color>" (:77-81) */
} omr_shape_mask_ctx;

/*
 * new ImageRegionCtx(params, key) (ImageRegionCtx.java:122-153).  names/values: the request's
 * MultiMap entries in insertion order (case-insensitive names, first value wins).
 * OMR_INVALID_ARGUMENT = IllegalArgumentException (400); OMR_INTERNAL = an unchecked exception
 * the reference does not catch (500).  err (optional) receives the message.
 */
omr_status omr_image_region_ctx_parse(const char* const* names, const char* const* values, int32_t n,
                                      omr_image_region_ctx* out, char* err, size_t err_cap);
/* new ShapeMaskCtx(params, key) (ShapeMaskCtx.java:61-72); bad shapeId -> OMR_INTERNAL (500). */
omr_status omr_shape_mask_ctx_parse(const char* const* names, const char* const* values, int32_t n,
                                    omr_shape_mask_ctx* out, char* err, size_t err_cap);

/* LutProviderImpl (LutProviderImpl.java:29-75): *.lut files under root, keyed by basename. */
typedef struct omr_lut_provider omr_lut_provider;
omr_status     omr_lut_provider_create(const char* root, omr_lut_provider** out);
void           omr_lut_provider_destroy(omr_lut_provider* p);
int32_t        omr_lut_provider_count(const omr_lut_provider* p);
omr_status     omr_lut_provider_add(omr_lut_provider* p, const char* name, const uint8_t lut_rgb768[768]);
/* 768-byte R[256] G[256] B[256] table owned by the provider, or NULL (getLutReaders -> null). */
const uint8_t* omr_lut_provider_get(const omr_lut_provider* p, const char* name);

/* createRenderingDef (ImageRegionRequestHandler.java:258-300) for size_c channels. */
omr_status omr_create_rendering_def(int32_t pixel_type, int32_t size_c, omr_quantum_def* qdef,
                                    omr_channel_binding* channels);
/*
 * updateSettings (ImageRegionRequestHandler.java:689-741) applied to a rendering def: active
 * flags, windows, colours or LUTs (luts may be NULL), reverse-intensity maps, model.
 * Reference failures (null channels / window / colour / model, short lists, bad maps entries)
 * return OMR_INTERNAL (500).
 */
omr_status omr_update_settings(const omr_image_region_ctx* ctx, int32_t size_c, omr_quantum_def* qdef,
                               omr_channel_binding* channels, const omr_lut_provider* luts,
                               char* err, size_t err_cap);

/* ---- tiled TIFF / OME-TIFF pixel data, LZW decoded on the device (K13) ------------------- */
/*
 * The second backend of PixelsService.getPixelBuffer: pyramidal OME-TIFF
 * as raw2ometiff writes it -- one IFD per plane in the main chain, the lower resolutions in each
 * IFD's SubIFDs (tag 330).  The TIFF image is a type of its own beside omr_pixel_buffer; what it
 * reads feeds the device-level render and encode calls by composition.
 *
 * Supported: classic TIFF and BigTIFF in either byte order; one sample per pixel; BitsPerSample
 * 8 / 16 / 32 / 64 with SampleFormat 1 / 2 / 3 (the eight OMR_PIXELS_* types); tiles or strips (a
 * strip is a full-width segment); Compression 1 (none) and 5 (LZW); Predictor 1, and 2 for 8-, 16-
 * and 32-bit samples; FillOrder 1; a segment with byte count 0 reads as zeros.  All planes have the
 * same size, type, compression, segment geometry and level count.  OME-XML is not parsed: the
 * caller gives Z, C, T and the dimension order (one of the six OME orders, "XYZCT" being the ROMIO
 * order), and plane (z, c, t) is the main-chain IFD at the index the order gives.
 *
 * open: OMR_NOT_FOUND for a missing file; OMR_INVALID_ARGUMENT for anything unsupported (another
 * compression, predictor 3, predictor 2 with 64-bit samples, several samples per pixel, FillOrder
 * 2, fewer IFDs than Z*C*T, planes that disagree, a segment above 256 MiB decoded); OMR_INTERNAL
 * for a corrupt file (an offset or count past the end of the file, an IFD chain that loops, a
 * count whose product overflows).  The file is read with pread, every offset bounds-checked.
 * Read-only; safe to share between contexts and threads.  Deflate, zstd, Predictor 3 and chunky
 * multi-sample files open through omr_tiff_image_open_ex below.
 */
typedef struct omr_tiff_image omr_tiff_image;
typedef struct omr_tiff_info {
    int32_t size_x, size_y, size_z, size_c, size_t_;   /* level 0 */
    int32_t pixel_type;                                /* OMR_PIXELS_* */
    int32_t big_endian;                                /* the file's byte order ("MM": 1) */
    int32_t n_levels;                                  /* 1 + SubIFDs per plane */
    int32_t compression, predictor;                    /* TIFF tag values: 1 / 5, 1 / 2; open_ex: also 8 / 50000 (32946 reads 8), 3 */
    int32_t tiled;                                     /* level 0: 1 tiles, 0 strips */
    int32_t segment_width, segment_height;             /* level 0: tile size, or size_x and RowsPerStrip */
    int32_t big_tiff;
} omr_tiff_info;
omr_status omr_tiff_image_open(const char* path, int32_t size_z, int32_t size_c, int32_t size_t_,
                               const char* dimension_order, omr_tiff_image** out);
/*
 * omr_tiff_image_open with the set of further forms the caller accepts; omr_tiff_image_open(...) is
 * open_ex with opt == NULL, which means accept = 0 and refuses them all as before.
 * OMR_INVALID_ARGUMENT: unknown bits in accept, a struct_size smaller than the struct, a form the
 * file uses whose bit is not set.
 *
 * DEFLATE and ZSTD: every segment is one zlib stream (Compression 8, or 32946, reported as 8) or one
 * Zstandard frame (50000), decoded on the host by omr_inflate_host / omr_zstd_decode_host and on the
 * device by K14a / K16a (kernel timing kinds 32 / 35 in place of 30).  Their rule is the strict one of the Zarr
 * reader, not LZW's rule of cutting an overrunning string: a segment must decode to exactly its
 * size, through the Adler-32 or the frame's end, and anything else is OMR_INTERNAL on that segment.
 * A compressed segment stays below 512 MiB.  Pinned against libtiff's own Deflate and zstd strips
 * (tests/golden/tiff_codecs.npz: 8- and 16-bit, Predictor 1 and 2, a short last strip).
 *
 * PREDICTOR3: the floating-point predictor, float and double samples, one sample per pixel
 * (libtiff's fpAcc): the running byte sum (mod 256) over a segment row's n * B bytes gives B planes
 * of n bytes, the most significant byte of every sample first in either file byte order; sample x
 * is the planes' bytes at x.  float32 little-endian is pinned against libtiff; double and the
 * big-endian forms rest on the project's own writer.
 *
 * SAMPLES: SamplesPerPixel 2..4 with PlanarConfiguration 1 (chunky, as brightfield RGB slides are
 * written).  size_c stays the channel count as OMERO sees it (3 for an RGB image) and must be a
 * multiple of SamplesPerPixel; the file holds Z * (C / spp) * T IFDs and channel c is sample c % spp
 * of the IFD of channel c / spp, in the caller's dimension order; info.size_c is the caller's.
 * ExtraSamples are ordinary channels.  All samples of a pixel have the same BitsPerSample and
 * SampleFormat; Predictor 2 runs per component, spp samples apart.  A read returns the one
 * requested sample; on the device two channels of one pixel share the segment, which is read and
 * decoded once per group.  Refused: Photometric 6 (YCbCr, but for JPEG segments: OMR_TIFF_ACCEPT_JPEG), PlanarConfiguration 2, more than 4
 * samples, Predictor 3.  The segment limit of 256 MiB decoded counts all samples.  8-bit RGB is
 * pinned against libtiff; 16-bit, 4 samples and big-endian rest on the project's own writer.
 */
#define OMR_TIFF_ACCEPT_DEFLATE    1u   /* Compression 8 and 32946: one zlib stream per segment   */
#define OMR_TIFF_ACCEPT_ZSTD       2u   /* Compression 50000: one Zstandard frame per segment     */
#define OMR_TIFF_ACCEPT_PREDICTOR3 4u   /* floating-point predictor, float and double samples     */
#define OMR_TIFF_ACCEPT_SAMPLES    8u   /* SamplesPerPixel 2..4, PlanarConfiguration 1 (chunky)   */
/* (16: OMR_TIFF_ACCEPT_JPEG, K17; 32: OMR_TIFF_ACCEPT_JPEG2000, K19; 64: OMR_TIFF_ACCEPT_JPEG2000_LOSSY, K20 -- all further down) */
typedef struct omr_tiff_open_options {
    uint32_t struct_size;                              /* sizeof(omr_tiff_open_options) */
    uint32_t accept;                                   /* OMR_TIFF_ACCEPT_* bits */
} omr_tiff_open_options;
omr_status omr_tiff_image_open_ex(const char* path, int32_t size_z, int32_t size_c, int32_t size_t_,
                                  const char* dimension_order, const omr_tiff_open_options* opt,
                                  omr_tiff_image** out);
/* SamplesPerPixel of the open image (1 unless opened with OMR_TIFF_ACCEPT_SAMPLES); negative status for NULL. */
int32_t    omr_tiff_image_samples_per_pixel(const omr_tiff_image* img);
void       omr_tiff_image_close(omr_tiff_image* img);
omr_status omr_tiff_image_info(const omr_tiff_image* img, omr_tiff_info* info);
/* (width, height) per level as stored in the file (not size >> k): up to cap_pairs pairs into
 * sizes_out; returns the level count, or -OMR_INVALID_ARGUMENT. */
int32_t    omr_tiff_image_level_sizes(const omr_tiff_image* img, int32_t* sizes_out, int32_t cap_pairs);
/*
 * The host route (no GPU): the bounds rule and packed rows of omr_pixel_buffer_get_tile at
 * resolution `level`, bytes in the file's byte order, decoded with a plain serial LZW decoder.
 * The reference the device route is tested against, and the route of single reads.  TIFF LZW as
 * libtiff reads it: MSB-first codes from 9 bits, 256 Clear, 257 EOI, first entry 258, early change
 * (10 bits once the next free entry is 511, 11 at 1023, 12 at 2047).  Decoding ends at EOI or once
 * the segment's size (tile_w * tile_h * bpp, or rows_in_strip * W * bpp) is produced; a string
 * that overruns it is cut.  OMR_INTERNAL: fewer bytes than that, a code above the next free entry,
 * an old-style LSB-first stream, an I/O error.  Deflate and zstd segments (open_ex) go through
 * omr_inflate_host / omr_zstd_decode_host by the strict rule stated there: exactly the segment's
 * size, nothing cut.  Predictor 3 and the per-component Predictor 2 are undone here, and for a
 * chunky image the rows hold the one sample of channel c.
 */
omr_status omr_tiff_image_get_tile(const omr_tiff_image* img, int32_t level, int32_t z, int32_t c, int32_t t,
                                   int32_t x, int32_t y, int32_t w, int32_t h, void* dst, size_t cap);
/* The host decoder alone: one stream into exactly `expected` bytes (OMR_OK / OMR_INTERNAL). */
omr_status omr_lzw_decode_host(const uint8_t* src, size_t length, uint8_t* dst, size_t expected);
/*
 * K13a alone: n independent TIFF LZW streams, stream i at d_src + d_offsets[i], d_lengths[i] bytes
 * (below 512 MiB), decoded into d_dst + d_dst_offsets[i], at most d_expected[i] bytes (below 1 GiB;
 * nothing is written behind them); d_status[i] = OMR_OK or OMR_INTERNAL (the cases of the host
 * decoder), one segment's failure leaving the others alone.  All tables in device memory.
 * Asynchronous on the context stream; omr_ctx_kernel_timings reports kind 30.
 */
omr_status omr_lzw_decode_batch_device(omr_ctx* ctx, const uint8_t* d_src, const uint64_t* d_offsets,
                                       const uint32_t* d_lengths, const uint32_t* d_expected, int32_t n,
                                       uint8_t* d_dst, const uint64_t* d_dst_offsets, int32_t* d_status);
/*
 * n regions of one level, all width x height: region i = reqs[i] (z, c, t, x, y; the get_tile
 * bounds rule, else OMR_INVALID_ARGUMENT and nothing is read) lands at d_dst + i *
 * region_stride_bytes (a multiple of the sample size, at least width * height * bpp; d_dst aligned
 * to the sample size) as height rows of width pixels in the file's byte order.  The host lists the
 * segments the regions touch -- one needed by several requests is read and decoded once -- preads
 * their compressed bytes into pinned staging and sends them in one copy with the segment table;
 * K13a decodes the LZW segments into scratch (kind 30), K13b undoes predictor 2, crops and stores
 * (kind 31); uncompressed segments go through K13b from the uploaded bytes.  Large calls are
 * worked off in groups.  Synchronous; OMR_INTERNAL when a segment is corrupt.
 */
omr_status omr_tiff_image_read_regions_device(omr_ctx* ctx, const omr_tiff_image* img, int32_t level,
                                              const omr_raw_tile_request* reqs, int32_t n, int32_t width,
                                              int32_t height, void* d_dst, int64_t region_stride_bytes);
/*
 * omr_render_pixel_buffer_tiles for a TIFF image level: the active channels' regions are read as
 * [tile][channel][h][w] (16-byte aligned strides) and rendered by
 * omr_render_batch_strided_device with the file's byte order.  size_c must be the image's.
 */
omr_status omr_render_tiff_tiles(omr_ctx* ctx, const omr_tiff_image* img, int32_t level,
                                 const omr_quantum_def* qdef, const omr_channel_binding* channels,
                                 int32_t size_c, const omr_tile_request* reqs, int32_t n, int32_t width,
                                 int32_t height, int32_t flip_h, int32_t flip_v, uint32_t* argb_out,
                                 int32_t out_on_device);

/* ---- OME-Zarr pyramids, zlib chunks inflated on the device (K14) -------------------------- */
/*
 * The third backend of PixelsService.getPixelBuffer: OME-Zarr as bioformats2raw writes it -- a
 * Zarr v2 directory per image (series), one 5-D TCZYX array per resolution, one file per chunk.
 * group_path is the image group (".../image.zarr/0").  Its .zattrs multiscales[0].datasets[*].path
 * lists the levels in order; without multiscales the levels are the sub-directories 0, 1, ... that
 * hold a .zarray.  axes, when present, must name t, c, z, y, x in that order.  Z, C and T come from
 * the array shape; OME-XML is not read.
 *
 * Supported per array: zarr_format 2, order "C", a 5-D shape with chunks [1, 1, 1, ch, cw], dtype
 * |u1 |i1 <u2 >u2 <i2 >i2 <u4 >u4 <i4 >i4 <f4 >f4 <f8 >f8 (the eight OMR_PIXELS_* types), filters
 * null, compressor null or {"id": "zlib"}, fill_value 0 / 0.0 / null, dimension_separator "." (the
 * default) or "/".  All levels have the same dtype, compressor and Z, C, T; level sizes are as the
 * arrays state them.  Edge chunks are stored whole (ch * cw * bpp bytes decoded); a chunk file that
 * does not exist reads as zeros.
 *
 * open: OMR_NOT_FOUND when the group directory or its first .zarray is missing;
 * OMR_INVALID_ARGUMENT for anything unsupported (another compressor id, any filter, order "F", not
 * five dimensions, a chunk deeper than 1 in t, c or z, a non-zero fill, another dtype, zarr_format
 * 3, levels that disagree, a chunk above 256 MiB decoded); OMR_INTERNAL for corrupt input (JSON
 * that does not parse, a shape or chunk that is not a positive integer or whose product
 * overflows).  Read-only; safe to share between contexts and threads.
 */
typedef struct omr_zarr_image omr_zarr_image;
typedef struct omr_zarr_info {
    int32_t size_x, size_y, size_z, size_c, size_t_;   /* level 0 */
    int32_t pixel_type;                                /* OMR_PIXELS_* */
    int32_t big_endian;                                /* the arrays' byte order (">": 1) */
    int32_t n_levels;
    int32_t compression;                               /* 0 none, 1 zlib, 2 Blosc, 3 zstd (open_ex only) */
    int32_t chunk_width, chunk_height;                 /* level 0 */
    int32_t dimension_separator;                       /* '.' or '/' */
} omr_zarr_info;
omr_status omr_zarr_image_open(const char* group_path, omr_zarr_image** out);
void       omr_zarr_image_close(omr_zarr_image* img);
omr_status omr_zarr_image_info(const omr_zarr_image* img, omr_zarr_info* info);
/* As omr_tiff_image_level_sizes. */
int32_t    omr_zarr_image_level_sizes(const omr_zarr_image* img, int32_t* sizes_out, int32_t cap_pairs);
/*
 * The host route (no GPU): the bounds rule and packed rows of omr_tiff_image_get_tile, bytes in
 * the array's byte order, zlib chunks decoded by omr_inflate_host.  OMR_INTERNAL: an uncompressed
 * chunk file whose size is not ch * cw * bpp, a bad zlib stream, an I/O error.
 */
omr_status omr_zarr_image_get_tile(const omr_zarr_image* img, int32_t level, int32_t z, int32_t c, int32_t t,
                                   int32_t x, int32_t y, int32_t w, int32_t h, void* dst, size_t cap);
/*
 * The host decoder alone, a plain serial one (nothing links libz): an RFC 1950 stream -- header
 * with CM = 8, CINFO <= 7, a good FCHECK and no FDICT -- of RFC 1951 blocks of all three types.
 * OMR_OK only when the stream yields exactly `expected` bytes, then the end-of-block of a final
 * block, then the Adler-32 of those bytes; anything else is OMR_INTERNAL (unlike the LZW rule of
 * cutting an overrunning string: a Zarr chunk's size is known exactly).  Bytes behind the Adler-32
 * are not looked at.
 */
omr_status omr_inflate_host(const uint8_t* src, size_t length, uint8_t* dst, size_t expected);
/*
 * K14a alone: n independent zlib streams, the table layout of omr_lzw_decode_batch_device (streams
 * below 512 MiB, d_expected[i] at most 256 MiB; nothing is written behind d_dst + d_dst_offsets[i]
 * + d_expected[i]); d_status[i] = OMR_OK or OMR_INTERNAL by the rule of omr_inflate_host, one
 * stream's failure leaving the others alone.  Asynchronous on the context stream;
 * omr_ctx_kernel_timings reports kind 32.
 */
omr_status omr_inflate_batch_device(omr_ctx* ctx, const uint8_t* d_src, const uint64_t* d_offsets,
                                    const uint32_t* d_lengths, const uint32_t* d_expected, int32_t n,
                                    uint8_t* d_dst, const uint64_t* d_dst_offsets, int32_t* d_status);
/*
 * The contract of omr_tiff_image_read_regions_device for a Zarr level: the host lists the chunks
 * the regions touch, each once per group, reads the chunk files into pinned staging on up to 16
 * threads and sends bytes and tables in one copy; K14a inflates into scratch (kind 32) and K13b
 * (predictor 1, kind 31) crops and stores; uncompressed chunks skip K14a, missing chunks store
 * zeros.  Synchronous; OMR_INTERNAL when a chunk is corrupt.
 */
omr_status omr_zarr_image_read_regions_device(omr_ctx* ctx, const omr_zarr_image* img, int32_t level,
                                              const omr_raw_tile_request* reqs, int32_t n, int32_t width,
                                              int32_t height, void* d_dst, int64_t region_stride_bytes);
/* omr_render_tiff_tiles for a Zarr image level. */
omr_status omr_render_zarr_tiles(omr_ctx* ctx, const omr_zarr_image* img, int32_t level,
                                 const omr_quantum_def* qdef, const omr_channel_binding* channels,
                                 int32_t size_c, const omr_tile_request* reqs, int32_t n, int32_t width,
                                 int32_t height, int32_t flip_h, int32_t flip_v, uint32_t* argb_out,
                                 int32_t out_on_device);

/* ---- Blosc OME-Zarr chunks, LZ4 blocks decoded on the device (K15) -------------------------- */
/*
 * omr_zarr_image_open_ex is omr_zarr_image_open with the set of chunk codecs the caller accepts:
 * omr_zarr_image_open(path, out) is open_ex with codecs = OMR_ZARR_CODEC_ZLIB, and opt == NULL
 * means the same.  OMR_INVALID_ARGUMENT: unknown bits in codecs, a struct_size smaller than the
 * struct, a codec named in .zarray but not in codecs.  With OMR_ZARR_CODEC_BLOSC the compressor
 * {"id": "blosc", "cname": "lz4" | "lz4hc", "shuffle": 0 | 1} is accepted (bioformats2raw's
 * default); "shuffle": -1 only for types wider than one byte (on a one-byte type numcodecs reads
 * it as bit-shuffle); clevel and blocksize are ignored.  Any other cname (blosclz, zstd, zlib,
 * snappy) and "shuffle": 2 are OMR_INVALID_ARGUMENT.  Every other rule of omr_zarr_image_open
 * holds.  On a Blosc image omr_zarr_info.compression reads 2, and omr_zarr_image_get_tile,
 * omr_zarr_image_read_regions_device and omr_render_zarr_tiles work unchanged: on the device route
 * the host checks each chunk's container (OMR_INTERNAL before any launch) and lists its streams,
 * K15a decodes the LZ4 streams and copies the stored ones into scratch (kind 33) and K15b crops
 * with the byte un-shuffle folded into its loads (kind 34); memcpyed chunks are placed from the
 * uploaded bytes, missing chunks store zeros.
 *
 * The Blosc 1 container as read here (as recalled, not pinned against c-blosc): a 16-byte header
 * -- version 2, codec version, flags, typesize, int32 LE nbytes, blocksize, cbytes -- with flags
 * 0x01 byte shuffle, 0x02 memcpyed, 0x04 bit shuffle (refused), 0x10 do not split, bits 5-7 the
 * compressor format (1 = LZ4 / LZ4HC, any other refused); then int32 bstarts[ceil(nbytes /
 * blocksize)]; a block is typesize splits when 0x10 is clear, typesize <= 16, blocksize / typesize
 * >= 128 and it is not the leftover block, else one; a split is int32 csize and csize bytes,
 * csize == its decoded size meaning stored raw.  The decoder follows the header's typesize.  The
 * splits listed, with their csize words, may not add up to more than the bytes behind the table,
 * and a chunk of more than 2^20 splits is refused (OMR_INTERNAL).
 */
#define OMR_ZARR_CODEC_ZLIB  1u
#define OMR_ZARR_CODEC_BLOSC 2u
typedef struct omr_zarr_open_options {
    uint32_t struct_size;                              /* sizeof(omr_zarr_open_options) */
    uint32_t codecs;                                   /* OMR_ZARR_CODEC_* bits */
} omr_zarr_open_options;
omr_status omr_zarr_image_open_ex(const char* group_path, const omr_zarr_open_options* opt, omr_zarr_image** out);
/*
 * One LZ4 block, serial (nothing links liblz4): sequences of a token (high nibble the literal
 * length, low nibble the match length minus 4, a nibble of 15 extended by bytes until one is not
 * 255), the literals, a 2-byte LE offset and the match, which may overlap its own output.  The
 * block ends only right after a literal run (possibly empty) that consumes the last input byte.
 * OMR_OK only when exactly `expected` bytes were produced at that point; OMR_INTERNAL for offset
 * 0, an offset beyond the bytes produced, literals or an extension running past the input, output
 * past `expected`, input that ends after a match or inside a sequence, too few or too many bytes.
 */
omr_status omr_lz4_decode_host(const uint8_t* src, size_t length, uint8_t* dst, size_t expected);
/* One Blosc 1 chunk (the container above) into exactly `expected` bytes, un-shuffled; OMR_INTERNAL
 * for anything the container rules or omr_lz4_decode_host refuse. */
omr_status omr_blosc_decode_host(const uint8_t* src, size_t length, uint8_t* dst, size_t expected);
/*
 * K15a alone: n independent LZ4 blocks, the table layout and limits of omr_inflate_batch_device;
 * d_status[i] = OMR_OK or OMR_INTERNAL by the rule of omr_lz4_decode_host, one stream's failure
 * leaving the others alone, nothing written behind d_dst + d_dst_offsets[i] + d_expected[i].
 * Asynchronous on the context stream; omr_ctx_kernel_timings reports kind 33.
 */
omr_status omr_lz4_decode_batch_device(omr_ctx* ctx, const uint8_t* d_src, const uint64_t* d_offsets,
                                       const uint32_t* d_lengths, const uint32_t* d_expected, int32_t n,
                                       uint8_t* d_dst, const uint64_t* d_dst_offsets, int32_t* d_status);

/* ---- Blosc-Zstd and zstd OME-Zarr chunks, frames decoded on the device (K16) ---------------- */
/*
 * Two more codec bits of omr_zarr_open_options.codecs.  OMR_ZARR_CODEC_BLOSC_ZSTD accepts
 * {"id": "blosc", "cname": "zstd"} under the shuffle rules of OMR_ZARR_CODEC_BLOSC (which alone
 * still refuses a zstd group); OMR_ZARR_CODEC_ZSTD accepts the bare {"id": "zstd"} codec of
 * numcodecs and tensorstore, whose level and checksum entries are ignored.  Bit 4u is not a codec:
 * it stays unknown and OMR_INVALID_ARGUMENT.  A Blosc image remembers which inner formats its open
 * allowed (1 = LZ4 with OMR_ZARR_CODEC_BLOSC, 4 = Zstd with OMR_ZARR_CODEC_BLOSC_ZSTD); a chunk
 * whose header names another is a corrupt chunk.  omr_zarr_info.compression reads 2 for Blosc with
 * either inner codec and 3 for bare zstd.  On the device route the Zstd streams of Blosc chunks and
 * the chunks of a zstd image are decoded by K16a (kind 35) and placed by K15b (34) or K13b (31).
 *
 * A stream is exactly one Zstandard frame (RFC 8878; pinned against libzstd 1.4.8): magic
 * 0xFD2FB528; single-segment or with a window descriptor (window log up to 31, as libzstd); Frame_Content_Size
 * absent or of 1, 2, 4 or 8 bytes and then equal to `expected`; raw, RLE and compressed blocks no
 * larger than the smaller of the window and 128 KiB; literals raw, RLE, Huffman (direct or
 * FSE-compressed weights, code lengths up to 11, one or four streams, each consumed exactly) and
 * treeless; sequence tables predefined, RLE, FSE-compressed (accuracy logs up to 9, 8, 9; offset
 * codes up to 31) and repeat, the backward bit stream consumed exactly; repeat offsets 1, 4, 8;
 * matches may reach into earlier blocks and overlap their own output; the content checksum (the
 * low 32 bits of XXH64, seed 0), when flagged, is verified.  OMR_INTERNAL: anything else -- a
 * skippable or second frame, trailing bytes, a dictionary id other than 0, a reserved bit, block
 * type 3, a treeless or repeat form without a table from an earlier block of the frame, an offset
 * beyond the bytes produced, and any output other than exactly `expected` bytes.  Blosc's format
 * number 4 for Zstd, one frame per split, is as recalled, not pinned against c-blosc.
 */
#define OMR_ZARR_CODEC_BLOSC_ZSTD 8u
#define OMR_ZARR_CODEC_ZSTD       16u
/* One frame into exactly `expected` bytes, serial (nothing links libzstd). */
omr_status omr_zstd_decode_host(const uint8_t* src, size_t length, uint8_t* dst, size_t expected);
/*
 * Walks a frame as the decoder does (the frame must be good; its size is taken from the frame, up
 * to 256 MiB) and sets one bit per form met in forms[0 .. OMR_ZSTD_FORM_WORDS): form f is bit
 * f & 31 of word f >> 5.  The tests use it to prove that their fixture reaches every branch.
 */
#define OMR_ZSTD_FORM_WORDS 2
enum {
    OMR_ZSTD_FORM_BLOCK_RAW = 0, OMR_ZSTD_FORM_BLOCK_RLE, OMR_ZSTD_FORM_BLOCK_COMPRESSED,
    OMR_ZSTD_FORM_LIT_RAW, OMR_ZSTD_FORM_LIT_RLE, OMR_ZSTD_FORM_LIT_HUFFMAN, OMR_ZSTD_FORM_LIT_TREELESS,
    OMR_ZSTD_FORM_STREAMS_1, OMR_ZSTD_FORM_STREAMS_4,
    OMR_ZSTD_FORM_WEIGHTS_DIRECT, OMR_ZSTD_FORM_WEIGHTS_FSE,
    OMR_ZSTD_FORM_SEQ_ZERO, OMR_ZSTD_FORM_SEQ_SHORT, OMR_ZSTD_FORM_SEQ_2BYTE, OMR_ZSTD_FORM_SEQ_3BYTE,
    OMR_ZSTD_FORM_LL_PREDEFINED, OMR_ZSTD_FORM_LL_RLE, OMR_ZSTD_FORM_LL_FSE, OMR_ZSTD_FORM_LL_REPEAT,
    OMR_ZSTD_FORM_OF_PREDEFINED, OMR_ZSTD_FORM_OF_RLE, OMR_ZSTD_FORM_OF_FSE, OMR_ZSTD_FORM_OF_REPEAT,
    OMR_ZSTD_FORM_ML_PREDEFINED, OMR_ZSTD_FORM_ML_RLE, OMR_ZSTD_FORM_ML_FSE, OMR_ZSTD_FORM_ML_REPEAT,
    OMR_ZSTD_FORM_SINGLE_SEGMENT, OMR_ZSTD_FORM_WINDOWED,
    OMR_ZSTD_FORM_FCS_ABSENT, OMR_ZSTD_FORM_FCS_1, OMR_ZSTD_FORM_FCS_2, OMR_ZSTD_FORM_FCS_4, OMR_ZSTD_FORM_FCS_8,
    OMR_ZSTD_FORM_CHECKSUM, OMR_ZSTD_FORM_MULTI_BLOCK,
    OMR_ZSTD_FORM_COUNT
};
omr_status omr_zstd_frame_forms(const uint8_t* src, size_t length, uint32_t* forms);
/*
 * omr_blosc_decode_host with the set of inner codecs accepted: OMR_BLOSC_INNER_LZ4 takes the
 * header's compressor format 1, OMR_BLOSC_INNER_ZSTD format 4 (each split one Zstandard frame).
 * omr_blosc_decode_host itself is inner = OMR_BLOSC_INNER_LZ4.  OMR_INVALID_ARGUMENT: no bit, or
 * an unknown one.
 */
#define OMR_BLOSC_INNER_LZ4  1u
#define OMR_BLOSC_INNER_ZSTD 2u
omr_status omr_blosc_decode_host_ex(const uint8_t* src, size_t length, uint8_t* dst, size_t expected, uint32_t inner);
/*
 * K16a alone: n independent Zstandard frames, the table layout and limits of
 * omr_inflate_batch_device; d_status[i] = OMR_OK or OMR_INTERNAL by the rule of
 * omr_zstd_decode_host, one stream's failure leaving the others alone, nothing written behind
 * d_dst + d_dst_offsets[i] + d_expected[i].  Asynchronous on the context stream;
 * omr_ctx_kernel_timings reports kind 35.
 */
omr_status omr_zstd_decode_batch_device(omr_ctx* ctx, const uint8_t* d_src, const uint64_t* d_offsets,
                                        const uint32_t* d_lengths, const uint32_t* d_expected, int32_t n,
                                        uint8_t* d_dst, const uint64_t* d_dst_offsets, int32_t* d_status);

/* ---- K17: JPEG-compressed TIFF segments (Compression 7) ---------------------------------------
 *
 * OMR_TIFF_ACCEPT_JPEG in omr_tiff_image_open_ex admits Compression 7 ("new-style" JPEG: every
 * segment one interchange or abbreviated stream, the shared tables in tag 347, JPEGTables, read at
 * open and bounded to 64 KiB); omr_tiff_image_open and Compression 6 keep refusing.  Accepted:
 * BitsPerSample 8, SampleFormat 1, Predictor 1, tiles or strips, and SamplesPerPixel 1 with
 * Photometric 0 or 1, or SamplesPerPixel 3 (which needs OMR_TIFF_ACCEPT_SAMPLES as well) with
 * Photometric 2 (the components are R, G, B) or 6 (YCbCr -> RGB on decode, as libtiff's
 * JPEGCOLORMODE_RGB).  The frame header, not the YCbCrSubSampling tag, decides the sampling.
 * The image then behaves as a chunky 8-bit one: get_tile, read_regions_device and
 * omr_render_tiff_tiles return the one sample of channel c, and a segment is decoded once per call.
 *
 * The decoder: baseline sequential DCT (SOF0), 8 bits, Huffman, all components in one interleaved
 * scan, luma sampled 1x1, 2x1 or 2x2 over 1x1 chroma; DQT with 8-bit entries, up to 4 + 4 + 4
 * tables, several per marker segment; a segment's own DQT / DHT override tag 347's for that segment;
 * DRI with RST0..7 in order; APPn and COM skipped (JFIF and Adobe markers do not matter: the
 * TIFF's Photometric decides the colour); fill FF bytes before a marker.  Arithmetic as
 * libjpeg(-turbo)'s defaults, byte for byte: the islow IDCT, the "fancy" triangle upsampling (plain
 * replication where the chroma is at most two samples wide), jdcolor's 16-bit YCbCr conversion
 * (tests/golden/tiff_jpeg.npz pins them against libtiff and libjpeg-turbo).
 * OMR_INVALID_ARGUMENT, the reason naming the form: SOF1/2/3/5+ (extended, progressive, lossless,
 * hierarchical, arithmetic), 12-bit samples, 16-bit quantisation entries, DNL, more than one scan,
 * four components, any other sampling.  OMR_INTERNAL (damage; stricter than libjpeg, which pads
 * with zeros and warns): a stream cut short, bits missing at the end of a restart interval, a code
 * that is not in the table, a coefficient index past 63, a DC category above 11, an AC category
 * above 10, a DC value outside [-2048, 2047], a missing, surplus or out-of-order RST, no EOI,
 * frame dimensions other than the segment's (the rows of a last strip), a table referenced but
 * never defined.
 */
#define OMR_TIFF_ACCEPT_JPEG 16u   /* Compression 7: one baseline JPEG stream per segment */
/*
 * The host decoder alone (get_tile's): tables (NULL or a JPEGTables stream: SOI, DQT / DHT, EOI)
 * and one segment's stream, whose frame must be width x height with `samples` (1 or 3) components;
 * chunky width * height * samples bytes to dst (at most 256 MiB), with ycbcr != 0 converted to RGB.
 * why (optional, why_cap bytes): the reason of a failure as text.
 */
omr_status omr_jpeg_decode_host(const uint8_t* tables, size_t tables_length, const uint8_t* src, size_t length,
                                int32_t width, int32_t height, int32_t samples, int32_t ycbcr, uint8_t* dst,
                                char* why, size_t why_cap);
/*
 * Decodes a good stream's entropy-coded data (its size and component count from its own frame
 * header) and sets bit f of *forms for every form met.  The tests use it to prove that their
 * fixture reaches every branch.
 */
enum {
    OMR_JPEG_FORM_EOB_EARLY = 0,   /* EOB before coefficient 63 */
    OMR_JPEG_FORM_FULL_BLOCK,      /* a block that reaches coefficient 63 */
    OMR_JPEG_FORM_ZRL,
    OMR_JPEG_FORM_LONG_CODE,       /* a code of 12 bits or more */
    OMR_JPEG_FORM_DC_CAT9,         /* a DC category >= 9 */
    OMR_JPEG_FORM_STUFFED_FF,      /* FF 00 */
    OMR_JPEG_FORM_RESTART,         /* a restart marker */
    OMR_JPEG_FORM_PAD_BITS,        /* pad bits before a marker */
    OMR_JPEG_FORM_TABLE_OVERRIDE,  /* a table of the segment that overrides one of JPEGTables */
    OMR_JPEG_FORM_MULTI_TABLE,     /* several tables in one DQT or DHT */
    OMR_JPEG_FORM_COM,
    OMR_JPEG_FORM_FILL_BYTES,      /* FF fill bytes before a marker */
    OMR_JPEG_FORM_TABLES_STREAM,   /* decoded with a JPEGTables stream */
    OMR_JPEG_FORM_COUNT
};
omr_status omr_jpeg_stream_forms(const uint8_t* tables, size_t tables_length, const uint8_t* src, size_t length,
                                 uint32_t* forms);
/*
 * K17 alone: n streams in HOST memory (the headers are parsed and the restart intervals listed on
 * the host, as in omr_tiff_image_read_regions_device), stream i = lengths[i] bytes at src +
 * offsets[i] with a frame of widths[i] x heights[i] and `samples` components, all sharing `tables`
 * (may be NULL), decoded on the device into d_dst + dst_offsets[i] as chunky widths[i] * heights[i] *
 * samples bytes (nothing is written behind them).  offsets, lengths, widths, heights, dst_offsets
 * and status are host arrays; status[i] = OMR_OK, OMR_INVALID_ARGUMENT or OMR_INTERNAL by the rule of
 * omr_jpeg_decode_host, one stream's failure leaving the others alone.  Synchronous.
 * omr_ctx_kernel_timings reports kinds 36 (K17a, entropy decode), 37 (K17b, IDCT) and 38 (K17c,
 * upsample, colour and store); omr_tiff_image_read_regions_device on a JPEG image reports them in
 * front of 31.
 */
omr_status omr_jpeg_decode_batch_device(omr_ctx* ctx, const uint8_t* tables, size_t tables_length, const uint8_t* src,
                                        const uint64_t* offsets, const uint32_t* lengths, const int32_t* widths,
                                        const int32_t* heights, int32_t n, int32_t samples, int32_t ycbcr,
                                        uint8_t* d_dst, const uint64_t* dst_offsets, int32_t* status);
/*
 * K18: the entropy decode of a long restart interval spread over a workgroup.  K17a gives an
 * interval to one wave and walks its symbol chain serially, which is slow for a stream without
 * restart markers (one interval per tile).  K18a cuts the interval into subsequences of
 * subsequence_bits bits and decodes it by the self-synchronising parallel Huffman decode
 * (Weissenberger and Schmidt, "Massively Parallel Huffman Decoding on GPUs", ICPP 2018, and
 * "Accelerating JPEG Decompression on GPUs", 2021): one workgroup of 256 lanes per interval, one
 * lane per subsequence from a guessed state, lanes adopting their predecessor's exit state until
 * nothing changes, then a pass that writes the coefficients; K18b turns the DC differences into
 * values.  K17b and K17c follow unchanged, and the pixels and statuses are K17's.
 *
 * OFF BY DEFAULT: a context that never makes this call launches what it launched before.  With
 * min_interval_bytes != 0 every interval of at least that many entropy-coded bytes (and fewer than
 * 128 MiB) takes K18, the others K17a; one call may launch both.  The setting applies to
 * omr_jpeg_decode_batch_device, omr_tiff_image_read_regions_device and omr_render_tiff_tiles.
 * opt == NULL: off.  OMR_INVALID_ARGUMENT: a struct_size below the struct's, or subsequence_bits
 * that is neither 0 nor a multiple of 32 in [32, 4096].
 * omr_ctx_kernel_timings reports kind 39 for K18a and 40 for K18b, in front of 37 and 38 (and
 * behind 36 when the call launches K17a too).
 */
typedef struct omr_jpeg_split_options {
    uint32_t struct_size;
    uint32_t min_interval_bytes;   /* 0: off (the default). An interval of at least this many bytes takes K18 */
    uint32_t subsequence_bits;     /* 0: the library's default (1024); else a multiple of 32 in [32, 4096] */
} omr_jpeg_split_options;
omr_status omr_ctx_set_jpeg_split(omr_ctx* ctx, const omr_jpeg_split_options* opt);   /* NULL: off */
/*
 * omr_jpeg_decode_host with the entropy decode done the way K18 does it, by the same per-lane
 * functions (csrc/omr_jpegdec.h): plain loops play a workgroup of `lanes` lanes (1..256) through
 * the rounds of K18a -- guess, settle, scan, write -- and then K18b's DC sums.  The statuses are
 * omr_jpeg_decode_host's, and on OMR_OK so are the bytes.  OMR_INVALID_ARGUMENT also for
 * subsequence_bits that is no multiple of 32 in [32, 4096] and lanes outside [1, 256].
 * stats (required) says what the decode met, summed over the stream's intervals: the subsequences,
 * the most rounds (of `lanes` subsequences) any interval took, the most settle iterations any round
 * took before no lane changed, and the lane decodes repeated from an adopted state.
 */
typedef struct omr_jpeg_split_stats {
    uint32_t subsequences, rounds, max_settle_iterations, redecodes;
} omr_jpeg_split_stats;
omr_status omr_jpeg_decode_host_split(const uint8_t* tables, size_t tables_length, const uint8_t* src, size_t length,
                                      int32_t width, int32_t height, int32_t samples, int32_t ycbcr,
                                      uint32_t subsequence_bits, uint32_t lanes, uint8_t* dst,
                                      omr_jpeg_split_stats* stats);

/* ---- K19: JPEG 2000 TIFF segments (Compression 33003, 33004, 33005, 34712), the reversible path ----
 *
 * OMR_TIFF_ACCEPT_JPEG2000 in omr_tiff_image_open_ex admits Compression 33003, 33004 and 33005
 * (Aperio's and Bio-Formats' numbers, as recalled) and 34712 (the registered one): every segment is
 * one raw JPEG 2000 codestream that starts with SOC (FF 4F).  omr_tiff_image_open and an open_ex
 * without the bit refuse them as before.  TIFF forms: Predictor 1, SampleFormat 1, tiles or strips,
 * BitsPerSample 8 with SamplesPerPixel 1 (Photometric 0 or 1) or 3 (Photometric 2; needs
 * OMR_TIFF_ACCEPT_SAMPLES), or BitsPerSample 16 with SamplesPerPixel 1.  The image then behaves like
 * a Deflate file of the same sample type (info.compression reads 34712 for all four numbers):
 * get_tile decodes on the host, read_regions_device and omr_render_tiff_tiles on the device, a
 * segment once per call, 16-bit samples stored in the file's byte order.
 *
 * Codestream forms accepted: one tile that covers the image, one tile-part, image and tile offsets
 * 0; 1 or 3 unsigned components of a precision equal to BitsPerSample, no subsampling; the
 * reversible 5/3 transform with QCD style 0 (no quantisation), and the reversible colour transform
 * when COD's MCT byte is 1; 0..32 decomposition levels; code-blocks of 4..1024 a side and at most
 * 4096 samples; user precincts; 1..65535 quality layers; the progression orders LRCP, RLCP, RPCL,
 * PCRL, CPRL; COM (and TLM, PLM, PLT, CRG) skipped; at most 30 magnitude bit-planes per subband
 * (guard bits + exponent - 1).  A stream truncated by its encoder (fewer coding passes than its
 * bit-planes hold) is reconstructed at the mid-point of what is left open, as OpenJPEG does
 * (csrc/omr_j2kdec.h states the rule).  Pinned byte for byte against OpenJPEG, through Pillow, by
 * tests/golden/tiff_j2k.npz.
 *
 * OMR_INVALID_ARGUMENT, the message naming the form: the irreversible 9/7 transform and
 * quantisation styles 1 and 2 (K20, further down, takes them behind switches of its own); any
 * code-block style bit (bypass, reset, termination on each pass,
 * vertically causal, predictable termination, segmentation symbols); SOP or EPH; COC, QCC, RGN,
 * POC, PPM, PPT; several tiles or tile-parts; non-zero offsets; subsampled or signed components; a
 * precision other than 8 or 16; a JP2 box wrapper; 16-bit with three samples.  OMR_INTERNAL
 * (damage): a stream cut inside a marker segment or a packet header, a packet body that runs past
 * the tile-part, more coding passes than 3 * (M_b - zero bit-planes) - 2, more zero bit-planes than
 * M_b, a frame size other than the segment's, no EOC.  A damaged packet BODY cannot be detected
 * without the termination styles that are refused: it decodes to defined, in-bounds garbage with
 * OMR_OK, the same garbage on the host and on the device.
 */
#define OMR_TIFF_ACCEPT_JPEG2000 32u   /* Compression 33003, 33004, 33005, 34712: one reversible JPEG 2000 codestream per segment */
/*
 * The host decoder alone (get_tile's): src a raw codestream whose frame must be width x height
 * with `samples` components (1 or 3) of `bits` bits (8 or 16; 16 with one sample only), decoded to
 * dst as chunky samples, 16-bit ones in the host's byte order (dst then 2-byte aligned).  Code-blocks
 * go to 16 threads from 65536 samples on.  why (may be NULL): the reason of a failure, cut to why_cap.
 */
omr_status omr_j2k_decode_host(const uint8_t* src, size_t length, int32_t width, int32_t height, int32_t samples,
                               int32_t bits, uint8_t* dst, char* why, size_t why_cap);
/* The coding forms a good stream uses, bit f of *forms for form f: what the fixture is measured by. */
enum {
    OMR_J2K_FORM_ZC0 = 0,          /* .. 8: the nine zero-coding contexts */
    OMR_J2K_FORM_SC9 = 9,          /* sign context 9 (it has no flip) */
    OMR_J2K_FORM_SC10 = 10,        /* .. 17: sign contexts 10..13, each without (even bit) and with the XOR flip */
    OMR_J2K_FORM_MR14 = 18,        /* .. 20: the refinement contexts 14, 15, 16 */
    OMR_J2K_FORM_RUN_TAKEN = 21,   /* a run of four zeros coded as one decision */
    OMR_J2K_FORM_RUN_BROKEN = 22,  /* a run broken, its place by the UNIFORM context */
    OMR_J2K_FORM_MPS_EXCHANGE = 23,
    OMR_J2K_FORM_LPS_EXCHANGE = 24,
    OMR_J2K_FORM_FF_BODY = 25,     /* an FF byte inside a code-block's bytes */
    OMR_J2K_FORM_FF_HEADER = 26,   /* an FF byte (and its stuffed bit) inside a packet header */
    OMR_J2K_FORM_PASSES_1 = 27,    /* the pass-count codewords: 1, 2, 3..5, 6..36, 37..164 */
    OMR_J2K_FORM_PASSES_2,
    OMR_J2K_FORM_PASSES_3_5,
    OMR_J2K_FORM_PASSES_6_36,
    OMR_J2K_FORM_PASSES_37_164,
    OMR_J2K_FORM_LBLOCK,           /* an Lblock increment */
    OMR_J2K_FORM_TAG_TREE_DEEP,    /* a tag tree of more than one level */
    OMR_J2K_FORM_LATE_INCLUSION,   /* a code-block absent from the first layer and included later */
    OMR_J2K_FORM_ZERO_BIT_PLANES,  /* a code-block with missing bit-planes */
    OMR_J2K_FORM_PARTIAL_BLOCK,    /* a code-block cut by its subband's or precinct's edge */
    OMR_J2K_FORM_RCT,
    OMR_J2K_FORM_BITS16,
    OMR_J2K_FORM_COUNT
};
omr_status omr_j2k_stream_forms(const uint8_t* src, size_t length, uint64_t* forms);
/*
 * K19 alone: n codestreams in HOST memory (headers and packets are walked on the host, as in
 * omr_tiff_image_read_regions_device), stream i = lengths[i] bytes at src + offsets[i] with a frame
 * of widths[i] x heights[i], `samples` components and `bits` bits, decoded on the device into d_dst
 * + dst_offsets[i] as chunky samples (16-bit ones little-endian, dst_offsets then even; nothing is
 * written behind them).  The arrays and status are host arrays; status[i] = OMR_OK,
 * OMR_INVALID_ARGUMENT or OMR_INTERNAL by the rule of omr_j2k_decode_host, one stream's failure
 * leaving the others alone.  Synchronous.  omr_ctx_kernel_timings reports kind 41 (K19a, one launch:
 * the code-blocks), 42 (K19b, one launch per decomposition level of the deepest stream) and 43
 * (K19c, one launch: colour, level shift, clamp, store); omr_tiff_image_read_regions_device on a
 * JPEG 2000 image reports them in front of 31.
 */
omr_status omr_j2k_decode_batch_device(omr_ctx* ctx, const uint8_t* src, const uint64_t* offsets, const uint32_t* lengths,
                                       const int32_t* widths, const int32_t* heights, int32_t n, int32_t samples,
                                       int32_t bits, uint8_t* d_dst, const uint64_t* dst_offsets, int32_t* status);

/* ---- K20: JPEG 2000 TIFF segments, the irreversible path ("JPEG-2000 Lossy") ----
 *
 * OMR_TIFF_ACCEPT_JPEG2000_LOSSY in omr_tiff_image_open_ex admits the same four Compression
 * numbers with segments coded by the irreversible 9/7 transform.  It implies nothing: 32 | 64 reads
 * both kinds (the transform is a property of a segment, and one file may mix them), 64 alone opens
 * the file and refuses a reversible segment by name when it is read, as 32 alone goes on refusing
 * an irreversible one ("j2k: the irreversible 9/7 transform").  Compression 33003's components are
 * passed through as stored, as K19 does; Aperio's YCbCr reading of that number is out of scope.
 *
 * Codestream forms: K19's, with the transform byte 0 (9/7), QCD style 1 (scalar derived: one
 * exponent and mantissa, the other subbands' exponents derived from it) or 2 (scalar expounded:
 * one pair per subband), and COD's MCT byte 1 meaning the irreversible colour transform.
 * OMR_INVALID_ARGUMENT by name in addition to K19's list: 9/7 with QCD style 0, and 5/3 with style
 * 1 or 2.
 *
 * Arithmetic (csrc/omr_j2kdec.h): float32 in a fixed order without contraction, the same functions
 * on the host and on the device, so the two routes give the same bytes.  The reference is OpenJPEG
 * 2.5.4: step = 0.5f * float((1 + mantissa / 2048) * 2^(precision - exponent)), coefficient =
 * (float)(signed value with its fractional bit) * step; per level all rows, then all columns: the
 * low-pass samples times 1.230174105f, the high-pass ones times 1.625732422f, then four lifting
 * steps a + (left + right) * c with c = -0.443506852f (even places), -0.882911075f (odd),
 * 0.052980118f (even), 1.586134342f (odd) and whole-sample symmetric extension, a line of one
 * sample untouched; r = y + v * 1.402f, g = y - u * 0.34413f - v * 0.71414f, b = y + u * 1.772f;
 * round to nearest, ties to even; add 2^(bits - 1); clamp.  tests/golden/tiff_j2k97.npz holds
 * OpenJPEG's pixels and, per stream, the number of samples where the host decoder differs from
 * them (by 1 at most).
 */
#define OMR_TIFF_ACCEPT_JPEG2000_LOSSY 64u   /* the same Compression numbers: irreversible (9/7) JPEG 2000 codestreams */
#define OMR_J2K_ALLOW_IRREVERSIBLE 1u        /* flags of the _ex calls: take 9/7 streams as well as 5/3 ones */
/* omr_j2k_decode_host with flags (0: the same call). */
omr_status omr_j2k_decode_host_ex(const uint8_t* src, size_t length, int32_t width, int32_t height, int32_t samples,
                                  int32_t bits, uint32_t flags, uint8_t* dst, char* why, size_t why_cap);
/* What an irreversible stream shows beyond the OMR_J2K_FORM_* bits (bit f of *lossy_forms; 0 for a reversible stream). */
enum {
    OMR_J2K_LOSSY_FORM_W97 = 0,          /* the 9/7 transform */
    OMR_J2K_LOSSY_FORM_QCD_EXPOUNDED,    /* QCD style 2 */
    OMR_J2K_LOSSY_FORM_QCD_DERIVED,      /* QCD style 1 */
    OMR_J2K_LOSSY_FORM_ICT,              /* three components with the irreversible colour transform */
    OMR_J2K_LOSSY_FORM_NO_MCT_3,         /* three components without a transform */
    OMR_J2K_LOSSY_FORM_TRUNCATED_BLOCK,  /* a code-block with fewer coding passes than its bit-planes allow */
    OMR_J2K_LOSSY_FORM_LINE_OF_1,        /* a lifted line of one sample (it passes through) */
    OMR_J2K_LOSSY_FORM_LINE_OF_2,        /* a lifted line of two samples */
    OMR_J2K_LOSSY_FORM_BITS16,
    OMR_J2K_LOSSY_FORM_COUNT
};
/* omr_j2k_stream_forms with flags; lossy_forms may be NULL. */
omr_status omr_j2k_stream_forms_ex(const uint8_t* src, size_t length, uint32_t flags, uint64_t* forms, uint32_t* lossy_forms);
/*
 * omr_j2k_decode_batch_device with flags.  Reversible and irreversible streams may share a call:
 * per level K19b (kind 42) runs for the reversible ones and K20b (kind 44, k_j2k_idwt97: one
 * workgroup per 64 x 32 output tile of a level, staged in LDS with a halo of four samples) for the
 * irreversible ones, neither when it has no stream; K19a and K19c serve both.
 */
omr_status omr_j2k_decode_batch_device_ex(omr_ctx* ctx, const uint8_t* src, const uint64_t* offsets, const uint32_t* lengths,
                                          const int32_t* widths, const int32_t* heights, int32_t n, int32_t samples,
                                          int32_t bits, uint32_t flags, uint8_t* d_dst, const uint64_t* dst_offsets,
                                          int32_t* status);

#ifdef __cplusplus
}
#endif
#endif /* OMR_OMR_H */
