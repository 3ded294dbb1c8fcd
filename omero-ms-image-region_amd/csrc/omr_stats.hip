// omr_stats.hip — K9: plane statistics (min / max / NaN count) and histograms on the device.
//
// What webgateway/histogram_json serves and what fills omr_channel_binding.global_min/global_max
// (OMERO's StatsInfo).  The reference snapshot has no histogram code; the binning rule is this
// project's (include/omr/omr.h, omr_histogram_bin_of) and the device reproduces it for every
// pixel: 8- and 16-bit types through a value -> bin table the host builds with that very
// function and a workgroup stages in LDS, the other types by evaluating the rule in fp64 (IEEE
// subtraction and division, one rounding each; the library is built with -ffp-contract=off).
//
// Both kernels read a region of up to 32 planes once, in 16-byte units: a workgroup covers a
// tile of (rows x units) of the region, a lane whose unit lies wholly inside its row loads it as
// one vector, and a lane on a row's ragged head or tail reads its pixels one by one.
#include "omr_device.h"

#include <cstdlib>
#include <limits>
#include <type_traits>

namespace omr {

constexpr int kMaxStatPlanes = 32;
constexpr int kStatBlock = 256;          // threads per workgroup of the statistics and evaluating kernels
constexpr int kTab16Block = 1024;        // ... of the 16-bit table histogram (its LDS allows 1-2 per CU)
// 16-byte loads a lane issues before it consumes them.  Measured (CHANGELOG.md): the statistics
// kernel is level from 2 to 8; the histogram loses time with every load it waits for before its
// LDS work starts (1 and 2 level, 4 12% slower, 8 50%).  Compile-time A/B switches.
#ifndef OMR_K9_STAT_DEPTH
#define OMR_K9_STAT_DEPTH 4
#endif
#ifndef OMR_K9_HIST_DEPTH
#define OMR_K9_HIST_DEPTH 2
#endif
#ifndef OMR_K9_STAT_BPC
#define OMR_K9_STAT_BPC 8
#endif
constexpr int kStatDepth = OMR_K9_STAT_DEPTH, kHistDepth = OMR_K9_HIST_DEPTH;
constexpr int kStatBlocksPerCu = OMR_K9_STAT_BPC;   // workgroups of a statistics launch per CU (guideline: 8)

#define OMR_GLOBAL_AS __attribute__((address_space(1)))
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct Geom {
    const uint8_t* planes[kMaxStatPlanes];
    int64_t org;          // bytes from a plane's start to the region's first pixel
    int64_t pitch;        // bytes between the starts of two region rows
    int64_t row_bytes;    // bytes of one region row
    uint32_t rows;        // region rows (1 when the region is one contiguous run of pixels)
    uint32_t lw_log2;     // a workgroup's tile: (blockDim >> lw_log2) rows x (1 << lw_log2) units
    uint32_t unit_blocks; // tiles along a row
    uint32_t tiles;       // tiles of the region
};

template <typename T> struct RawOf;
template <> struct RawOf<int8_t> { using U = uint8_t; };
template <> struct RawOf<uint8_t> { using U = uint8_t; };
template <> struct RawOf<int16_t> { using U = uint16_t; };
template <> struct RawOf<uint16_t> { using U = uint16_t; };
template <> struct RawOf<int32_t> { using U = uint32_t; };
template <> struct RawOf<uint32_t> { using U = uint32_t; };
template <> struct RawOf<float> { using U = uint32_t; };
template <> struct RawOf<double> { using U = uint64_t; };

template <typename T, bool BE>
__device__ __forceinline__ T px_from_raw(typename RawOf<T>::U u) {
    using U = typename RawOf<T>::U;
    if constexpr (BE && sizeof(U) == 2) u = (U)(((u & 0xFFu) << 8) | (u >> 8));
    else if constexpr (BE && sizeof(U) == 4) u = bswap32(u);
    else if constexpr (BE && sizeof(U) == 8) u = ((uint64_t)bswap32((uint32_t)u) << 32) | bswap32((uint32_t)(u >> 32));
    T t;
    __builtin_memcpy(&t, &u, sizeof(T));
    return t;
}

// One lane's share of a tile: n = -1 a whole 16-byte unit (in q), n > 0 that many pixels at p
// (a row's head or tail), n = 0 nothing.
struct Unit {
    u32x4 q;
    const uint8_t* p;
    int32_t n;
};

template <int BPP>
__device__ __forceinline__ Unit fetch_unit(const Geom& G, const uint8_t* plane, uint64_t tile) {
    Unit u;
    u.q = u32x4{0u, 0u, 0u, 0u};
    u.p = nullptr;
    u.n = 0;
    if (tile >= G.tiles) return u;
    const uint32_t t = (uint32_t)tile;
    const uint32_t rb = t / G.unit_blocks, ub = t - rb * G.unit_blocks;
    const uint32_t lw = 1u << G.lw_log2;
    const uint32_t row = rb * (blockDim.x >> G.lw_log2) + (threadIdx.x >> G.lw_log2);
    if (row >= G.rows) return u;
    const uint64_t unit = (uint64_t)ub * lw + (threadIdx.x & (lw - 1));
    const uintptr_t s = reinterpret_cast<uintptr_t>(plane) + (uintptr_t)(G.org + (int64_t)row * G.pitch);
    const uintptr_t e = s + (uintptr_t)G.row_bytes;
    const uintptr_t a = (s & ~(uintptr_t)15) + unit * 16;
    if (a >= e) return u;
    if (a >= s && a + 16 <= e) {
        u.q = __builtin_nontemporal_load(reinterpret_cast<const OMR_GLOBAL_AS u32x4*>(a));   // read once
        u.n = -1;
        return u;
    }
    const uintptr_t b0 = a > s ? a : s, b1 = a + 16 < e ? a + 16 : e;   // pixel-aligned: s is, and BPP divides 16
    u.p = reinterpret_cast<const uint8_t*>(b0);
    u.n = (int32_t)((b1 - b0) / BPP);
    return u;
}

template <typename T, bool BE, typename F>
__device__ __forceinline__ void for_each_px(const Unit& u, F&& f) {
    using U = typename RawOf<T>::U;
    constexpr int V = 16 / (int)sizeof(T);
    if (u.n < 0) {
        U a[V];
        __builtin_memcpy(&a[0], &u.q, 16);
#pragma unroll
        for (int j = 0; j < V; ++j) f(px_from_raw<T, BE>(a[j]));
    } else {
        for (int j = 0; j < u.n; ++j) f(px_from_raw<T, BE>(ld_global<U>(u.p + (size_t)j * sizeof(T))));
    }
}

// Every pixel of plane blockIdx.y's region that this workgroup owns, DEPTH tiles at a time.
template <typename T, bool BE, int DEPTH, typename FU>
__device__ __forceinline__ void walk_region(const Geom& G, FU&& on_unit) {
    const uint8_t* plane = G.planes[blockIdx.y];
    const uint64_t step = gridDim.x;
    for (uint64_t t0 = blockIdx.x; t0 < G.tiles; t0 += step * DEPTH) {
        Unit u[DEPTH];
#pragma unroll
        for (int k = 0; k < DEPTH; ++k) u[k] = fetch_unit<(int)sizeof(T)>(G, plane, t0 + step * k);
#pragma unroll
        for (int k = 0; k < DEPTH; ++k) on_unit(u[k]);
    }
}

// ------------------------------------------------------------------------- statistics
struct StatPartial {
    double mn, mx;
    uint64_t nan;
};

__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { const double o = __shfl_xor(v, m); v = o < v ? o : v; }
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { const double o = __shfl_xor(v, m); v = o > v ? o : v; }
    return v;
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}
__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// Minimum, maximum and NaN count of the workgroup's lanes, valid in thread 0.
__device__ __forceinline__ StatPartial block_reduce(double mn, double mx, uint64_t nan) {
    __shared__ StatPartial s_w[kStatBlock / 64];
    mn = wave_min(mn);
    mx = wave_max(mx);
    nan = wave_sum64(nan);
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0) s_w[wave] = StatPartial{mn, mx, nan};
    __syncthreads();
    StatPartial r = s_w[0];
    for (uint32_t w = 1; w < blockDim.x >> 6; ++w) {
        const StatPartial o = s_w[w];
        r.mn = o.mn < r.mn ? o.mn : r.mn;
        r.mx = o.mx > r.mx ? o.mx : r.mx;
        r.nan += o.nan;
    }
    return r;
}

// One partial per workgroup: the region's extrema reduced in the pixel type per lane (16-bit types
// two at a time on their order-preserving unsigned keys), then across the wave and the workgroup.
template <typename T, bool BE>
__global__ void __launch_bounds__(kStatBlock) k_plane_minmax(Geom G, StatPartial* __restrict__ partials) {
    double dmn, dmx;
    uint32_t nan = 0;
    if constexpr (sizeof(T) == 2) {
        constexpr uint32_t kFlip = std::is_signed<T>::value ? 0x80008000u : 0u;   // int16 -> unsigned order
        uint32_t pmn = 0xFFFFFFFFu, pmx = 0u;
        walk_region<T, BE, kStatDepth>(G, [&](const Unit& u) {
            if (u.n < 0) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    uint32_t d = u.q[i];
                    if constexpr (BE) d = bswap16x2(d);
                    d ^= kFlip;
                    pmn = pk_min_u16(pmn, d);
                    pmx = pk_max_u16(pmx, d);
                }
            } else {
                for (int j = 0; j < u.n; ++j) {
                    uint32_t d = ld_global<uint16_t>(u.p + 2 * (size_t)j);
                    if constexpr (BE) d = ((d & 0xFFu) << 8) | (d >> 8);
                    d = (d | (d << 16)) ^ kFlip;
                    pmn = pk_min_u16(pmn, d);
                    pmx = pk_max_u16(pmx, d);
                }
            }
        });
        const uint32_t kmn = min(pmn & 0xFFFFu, pmn >> 16) ^ (kFlip & 0xFFFFu);
        const uint32_t kmx = max(pmx & 0xFFFFu, pmx >> 16) ^ (kFlip & 0xFFFFu);
        dmn = (double)(T)(uint16_t)kmn;
        dmx = (double)(T)(uint16_t)kmx;
        // a lane that saw no pixel: keys 0xFFFF / 0 -> neutral elements of the reduction
        if (pmn == 0xFFFFFFFFu && pmx == 0u) { dmn = INFINITY; dmx = -INFINITY; }
    } else if constexpr (std::is_floating_point<T>::value) {
        T mn = (T)INFINITY, mx = (T)-INFINITY;
        walk_region<T, BE, kStatDepth>(G, [&](const Unit& u) {
            for_each_px<T, BE>(u, [&](T v) {
                nan += v != v ? 1u : 0u;
                mn = v < mn ? v : mn;        // a NaN compares false: it takes no part
                mx = v > mx ? v : mx;
            });
        });
        dmn = (double)mn;
        dmx = (double)mx;
    } else {
        T mn = std::numeric_limits<T>::max(), mx = std::numeric_limits<T>::lowest();
        bool any = false;
        walk_region<T, BE, kStatDepth>(G, [&](const Unit& u) {
            any |= u.n != 0;
            for_each_px<T, BE>(u, [&](T v) {
                mn = v < mn ? v : mn;
                mx = v > mx ? v : mx;
            });
        });
        dmn = any ? (double)mn : (double)INFINITY;
        dmx = any ? (double)mx : (double)-INFINITY;
    }
    const StatPartial r = block_reduce(dmn, dmx, nan);
    if (threadIdx.x == 0) partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = r;
}

// One workgroup per plane folds that plane's partials: minima, maxima and integer sums, so the
// result does not depend on the order in which the workgroups finished.
__global__ void __launch_bounds__(kStatBlock) k_plane_minmax_final(const StatPartial* __restrict__ partials,
                                                                   uint32_t per_plane, uint64_t region_px,
                                                                   omr_plane_stats* __restrict__ out) {
    double mn = INFINITY, mx = -INFINITY;
    uint64_t nan = 0;
    for (uint32_t i = threadIdx.x; i < per_plane; i += kStatBlock) {
        const StatPartial p = partials[(size_t)blockIdx.x * per_plane + i];
        mn = p.mn < mn ? p.mn : mn;
        mx = p.mx > mx ? p.mx : mx;
        nan += p.nan;
    }
    const StatPartial r = block_reduce(mn, mx, nan);
    if (threadIdx.x == 0) {
        omr_plane_stats s;
        s.min = r.mn;
        s.max = r.mx;
        s.count = region_px - r.nan;
        s.nan_count = r.nan;
        out[blockIdx.x] = s;
    }
}

// -------------------------------------------------------------------------- histogram
struct HistArgs {
    Geom G;
    double lo[kMaxStatPlanes], hi[kMaxStatPlanes], bin_range[kMaxStatPlanes];
    int32_t ilo[kMaxStatPlanes], ihi[kMaxStatPlanes];   // table routes: v < lo <=> v < ilo, v > hi <=> v > ihi
    const uint8_t* table[kMaxStatPlanes];               // table routes: the plane's value -> bin table
    uint32_t* counts;                                   // [planes][n]
    unsigned long long* outside;                        // [planes][3]: below, above, NaN
    int32_t n;
    uint32_t rep_log2;                                  // log2 of the sub-histogram copies per workgroup
};

// TAB 0: the rule evaluated in fp64.  TAB 1 / 2: 8- and 16-bit types through a host-built table of
// uint8_t (n <= 256) / uint16_t entries indexed by the pixel's unsigned bits, staged in LDS.
// LDS: [n << rep_log2] 32-bit counters (bin-major: the copies of one bin sit in neighbouring
// banks, so lanes that hit the same bin spread over them), 4 outside counters, then the table.
template <typename T, bool BE, int TAB>
__global__ void __launch_bounds__(TAB != 0 && sizeof(T) == 2 ? kTab16Block : kStatBlock)
k_plane_histogram(HistArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_mem[];
    using U = typename RawOf<T>::U;
    using E = typename std::conditional<TAB == 1, uint8_t, uint16_t>::type;
    constexpr uint32_t kCodes = sizeof(T) == 1 ? 256u : 65536u;
    const uint32_t n = (uint32_t)A.n, nrep = n << A.rep_log2;
    uint32_t* s_hist = s_mem;
    uint32_t* s_out = s_mem + nrep;
    const E* s_tab = reinterpret_cast<const E*>(s_mem + ((nrep + 4 + 3) & ~3u));
    const int plane = blockIdx.y;
    for (uint32_t i = threadIdx.x; i < nrep + 4; i += blockDim.x) s_mem[i] = 0u;
    if constexpr (TAB != 0) {
        u32x4* dst = reinterpret_cast<u32x4*>(s_mem + ((nrep + 4 + 3) & ~3u));
        const uint8_t* src = A.table[plane];
        for (uint32_t i = threadIdx.x; i < kCodes * (uint32_t)sizeof(E) / 16u; i += blockDim.x)
            dst[i] = ld_global<u32x4>(src + (size_t)i * 16);
    }
    __syncthreads();
    const uint32_t rep = threadIdx.x & ((1u << A.rep_log2) - 1u);
    uint32_t below = 0, above = 0, nan = 0;
    const double lo = A.lo[plane], hi = A.hi[plane], br = A.bin_range[plane];
    const int32_t ilo = A.ilo[plane], ihi = A.ihi[plane];
    walk_region<T, BE, kHistDepth>(A.G, [&](const Unit& u) {
        for_each_px<T, BE>(u, [&](T v) {
            uint32_t bin;
            if constexpr (TAB != 0) {
                const int32_t x = (int32_t)v;
                if (x < ilo) { ++below; return; }
                if (x > ihi) { ++above; return; }
                U code;
                __builtin_memcpy(&code, &v, sizeof(T));
                bin = s_tab[code];
            } else {
                const double d = (double)v;                // exact for every supported type
                if (d != d) { ++nan; return; }
                if (d < lo) { ++below; return; }
                if (d > hi) { ++above; return; }
                const double q = (d - lo) / br;            // 0 <= q <= n (1 + 2^-52)
                bin = min((uint32_t)q, n - 1u);
            }
            atomicAdd(&s_hist[(bin << A.rep_log2) + rep], 1u);
        });
    });
    below = wave_sum(below);
    above = wave_sum(above);
    nan = wave_sum(nan);
    if ((threadIdx.x & 63u) == 0) {
        if (below) atomicAdd(&s_out[0], below);
        if (above) atomicAdd(&s_out[1], above);
        if (nan) atomicAdd(&s_out[2], nan);
    }
    __syncthreads();
    // integer adds: the counts do not depend on the order the workgroups arrive in
    for (uint32_t b = threadIdx.x; b < n; b += blockDim.x) {
        uint32_t c = 0;
        for (uint32_t r = 0; r < (1u << A.rep_log2); ++r) c += s_hist[(b << A.rep_log2) + r];
        if (c) atomicAdd(&A.counts[(size_t)plane * n + b], c);
    }
    if (threadIdx.x < 3 && s_out[threadIdx.x])
        atomicAdd(&A.outside[(size_t)plane * 3 + threadIdx.x], (unsigned long long)s_out[threadIdx.x]);
}

// ------------------------------------------------------------------------------- host
static bool type_range(int32_t pixel_type, double* lo, double* hi) {
    switch (pixel_type) {   // StatsFactory.initPixelsRange, as omr_create_rendering_def
    case OMR_PIXELS_INT8: *lo = -128.0; *hi = 127.0; return true;
    case OMR_PIXELS_UINT8: *lo = 0.0; *hi = 255.0; return true;
    case OMR_PIXELS_INT16: *lo = -32768.0; *hi = 32767.0; return true;
    case OMR_PIXELS_UINT16: *lo = 0.0; *hi = 65535.0; return true;
    case OMR_PIXELS_INT32: *lo = -2147483648.0; *hi = 2147483647.0; return true;
    case OMR_PIXELS_UINT32: *lo = 0.0; *hi = 4294967295.0; return true;
    case OMR_PIXELS_FLOAT:
    case OMR_PIXELS_DOUBLE: *lo = 0.0; *hi = 1.0; return true;
    default: return false;
    }
}

// The region's geometry; *region_px its pixel count.  Every argument error of the plane and
// region (include/omr/omr.h) is decided here, before any launch.
static omr_status make_geom(Ctx* ctx, const void* const* d_planes, int32_t n_planes, int32_t pixel_type,
                            int32_t width, int32_t height, int64_t row_stride_px, const omr_region* region,
                            uint32_t block, Geom* g, uint64_t* region_px) {
    const int bpp = bytes_per_pixel(pixel_type);
    if (!bpp) return fail(ctx, OMR_INVALID_ARGUMENT, "unsupported pixel type");
    if (n_planes < 1 || n_planes > kMaxStatPlanes) return fail(ctx, OMR_INVALID_ARGUMENT, "1..32 planes per call");
    if (!d_planes) return fail(ctx, OMR_INVALID_ARGUMENT, "null plane list");
    if (width <= 0 || height <= 0) return fail(ctx, OMR_INVALID_ARGUMENT, "bad plane size");
    if (row_stride_px < 0 || (row_stride_px > 0 && row_stride_px < width))
        return fail(ctx, OMR_INVALID_ARGUMENT, "row stride shorter than a row");
    const int64_t stride = row_stride_px ? row_stride_px : width;
    int64_t x = 0, y = 0, w = width, h = height;
    if (region) {
        x = region->x; y = region->y; w = region->width; h = region->height;
        if (w <= 0 || h <= 0) return fail(ctx, OMR_INVALID_ARGUMENT, "empty region");
        if (x < 0 || y < 0 || x + w > width || y + h > height)
            return fail(ctx, OMR_INVALID_ARGUMENT, "region outside the plane");
    }
    if ((uint64_t)w * (uint64_t)h >= (1ull << 32)) return fail(ctx, OMR_INVALID_ARGUMENT, "region of 2^32 pixels or more");
    std::memset(g, 0, sizeof(*g));
    for (int i = 0; i < n_planes; ++i) {
        if (!d_planes[i]) return fail(ctx, OMR_INVALID_ARGUMENT, "null plane");
        if (reinterpret_cast<uintptr_t>(d_planes[i]) % (uintptr_t)bpp)
            return fail(ctx, OMR_INVALID_ARGUMENT, "plane not aligned to its pixel size");
        g->planes[i] = static_cast<const uint8_t*>(d_planes[i]);
    }
    *region_px = (uint64_t)w * (uint64_t)h;
    const bool run = w == stride || h == 1;          // the region is one contiguous run of pixels
    const uint64_t row_px = run ? (uint64_t)w * (uint64_t)h : (uint64_t)w;
    g->org = (y * stride + x) * bpp;
    g->pitch = stride * bpp;
    g->row_bytes = (int64_t)(row_px * (uint64_t)bpp);
    g->rows = run ? 1u : (uint32_t)h;
    const uint64_t units = (row_px * (uint64_t)bpp + 15) / 16 + 1;   // a row that starts inside a unit spans one more
    uint32_t lw = 0;
    while ((1ull << lw) < std::min<uint64_t>(units, block)) ++lw;
    g->lw_log2 = lw;
    const uint64_t rows_per_tile = block >> lw;
    const uint64_t ub = (units + (1ull << lw) - 1) >> lw;
    const uint64_t tiles = ((uint64_t)g->rows + rows_per_tile - 1) / rows_per_tile * ub;
    if (tiles >= (1ull << 32)) return fail(ctx, OMR_INVALID_ARGUMENT, "region too large");
    g->unit_blocks = (uint32_t)ub;
    g->tiles = (uint32_t)tiles;
    return OMR_OK;
}

static uint32_t grid_x(const Ctx* ctx, const Geom& g, int n_planes, int blocks_per_cu) {
    const int64_t cap = std::max<int64_t>(1, (int64_t)ctx->cu_count * blocks_per_cu / n_planes);
    return (uint32_t)std::min<int64_t>((int64_t)g.tiles, cap);
}

template <typename T>
static void launch_minmax(const Geom& g, bool be, dim3 grid, hipStream_t s, StatPartial* partials) {
    if (be) hipLaunchKernelGGL((k_plane_minmax<T, true>), grid, dim3(kStatBlock), 0, s, g, partials);
    else hipLaunchKernelGGL((k_plane_minmax<T, false>), grid, dim3(kStatBlock), 0, s, g, partials);
}

constexpr size_t kStatsMaxGrid = 2048 * 8;   // workgroups of one statistics launch, at most

static size_t stats_scratch_bytes(int32_t n_planes) {
    return align_up(sizeof(StatPartial) * kStatsMaxGrid, 256) + align_up(sizeof(omr_plane_stats) * (size_t)n_planes, 256);
}

// Statistics of validated planes into `scratch` (device, stats_scratch_bytes) and from there to
// stats_out (host) on the context's stream; the caller synchronises.
static omr_status enqueue_stats(Ctx* ctx, const Geom& g, int32_t n_planes, int32_t pixel_type, int32_t be,
                                uint64_t region_px, uint8_t* scratch, omr_plane_stats* stats_out) {
    uint32_t gx = grid_x(ctx, g, n_planes, kStatBlocksPerCu);
    gx = (uint32_t)std::min<size_t>(gx, kStatsMaxGrid / (size_t)n_planes);
    StatPartial* partials = reinterpret_cast<StatPartial*>(scratch);
    omr_plane_stats* d_stats = reinterpret_cast<omr_plane_stats*>(scratch + align_up(sizeof(StatPartial) * kStatsMaxGrid, 256));
    const dim3 grid(gx, (unsigned)n_planes);
    const bool b = be != 0;
    switch (pixel_type) {
    case OMR_PIXELS_INT8: launch_minmax<int8_t>(g, false, grid, ctx->stream, partials); break;
    case OMR_PIXELS_UINT8: launch_minmax<uint8_t>(g, false, grid, ctx->stream, partials); break;
    case OMR_PIXELS_INT16: launch_minmax<int16_t>(g, b, grid, ctx->stream, partials); break;
    case OMR_PIXELS_UINT16: launch_minmax<uint16_t>(g, b, grid, ctx->stream, partials); break;
    case OMR_PIXELS_INT32: launch_minmax<int32_t>(g, b, grid, ctx->stream, partials); break;
    case OMR_PIXELS_UINT32: launch_minmax<uint32_t>(g, b, grid, ctx->stream, partials); break;
    case OMR_PIXELS_FLOAT: launch_minmax<float>(g, b, grid, ctx->stream, partials); break;
    default: launch_minmax<double>(g, b, grid, ctx->stream, partials); break;
    }
    OMR_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_plane_minmax_final, dim3((unsigned)n_planes), dim3(kStatBlock), 0, ctx->stream, partials, gx,
                       region_px, d_stats);
    OMR_HIP(ctx, hipGetLastError());
    OMR_HIP(ctx, hipMemcpyAsync(stats_out, d_stats, sizeof(omr_plane_stats) * (size_t)n_planes, hipMemcpyDeviceToHost,
                                ctx->stream));
    return OMR_OK;
}

static omr_status validate_ranges(Ctx* ctx, const double* lo, const double* hi, int32_t n_planes, int32_t bin_count) {
    if (bin_count < 1 || bin_count > OMR_HIST_MAX_BINS) return fail(ctx, OMR_INVALID_ARGUMENT, "1..4096 bins");
    if (!lo || !hi) return fail(ctx, OMR_INVALID_ARGUMENT, "null range");
    for (int i = 0; i < n_planes; ++i) {
        if (!std::isfinite(lo[i]) || !std::isfinite(hi[i]) || !std::isfinite(hi[i] - lo[i]))
            return fail(ctx, OMR_INVALID_ARGUMENT, "histogram range not finite");
        if (lo[i] > hi[i]) return fail(ctx, OMR_INVALID_ARGUMENT, "histogram range with lo > hi");
    }
    return OMR_OK;
}

static int env_int(const char* name, int dflt) {
    const char* v = std::getenv(name);
    return v && *v ? std::atoi(v) : dflt;
}

// Sub-histogram copies per workgroup: the largest power of two, at most 8, whose counters fit
// `budget` bytes of LDS (CHANGELOG.md has the measured factors); OMR_HIST_REP overrides it for
// measurements, within what `limit` bytes allow.
static uint32_t pick_rep_log2(int32_t n, size_t budget, size_t limit) {
    const int forced = env_int("OMR_HIST_REP", 0);
    uint32_t r = 0;
    if (forced >= 1) {
        while (r < 5 && (2u << r) <= (uint32_t)forced && ((size_t)n * 4 << (r + 1)) <= limit) ++r;
        return r;
    }
    while (r < 3 && ((size_t)n * 4 << (r + 1)) <= budget) ++r;
    return r;
}

template <typename T, int TAB>
static hipError_t launch_hist_tab(const HistArgs& a, bool be, dim3 grid, uint32_t block, size_t lds, hipStream_t s) {
    if (be) {
        if (lds > 64 * 1024) {
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_plane_histogram<T, true, TAB>),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL((k_plane_histogram<T, true, TAB>), grid, dim3(block), lds, s, a);
    } else {
        if (lds > 64 * 1024) {
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_plane_histogram<T, false, TAB>),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL((k_plane_histogram<T, false, TAB>), grid, dim3(block), lds, s, a);
    }
    return hipGetLastError();
}

template <typename T>
static hipError_t launch_hist(const HistArgs& a, int tab, bool be, dim3 grid, uint32_t block, size_t lds, hipStream_t s) {
    if constexpr (sizeof(T) <= 2) {
        if (tab == 1) return launch_hist_tab<T, 1>(a, be, grid, block, lds, s);
        if (tab == 2) return launch_hist_tab<T, 2>(a, be, grid, block, lds, s);
    }
    return launch_hist_tab<T, 0>(a, be, grid, block, lds, s);
}

static size_t table_bytes(int32_t pixel_type, int32_t bin_count) {
    const int bpp = bytes_per_pixel(pixel_type);
    if (bpp > 2) return 0;
    return (bpp == 1 ? 256u : 65536u) * (size_t)(bin_count <= 256 ? 1 : 2);
}

static size_t hist_scratch_bytes(int32_t n_planes, int32_t pixel_type, int32_t bin_count) {
    return align_up(align_up(sizeof(uint32_t) * (size_t)n_planes * bin_count, 8) + 3 * sizeof(uint64_t) * (size_t)n_planes, 256) +
           align_up(table_bytes(pixel_type, bin_count), 256) * (size_t)n_planes;
}

// The value -> bin table of one range, indexed by a pixel's unsigned bits: omr_histogram_bin_of
// for every value inside [lo, hi] (0 outside: the kernel never reads those entries).
static void build_table(int32_t pixel_type, double lo, double hi, int32_t n, uint8_t* out) {
    const bool sgn = pixel_type == OMR_PIXELS_INT8 || pixel_type == OMR_PIXELS_INT16;
    const bool wide = bytes_per_pixel(pixel_type) == 2;
    const uint32_t codes = wide ? 65536u : 256u;
    for (uint32_t c = 0; c < codes; ++c) {
        const int32_t v = !sgn ? (int32_t)c : wide ? (int32_t)(int16_t)(uint16_t)c : (int32_t)(int8_t)(uint8_t)c;
        const int32_t b = omr_histogram_bin_of((double)v, lo, hi, n);
        const uint32_t e = b < 0 ? 0u : (uint32_t)b;
        if (n <= 256) out[c] = (uint8_t)e;
        else reinterpret_cast<uint16_t*>(out)[c] = (uint16_t)e;
    }
}

// Histograms of validated planes: counts and outside counters in `scratch` (device,
// hist_scratch_bytes), then to counts_out / h_outside (host: [n_planes][3]) on the context's
// stream; the caller synchronises and keeps `tables` alive until then.
static omr_status enqueue_hist(Ctx* ctx, int32_t n_planes, int32_t pixel_type, int32_t be, int32_t width,
                               int32_t height, int64_t row_stride_px, const omr_region* region,
                               const void* const* d_planes, const double* lo, const double* hi, int32_t n,
                               uint8_t* scratch, std::vector<uint8_t>& tables, uint32_t* counts_out,
                               uint64_t* h_outside) {
    const int bpp = bytes_per_pixel(pixel_type);
    const size_t tab_one = table_bytes(pixel_type, n);
    const size_t counts_bytes = sizeof(uint32_t) * (size_t)n_planes * n, out_bytes = 3 * sizeof(uint64_t) * (size_t)n_planes;
    const size_t out_off = align_up(counts_bytes, 8);          // the outside counters are 64-bit
    uint8_t* d_tables = scratch + align_up(out_off + out_bytes, 256);
    HistArgs a;
    std::memset(&a, 0, sizeof(a));
    // Route.  Tables for the 8- and 16-bit types, except that a 16-bit region smaller than its
    // table, or a device whose workgroups cannot hold the table, takes the fp64 evaluation like
    // every other type.  OMR_HIST_ROUTE=1 forces the evaluation, 2 the table (measurement switch).
    const int forced = env_int("OMR_HIST_ROUTE", 0);
    uint64_t region_px = 0;
    omr_status st = make_geom(ctx, d_planes, n_planes, pixel_type, width, height, row_stride_px, region, kStatBlock,
                              &a.G, &region_px);
    if (st) return st;
    const size_t lds_limit = ctx->lds_per_block;
    int tab = tab_one && forced != 1 ? (n <= 256 ? 1 : 2) : 0;
    if (tab && bpp == 2 && (tab_one + 4096 > lds_limit || (forced != 2 && region_px * 2 < tab_one))) tab = 0;
    const bool tab16 = tab && bpp == 2;
    const uint32_t block = tab16 ? kTab16Block : kStatBlock;
    uint32_t gx;
    if (tab16) {
        st = make_geom(ctx, d_planes, n_planes, pixel_type, width, height, row_stride_px, region, block, &a.G, &region_px);
        if (st) return st;
        // at most two resident workgroups per CU, each reading at least its table's size in pixels
        const uint64_t by_work = std::max<uint64_t>(1, region_px * 2 / tab_one);
        gx = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(a.G.tiles, by_work),
                                          std::max<uint64_t>(1, (uint64_t)ctx->cu_count * 2 / n_planes));
    } else {
        gx = grid_x(ctx, a.G, n_planes, 8);
    }
    const size_t lds_tab = tab ? tab_one : 0;
    const size_t rep_limit = tab16 ? lds_limit - lds_tab - 64 : 60 * 1024;
    a.rep_log2 = pick_rep_log2(n, std::min<size_t>(32 * 1024, rep_limit), rep_limit);
    a.n = n;
    a.counts = reinterpret_cast<uint32_t*>(scratch);
    a.outside = reinterpret_cast<unsigned long long*>(scratch + out_off);
    const size_t tab_al = align_up(tab_one, 256);
    int n_tables = 0;
    std::vector<int> tab_of(n_planes, 0);
    if (tab) tables.resize(tab_al * (size_t)n_planes);
    double tmin, tmax;
    type_range(pixel_type, &tmin, &tmax);
    for (int i = 0; i < n_planes; ++i) {
        a.lo[i] = lo[i];
        a.hi[i] = hi[i];
        const double range = hi[i] - lo[i] + 1.0;
        a.bin_range[i] = range / (double)n;
        if (!tab) continue;
        // integer pixels: v < lo <=> v < ceil(lo), v > hi <=> v > floor(hi); clamped so they fit int32
        a.ilo[i] = (int32_t)std::min(std::max(std::ceil(lo[i]), tmin - 1.0), tmax + 1.0);
        a.ihi[i] = (int32_t)std::min(std::max(std::floor(hi[i]), tmin - 1.0), tmax + 1.0);
        int t = -1;
        for (int k = 0; k < i && t < 0; ++k)
            if (lo[k] == lo[i] && hi[k] == hi[i]) t = tab_of[k];      // planes of one range share a table
        if (t < 0) {
            t = n_tables++;
            build_table(pixel_type, lo[i], hi[i], n, tables.data() + tab_al * (size_t)t);
        }
        tab_of[i] = t;
        a.table[i] = d_tables + tab_al * (size_t)t;
    }
    OMR_HIP(ctx, hipMemsetAsync(scratch, 0, out_off + out_bytes, ctx->stream));
    if (n_tables)
        OMR_HIP(ctx, hipMemcpyAsync(d_tables, tables.data(), tab_al * (size_t)n_tables, hipMemcpyHostToDevice, ctx->stream));
    const size_t lds = (((size_t)n << a.rep_log2) + 4 + 3) / 4 * 16 + lds_tab;
    const dim3 grid(gx, (unsigned)n_planes);
    const bool b = be != 0;
    hipError_t e;
    switch (pixel_type) {
    case OMR_PIXELS_INT8: e = launch_hist<int8_t>(a, tab, false, grid, block, lds, ctx->stream); break;
    case OMR_PIXELS_UINT8: e = launch_hist<uint8_t>(a, tab, false, grid, block, lds, ctx->stream); break;
    case OMR_PIXELS_INT16: e = launch_hist<int16_t>(a, tab, b, grid, block, lds, ctx->stream); break;
    case OMR_PIXELS_UINT16: e = launch_hist<uint16_t>(a, tab, b, grid, block, lds, ctx->stream); break;
    case OMR_PIXELS_INT32: e = launch_hist<int32_t>(a, tab, b, grid, block, lds, ctx->stream); break;
    case OMR_PIXELS_UINT32: e = launch_hist<uint32_t>(a, tab, b, grid, block, lds, ctx->stream); break;
    case OMR_PIXELS_FLOAT: e = launch_hist<float>(a, tab, b, grid, block, lds, ctx->stream); break;
    default: e = launch_hist<double>(a, tab, b, grid, block, lds, ctx->stream); break;
    }
    OMR_HIP(ctx, e);
    OMR_HIP(ctx, hipMemcpyAsync(counts_out, a.counts, counts_bytes, hipMemcpyDeviceToHost, ctx->stream));
    OMR_HIP(ctx, hipMemcpyAsync(h_outside, a.outside, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    return OMR_OK;
}

size_t histogram_plane_ws_bytes(int32_t pixel_type, int32_t bin_count) {
    return stats_scratch_bytes(1) + hist_scratch_bytes(1, pixel_type, bin_count);
}

omr_status validate_histogram_plane(Ctx* ctx, int32_t pixel_type, int32_t width, int32_t height,
                                    const omr_region* region, int32_t range_mode, double lo, double hi,
                                    int32_t bin_count, const void* counts_out, const void* info_out) {
    if (!counts_out || !info_out) return fail(ctx, OMR_INVALID_ARGUMENT, "null output");
    if (range_mode < OMR_HIST_RANGE_TYPE || range_mode > OMR_HIST_RANGE_EXPLICIT)
        return fail(ctx, OMR_INVALID_ARGUMENT, "unknown range mode");
    Geom g;
    uint64_t px;
    const void* dummy[1] = {reinterpret_cast<const void*>((uintptr_t)256)};   // geometry only: never dereferenced
    omr_status st = make_geom(ctx, dummy, 1, pixel_type, width, height, 0, region, kStatBlock, &g, &px);
    if (st) return st;
    double l = 0.0, h = 0.0;
    if (range_mode == OMR_HIST_RANGE_EXPLICIT) { l = lo; h = hi; }
    return validate_ranges(ctx, &l, &h, 1, bin_count);
}

// One plane already in device memory at d_plane (width x height, rows packed), validated by
// validate_histogram_plane; scratch: histogram_plane_ws_bytes of device memory.  Synchronous.
omr_status histogram_plane_uploaded(Ctx* ctx, const void* d_plane, uint8_t* scratch, int32_t pixel_type,
                                    int32_t big_endian, int32_t width, int32_t height, const omr_region* region,
                                    int32_t range_mode, double lo, double hi, int32_t bin_count,
                                    uint32_t* counts_out, omr_histogram_info* info_out, omr_plane_stats* stats_out) {
    const void* planes[1] = {d_plane};
    omr_plane_stats stats;
    std::memset(&stats, 0, sizeof(stats));
    if (range_mode == OMR_HIST_RANGE_PLANE || stats_out) {
        Geom g;
        uint64_t px = 0;
        omr_status st = make_geom(ctx, planes, 1, pixel_type, width, height, 0, region, kStatBlock, &g, &px);
        if (st) return st;
        st = enqueue_stats(ctx, g, 1, pixel_type, big_endian, px, scratch, &stats);
        if (st) return st;
        OMR_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (stats_out) *stats_out = stats;
    }
    if (range_mode == OMR_HIST_RANGE_TYPE) {
        type_range(pixel_type, &lo, &hi);
    } else if (range_mode == OMR_HIST_RANGE_PLANE) {
        lo = stats.min;
        hi = stats.max;
        if (stats.count == 0) {            // nothing but NaN: no range, every count 0
            std::memset(counts_out, 0, sizeof(uint32_t) * (size_t)bin_count);
            info_out->lo = lo;
            info_out->hi = hi;
            info_out->below = info_out->above = 0;
            info_out->nan_count = stats.nan_count;
            return OMR_OK;
        }
        omr_status st = validate_ranges(ctx, &lo, &hi, 1, bin_count);
        if (st) return st;
    }
    std::vector<uint8_t> tables;
    uint64_t outside[3] = {0, 0, 0};
    omr_status st = enqueue_hist(ctx, 1, pixel_type, big_endian, width, height, 0, region, planes, &lo, &hi, bin_count,
                                 scratch + stats_scratch_bytes(1), tables, counts_out, outside);
    if (st) return st;
    OMR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    info_out->lo = lo;
    info_out->hi = hi;
    info_out->below = outside[0];
    info_out->above = outside[1];
    info_out->nan_count = outside[2];
    return OMR_OK;
}

}  // namespace omr

using namespace omr;

extern "C" {

int32_t omr_histogram_bin_of(double v, double lo, double hi, int32_t bin_count) {
    if (v != v) return -3;
    if (v < lo) return -1;
    if (v > hi) return -2;
    if (bin_count < 1) bin_count = 1;
    const double range = hi - lo + 1.0;
    const double bin_range = range / (double)bin_count;
    const double q = (v - lo) / bin_range;
    // q >= 0 here, and q <= bin_count (1 + 2^-52) for a finite range; the guard keeps the
    // conversion defined for ranges the device calls reject (infinite ends)
    const int64_t b = q < 9.0e18 ? (int64_t)q : INT64_MAX;
    return (int32_t)std::min<int64_t>(b, (int64_t)bin_count - 1);
}

omr_status omr_plane_stats_device(omr_ctx* ctx, const void* const* d_planes, int32_t n_planes, int32_t pixel_type,
                                  int32_t big_endian, int32_t width, int32_t height, int64_t row_stride_px,
                                  const omr_region* region, omr_plane_stats* stats_out) {
    if (!ctx) return OMR_INVALID_ARGUMENT;
    if (!stats_out) return fail(ctx, OMR_INVALID_ARGUMENT, "null output");
    Geom g;
    uint64_t px = 0;
    omr_status st = make_geom(ctx, d_planes, n_planes, pixel_type, width, height, row_stride_px, region, kStatBlock, &g, &px);
    if (st) return st;
    OMR_HIP(ctx, hipSetDevice(ctx->device));
    st = ensure_workspace(ctx, stats_scratch_bytes(n_planes));
    if (st) return st;
    st = enqueue_stats(ctx, g, n_planes, pixel_type, big_endian, px, static_cast<uint8_t*>(ctx->ws), stats_out);
    if (st) return st;
    OMR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return OMR_OK;
}

omr_status omr_histogram_device(omr_ctx* ctx, const void* const* d_planes, int32_t n_planes, int32_t pixel_type,
                                int32_t big_endian, int32_t width, int32_t height, int64_t row_stride_px,
                                const omr_region* region, const double* lo, const double* hi, int32_t bin_count,
                                uint32_t* counts_out, omr_histogram_info* info_out) {
    if (!ctx) return OMR_INVALID_ARGUMENT;
    if (!counts_out || !info_out) return fail(ctx, OMR_INVALID_ARGUMENT, "null output");
    Geom g;
    uint64_t px = 0;
    omr_status st = make_geom(ctx, d_planes, n_planes, pixel_type, width, height, row_stride_px, region, kStatBlock, &g, &px);
    if (st) return st;
    st = validate_ranges(ctx, lo, hi, n_planes, bin_count);
    if (st) return st;
    OMR_HIP(ctx, hipSetDevice(ctx->device));
    st = ensure_workspace(ctx, hist_scratch_bytes(n_planes, pixel_type, bin_count));
    if (st) return st;
    std::vector<uint8_t> tables;
    uint64_t outside[kMaxStatPlanes * 3];
    st = enqueue_hist(ctx, n_planes, pixel_type, big_endian, width, height, row_stride_px, region, d_planes, lo, hi,
                      bin_count, static_cast<uint8_t*>(ctx->ws), tables, counts_out, outside);
    if (st) return st;
    OMR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < n_planes; ++i) {
        info_out[i].lo = lo[i];
        info_out[i].hi = hi[i];
        info_out[i].below = outside[3 * i];
        info_out[i].above = outside[3 * i + 1];
        info_out[i].nan_count = outside[3 * i + 2];
    }
    return OMR_OK;
}

omr_status omr_histogram(omr_ctx* ctx, const void* plane, int32_t pixel_type, int32_t big_endian, int32_t width,
                         int32_t height, const omr_region* region, int32_t range_mode, double lo, double hi,
                         int32_t bin_count, uint32_t* counts_out, omr_histogram_info* info_out,
                         omr_plane_stats* stats_out) {
    if (!ctx) return OMR_INVALID_ARGUMENT;
    if (!plane) return fail(ctx, OMR_INVALID_ARGUMENT, "null plane");
    omr_status st = validate_histogram_plane(ctx, pixel_type, width, height, region, range_mode, lo, hi, bin_count,
                                             counts_out, info_out);
    if (st) return st;
    OMR_HIP(ctx, hipSetDevice(ctx->device));
    const size_t bytes = (size_t)width * height * bytes_per_pixel(pixel_type), plane_al = align_up(bytes, 256);
    st = ensure_workspace(ctx, plane_al + histogram_plane_ws_bytes(pixel_type, bin_count));
    if (st) return st;
    uint8_t* ws = static_cast<uint8_t*>(ctx->ws);
    OMR_HIP(ctx, hipMemcpyAsync(ws, plane, bytes, hipMemcpyHostToDevice, ctx->stream));
    return histogram_plane_uploaded(ctx, ws, ws + plane_al, pixel_type, big_endian, width, height, region, range_mode,
                                    lo, hi, bin_count, counts_out, info_out, stats_out);
}

}  // extern "C"
