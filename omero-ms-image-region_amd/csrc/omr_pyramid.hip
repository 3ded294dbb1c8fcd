// omr_pyramid.hip — K11: resolution pyramid levels of planes in HBM.
//
// The rule (include/omr/omr.h, DESIGN.md §4 "K11 pyramid"): level k is floor(W/2^k) x floor(H/2^k)
// and is made from the stored level k-1, either by taking the top-left pixel of each 2x2 box
// (subsample, bytes verbatim) or by its mean (integers: floor((a+b+c+d+2)/4); float through
// double; double as written), one IEEE rounding per operation.
//
//   k_pyramid   a lane owns 8 source rows x 16 bytes (32 bytes of 64-bit pixels): 8 x 16, 8 x 8,
//               8 x 4 or 8 x 4 pixels.  It loads them once, back to back, and reduces them in
//               registers to its 4-, 2- and 1-row pieces of the next three levels (two levels for
//               32- and 64-bit pixels); one more level comes from a register exchange between
//               neighbouring lanes of a wave.  So level 0 is read once per launch: no LDS, no
//               atomics, no dependence on scheduling.  Deeper levels come from running the kernel
//               again on the last level written (<= 1/256 of the plane; 1/64 for 32- and 64-bit
//               pixels).  blockIdx.y is the plane.
#include "omr_device.h"

#include <type_traits>

namespace omr {

constexpr int kKindPyramid = 12;       // omr_ctx_kernel_timings kind
constexpr int kPyrRows = 8;            // source rows a lane owns
constexpr int kPyrMaxPlanes = 32;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

template <int BPP> struct PyrGeom {
    static constexpr int CH = BPP == 8 ? 2 : 1;        // 16-byte chunks per lane and row
    static constexpr int WORDS = 4 * CH;               // dwords per lane and source row
    static constexpr int PX = 16 * CH / BPP;           // pixels per lane and source row
    static constexpr int NL = PX >= 8 ? 3 : 2;         // levels one launch writes
};
template <int BPP> struct PyrBits;
template <> struct PyrBits<1> { typedef uint8_t U; };
template <> struct PyrBits<2> { typedef uint16_t U; };
template <> struct PyrBits<4> { typedef uint32_t U; };
template <> struct PyrBits<8> { typedef uint64_t U; };

// Store through an explicit global pointer (as ld_global, omr_device.h).
template <typename T>
__device__ __forceinline__ void st_global(void* p, T v) {
    *(__attribute__((address_space(1))) T*)p = v;
}

// Pixel p of a row segment held as dwords in memory order.
template <int BPP>
__device__ __forceinline__ typename PyrBits<BPP>::U px_get(const uint32_t* w, int p) {
    if constexpr (BPP == 1) return (uint8_t)(w[p >> 2] >> (8 * (p & 3)));
    else if constexpr (BPP == 2) return (uint16_t)(w[p >> 1] >> (16 * (p & 1)));
    else if constexpr (BPP == 4) return w[p];
    else return (uint64_t)w[2 * p] | ((uint64_t)w[2 * p + 1] << 32);
}
// The same, into dwords that start as zero.
template <int BPP>
__device__ __forceinline__ void px_set(uint32_t* w, int p, typename PyrBits<BPP>::U v) {
    if constexpr (BPP == 1) w[p >> 2] |= (uint32_t)v << (8 * (p & 3));
    else if constexpr (BPP == 2) w[p >> 1] |= (uint32_t)v << (16 * (p & 1));
    else if constexpr (BPP == 4) w[p] = v;
    else {
        w[2 * p] = (uint32_t)v;
        w[2 * p + 1] = (uint32_t)(v >> 32);
    }
}
// Big-endian pixels <-> native, a row segment at a time in registers (v_perm_b32); its own inverse.
template <int BPP, bool BE, int N>
__device__ __forceinline__ void swap_words(uint32_t (&w)[N]) {
    if constexpr (BE && BPP == 2) {
#pragma unroll
        for (int i = 0; i < N; ++i) w[i] = bswap16x2(w[i]);
    } else if constexpr (BE && BPP == 4) {
#pragma unroll
        for (int i = 0; i < N; ++i) w[i] = bswap32(w[i]);
    } else if constexpr (BE && BPP == 8) {
#pragma unroll
        for (int i = 0; i + 1 < N; i += 2) {
            const uint32_t t = bswap32(w[i]);
            w[i] = bswap32(w[i + 1]);
            w[i + 1] = t;
        }
    }
}

// The two rules on the bits of a 2x2 box (a b / c d).
struct PyrSub {
    template <typename U>
    static __device__ __forceinline__ U op(U a, U, U, U) { return a; }
};
template <typename T> struct PyrMean {
    template <typename U>
    static __device__ __forceinline__ U op(U ua, U ub, U uc, U ud) {
        static_assert(sizeof(U) == sizeof(T), "pixel size");
        const T a = __builtin_bit_cast(T, ua), b = __builtin_bit_cast(T, ub), c = __builtin_bit_cast(T, uc),
                d = __builtin_bit_cast(T, ud);
        T r;
        if constexpr (sizeof(T) == 8) {                       // double
            r = ((a + b) + (c + d)) * 0.25;
        } else if constexpr (std::is_floating_point<T>::value) {               // float, through double
            r = (float)((((double)a + (double)b) + ((double)c + (double)d)) * 0.25);
        } else if constexpr (sizeof(T) == 4 && std::is_unsigned<T>::value) {   // uint32: the sum needs 34 bits
            r = (T)(((uint64_t)a + b + c + d + 2) >> 2);
        } else if constexpr (sizeof(T) == 4) {                // int32; >> of a negative is arithmetic
            r = (T)(((int64_t)a + b + c + d + 2) >> 2);
        } else {                                              // 8 and 16 bits: the sum fits int32
            r = (T)(((int32_t)a + (int32_t)b + (int32_t)c + (int32_t)d + 2) >> 2);
        }
        return __builtin_bit_cast(U, r);
    }
};

constexpr int kPyrMaxLaunchLevels = 4;   // three lane-local levels and one across lanes

struct PyrArgs {
    const uint8_t* src[kPyrMaxPlanes];         // source planes (uniform index blockIdx.y)
    uint8_t* dst[kPyrMaxLaunchLevels];         // plane 0 of each level this launch writes
    int64_t dst_plane[kPyrMaxLaunchLevels];    // bytes per plane of those levels
    int64_t row_stride;                        // source row stride, bytes
    int32_t W, H;                              // source size
    int32_t w[kPyrMaxLaunchLevels], h[kPyrMaxLaunchLevels];   // sizes of the levels written
    int32_t nl;                                // levels to write: 1..NL+1
    int32_t vec;                               // planes, strides and level rows on the vector grid
    uint32_t CW, CHR;                          // lane blocks per source row and per column
    uint32_t waves, WC;                        // waves per plane; waves per row of lane blocks
    FastDiv divWC;
};

// One level's piece of a lane: ROWS x NPX pixels held as NW dwords per row, at (xk0, yk0).
template <int BPP, int ROWS, int NPX, int NW>
__device__ __forceinline__ void store_piece(uint8_t* dst, int32_t wk, int32_t hk, int32_t xk0, int32_t yk0,
                                            const uint32_t (&o)[ROWS][NW], bool fast) {
    typedef typename PyrBits<BPP>::U U;
    constexpr int kBytes = NPX * BPP;
#pragma unroll
    for (int j = 0; j < ROWS; ++j) {
        const int32_t yk = yk0 + j;
        if (yk >= hk) continue;
        uint8_t* const row = dst + ((int64_t)yk * wk + xk0) * BPP;
        if (fast) {
            if constexpr (kBytes == 16) {
                u32x4 v;
                v[0] = o[j][0]; v[1] = o[j][1]; v[2] = o[j][2]; v[3] = o[j][3];
                st_global<u32x4>(row, v);
            } else if constexpr (kBytes == 8) {
                u32x2 v;
                v[0] = o[j][0]; v[1] = o[j][1];
                st_global<u32x2>(row, v);
            } else if constexpr (kBytes == 4) {
                st_global<uint32_t>(row, o[j][0]);
            } else {
                static_assert(kBytes == 2, "piece width");
                st_global<uint16_t>(row, (uint16_t)o[j][0]);
            }
        } else {
#pragma unroll
            for (int i = 0; i < NPX; ++i)
                if (xk0 + i < wk) st_global<U>(row + i * BPP, px_get<BPP>(o[j], i));
        }
    }
}

// ROWS x NPX pixels of a level from the 2*ROWS x 2*NPX pixels under them (native byte order).
template <int BPP, typename OP, int ROWS, int NPX, int NWI, int NWO>
__device__ __forceinline__ void reduce_piece(const uint32_t (&in)[2 * ROWS][NWI], uint32_t (&out)[ROWS][NWO]) {
#pragma unroll
    for (int j = 0; j < ROWS; ++j) {
#pragma unroll
        for (int i = 0; i < NWO; ++i) out[j][i] = 0;
#pragma unroll
        for (int i = 0; i < NPX; ++i)
            px_set<BPP>(out[j], i,
                        OP::op(px_get<BPP>(in[2 * j], 2 * i), px_get<BPP>(in[2 * j], 2 * i + 1),
                               px_get<BPP>(in[2 * j + 1], 2 * i), px_get<BPP>(in[2 * j + 1], 2 * i + 1)));
    }
}

template <int BPP, bool BE, typename OP>
__global__ void __launch_bounds__(256) k_pyramid(const PyrArgs A) {
    typedef PyrGeom<BPP> G;
    typedef typename PyrBits<BPP>::U U;
    // A wave covers 32 lane blocks of one block row and the 32 below them (lanes 32..63), so a
    // row's loads are 512 contiguous bytes and the lanes that meet in the level made across lanes
    // (l, l ^ 1, l ^ 32, l ^ 33) sit in one wave.
    const uint32_t wv = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (wv >= A.waves) return;
    const uint32_t wr = fdiv(wv, A.divWC), wc = wv - wr * A.WC;
    const uint32_t cx = wc * 32u + (lane & 31u), by = wr * 2u + (lane >> 5);
    // (no result that is stored depends on a lane outside the plane: a level's pixel exists only
    // when the whole 2x2 box under it does)
    if (cx >= A.CW || by >= A.CHR) return;
    const int32_t x0 = (int32_t)cx * G::PX, y0 = (int32_t)by * kPyrRows;
    const uint8_t* const src = A.src[blockIdx.y];
    // The vector form: the lane's block lies inside the row (a block hanging over the bottom edge
    // repeats the last row, whose results are not stored) and everything is on the 16-byte grid.
    // Otherwise the same registers are filled pixel by pixel from clamped coordinates.
    const bool fast = A.vec && x0 + G::PX <= A.W;
    uint32_t s[kPyrRows][G::WORDS];
    if (fast) {
#pragma unroll
        for (int r = 0; r < kPyrRows; ++r) {
            const int32_t y = min(y0 + r, A.H - 1);
            const uint8_t* const row = src + (int64_t)y * A.row_stride + (int64_t)x0 * BPP;
#pragma unroll
            for (int c = 0; c < G::CH; ++c) {
                const u32x4 v = ld_global<u32x4>(row + 16 * c);
                s[r][4 * c] = v[0]; s[r][4 * c + 1] = v[1]; s[r][4 * c + 2] = v[2]; s[r][4 * c + 3] = v[3];
            }
        }
    } else {
#pragma unroll
        for (int r = 0; r < kPyrRows; ++r) {
            const int32_t y = min(y0 + r, A.H - 1);
            const uint8_t* const row = src + (int64_t)y * A.row_stride;
#pragma unroll
            for (int i = 0; i < G::WORDS; ++i) s[r][i] = 0;
#pragma unroll
            for (int q = 0; q < G::PX; ++q) {
                const int32_t x = min(x0 + q, A.W - 1);
                px_set<BPP>(s[r], q, ld_global<U>(row + (int64_t)x * BPP));
            }
        }
    }
#pragma unroll
    for (int r = 0; r < kPyrRows; ++r) swap_words<BPP, BE>(s[r]);

    const int64_t plane = blockIdx.y;
    constexpr int NP1 = G::PX / 2, NW1 = NP1 * BPP / 4;
    uint32_t o1[4][NW1];
    reduce_piece<BPP, OP, 4, NP1>(s, o1);
    constexpr int NP2 = G::PX / 4, NW2 = (NP2 * BPP + 3) / 4;
    uint32_t o2[2][NW2];
    if (A.nl >= 2) reduce_piece<BPP, OP, 2, NP2>(o1, o2);
#pragma unroll
    for (int j = 0; j < 4; ++j) swap_words<BPP, BE>(o1[j]);
    store_piece<BPP, 4, NP1>(A.dst[0] + plane * A.dst_plane[0], A.w[0], A.h[0], x0 >> 1, y0 >> 1, o1, fast);
    if (A.nl < 2) return;                                                  // (uniform)
    // The lane's deepest piece in native byte order, as the two rows of the box the next level is
    // made from: its own two rows (32- and 64-bit pixels: 2 rows x 1 pixel), or its one row and,
    // further down, the row of the lane below (8- and 16-bit pixels: 1 row x 2 / 1 pixels).
    constexpr int NPT = G::PX >> G::NL, NWT = (NPT * BPP + 3) / 4;
    uint32_t top[2][NWT];
    if constexpr (G::NL == 3) {
        constexpr int NP3 = G::PX / 8;
        uint32_t o3[1][1];
        if (A.nl >= 3) {
            reduce_piece<BPP, OP, 1, NP3>(o2, o3);
            top[0][0] = top[1][0] = o3[0][0];
            swap_words<BPP, BE>(o3[0]);
            store_piece<BPP, 1, NP3>(A.dst[2] + plane * A.dst_plane[2], A.w[2], A.h[2], x0 >> 3, y0 >> 3, o3, fast);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < NWT; ++i) top[j][i] = o2[j][i];
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) swap_words<BPP, BE>(o2[j]);
    store_piece<BPP, 2, NP2>(A.dst[1] + plane * A.dst_plane[1], A.w[1], A.h[1], x0 >> 2, y0 >> 2, o2, fast);
    if (A.nl <= G::NL) return;                                             // (uniform)
    // One more level across lanes: the box of an even lane is its own piece and its right
    // neighbour's, over the same two of the lane below (8- and 16-bit pixels) or over their second
    // rows (32- and 64-bit pixels).  Every lane of the plane gets here, so the exchanges are whole.
    uint32_t box[2][(2 * NPT * BPP + 3) / 4];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        uint32_t mine[NWT], right[NWT];
#pragma unroll
        for (int i = 0; i < NWT; ++i) {
            uint32_t v = top[j][i];
            if constexpr (G::NL == 3) {
                if (j == 1) v = (uint32_t)__shfl_xor((int)v, 32);
            }
            mine[i] = v;
            right[i] = (uint32_t)__shfl_xor((int)v, 1);
        }
#pragma unroll
        for (int i = 0; i < (2 * NPT * BPP + 3) / 4; ++i) box[j][i] = 0;
#pragma unroll
        for (int i = 0; i < NPT; ++i) {
            px_set<BPP>(box[j], i, px_get<BPP>(mine, i));
            px_set<BPP>(box[j], NPT + i, px_get<BPP>(right, i));
        }
    }
    uint32_t ox[1][NWT];
    reduce_piece<BPP, OP, 1, NPT>(box, ox);
    swap_words<BPP, BE>(ox[0]);
    const bool owner = (lane & 1u) == 0 && (G::NL == 2 || lane < 32u);
    if (owner)
        store_piece<BPP, 1, NPT>(A.dst[G::NL] + plane * A.dst_plane[G::NL], A.w[G::NL], A.h[G::NL], x0 >> (G::NL + 1),
                                 y0 >> (G::NL + 1), ox, false);
}

template <int BPP, bool BE, typename OP>
static void launch_pyramid_k(dim3 g, hipStream_t st, const PyrArgs& a) {
    omr_launch(k_pyramid<BPP, BE, OP>, g, dim3(256), 0u, st, a);
}

template <bool BE>
static void launch_pyramid_mean(dim3 g, hipStream_t st, const PyrArgs& a, int32_t pt) {
    switch (pt) {
    case OMR_PIXELS_INT8: launch_pyramid_k<1, false, PyrMean<int8_t>>(g, st, a); break;
    case OMR_PIXELS_UINT8: launch_pyramid_k<1, false, PyrMean<uint8_t>>(g, st, a); break;
    case OMR_PIXELS_INT16: launch_pyramid_k<2, BE, PyrMean<int16_t>>(g, st, a); break;
    case OMR_PIXELS_UINT16: launch_pyramid_k<2, BE, PyrMean<uint16_t>>(g, st, a); break;
    case OMR_PIXELS_INT32: launch_pyramid_k<4, BE, PyrMean<int32_t>>(g, st, a); break;
    case OMR_PIXELS_UINT32: launch_pyramid_k<4, BE, PyrMean<uint32_t>>(g, st, a); break;
    case OMR_PIXELS_FLOAT: launch_pyramid_k<4, BE, PyrMean<float>>(g, st, a); break;
    default: launch_pyramid_k<8, BE, PyrMean<double>>(g, st, a); break;
    }
}

static int pyr_lane_levels(int bpp) { return bpp <= 2 ? 3 : 2; }            // levels a lane makes alone
static int pyr_levels_per_launch(int bpp) { return pyr_lane_levels(bpp) + 1; }   // and one across lanes
static int pyr_lane_px(int bpp) { return bpp == 8 ? 4 : 16 / bpp; }

bool pyramid_levels_valid(int64_t w, int64_t h, int64_t n_levels) {
    if (w < 1 || h < 1 || n_levels < 1 || n_levels > OMR_PYRAMID_MAX_LEVELS) return false;
    return (std::min(w, h) >> (n_levels - 1)) >= 1;      // n_levels <= 1 + floor(log2(min(w, h)))
}

// One launch: levels k0 .. k0+nl-1 (sizes lw/lh, bases dst) from n source planes of W x H.
static omr_status enqueue_pyramid(Ctx* ctx, const uint8_t* const* src, int32_t n, int32_t pt, bool be, int32_t W,
                                  int32_t H, int64_t row_stride_px, int32_t rule, int32_t nl, uint8_t* const* dst) {
    const int bpp = bytes_per_pixel(pt), px = pyr_lane_px(bpp);
    PyrArgs a;
    std::memset(&a, 0, sizeof(a));
    a.row_stride = row_stride_px * bpp;
    a.W = W; a.H = H;
    a.nl = nl;
    bool vec = a.row_stride % 16 == 0;
    for (int p = 0; p < n; ++p) {
        a.src[p] = src[p];
        vec = vec && (uintptr_t)src[p] % 16 == 0;
    }
    for (int k = 0; k < nl; ++k) {
        a.w[k] = W >> (k + 1);
        a.h[k] = H >> (k + 1);
        a.dst[k] = dst[k];
        a.dst_plane[k] = (int64_t)a.w[k] * a.h[k] * bpp;
        // a lane's piece of level k+1 is px >> (k+1) pixels wide: every row of every plane must
        // start on a multiple of that store (the level made across lanes is stored pixel by pixel)
        if (k < pyr_lane_levels(bpp)) {
            const int64_t piece = (int64_t)(px >> (k + 1)) * bpp;
            vec = vec && (uintptr_t)dst[k] % 16 == 0 && ((int64_t)a.w[k] * bpp) % piece == 0;
        }
    }
    a.vec = vec ? 1 : 0;
    a.CW = (uint32_t)((W + px - 1) / px);
    a.CHR = (uint32_t)((H + kPyrRows - 1) / kPyrRows);
    a.WC = (a.CW + 31u) / 32u;
    a.waves = a.WC * ((a.CHR + 1u) / 2u);                            // < W*H < 2^31
    a.divWC = make_fastdiv(a.WC);
    const dim3 g((a.waves + 3u) / 4u, (unsigned)n);
    KernelTimer timer(ctx, kKindPyramid, true);
    if (rule == OMR_PYRAMID_SUBSAMPLE) {
        switch (bpp) {
        case 1: launch_pyramid_k<1, false, PyrSub>(g, ctx->stream, a); break;
        case 2: launch_pyramid_k<2, false, PyrSub>(g, ctx->stream, a); break;
        case 4: launch_pyramid_k<4, false, PyrSub>(g, ctx->stream, a); break;
        default: launch_pyramid_k<8, false, PyrSub>(g, ctx->stream, a); break;
        }
    } else if (be) {
        launch_pyramid_mean<true>(g, ctx->stream, a, pt);
    } else {
        launch_pyramid_mean<false>(g, ctx->stream, a, pt);
    }
    OMR_HIP(ctx, hipGetLastError());
    return OMR_OK;
}

}  // namespace omr

using namespace omr;

extern "C" {

int32_t omr_pyramid_level_count(int32_t size_x, int32_t size_y, int32_t min_side) {
    if (size_x < 1 || size_y < 1 || min_side < 1) return -(int32_t)OMR_INVALID_ARGUMENT;
    int32_t n = 1;
    while (std::max(size_x >> (n - 1), size_y >> (n - 1)) > min_side && pyramid_levels_valid(size_x, size_y, n + 1))
        ++n;
    return n;
}

omr_status omr_pyramid_level_sizes(int32_t size_x, int32_t size_y, int32_t n_levels, int32_t* sizes_out) {
    if (!sizes_out || !pyramid_levels_valid(size_x, size_y, n_levels)) return OMR_INVALID_ARGUMENT;
    for (int k = 0; k < n_levels; ++k) {
        sizes_out[2 * k] = size_x >> k;
        sizes_out[2 * k + 1] = size_y >> k;
    }
    return OMR_OK;
}

omr_status omr_pyramid_build_device(omr_ctx* ctx, const void* const* d_planes, int32_t n_planes, int32_t pixel_type,
                                    int32_t big_endian, int32_t width, int32_t height, int64_t row_stride_px,
                                    int32_t rule, int32_t n_levels, void* const* d_levels_out) {
    if (!ctx) return OMR_INVALID_ARGUMENT;
    const int bpp = bytes_per_pixel(pixel_type);
    if (!bpp) return fail(ctx, OMR_INVALID_ARGUMENT, "pyramid: unknown pixel type");
    if (rule != OMR_PYRAMID_SUBSAMPLE && rule != OMR_PYRAMID_MEAN)
        return fail(ctx, OMR_INVALID_ARGUMENT, "pyramid: unknown rule");
    if (n_planes < 1 || n_planes > kPyrMaxPlanes) return fail(ctx, OMR_INVALID_ARGUMENT, "pyramid: n_planes outside 1..32");
    if (width < 1 || height < 1) return fail(ctx, OMR_INVALID_ARGUMENT, "pyramid: empty plane");
    if ((int64_t)width * height >= ((int64_t)1 << 31))
        return fail(ctx, OMR_INVALID_ARGUMENT, "pyramid: plane of 2^31 pixels or more");
    if (!pyramid_levels_valid(width, height, n_levels))
        return fail(ctx, OMR_INVALID_ARGUMENT, "pyramid: n_levels outside 1..min(16, 1 + floor(log2(min(width, height))))");
    if (row_stride_px == 0) row_stride_px = width;
    if (row_stride_px < width) return fail(ctx, OMR_INVALID_ARGUMENT, "row stride smaller than width");
    if (!d_planes) return fail(ctx, OMR_INVALID_ARGUMENT, "pyramid: null plane table");
    for (int p = 0; p < n_planes; ++p)
        if (!d_planes[p] || (uintptr_t)d_planes[p] % (uintptr_t)bpp)
            return fail(ctx, OMR_INVALID_ARGUMENT, "pyramid: plane pointer null or not a multiple of the pixel size");
    if (n_levels > 1 && !d_levels_out) return fail(ctx, OMR_INVALID_ARGUMENT, "pyramid: null level table");
    for (int k = 1; k < n_levels; ++k)
        if (!d_levels_out[k - 1] || (uintptr_t)d_levels_out[k - 1] % (uintptr_t)bpp)
            return fail(ctx, OMR_INVALID_ARGUMENT, "pyramid: level pointer null or not a multiple of the pixel size");
    if (n_levels == 1) return OMR_OK;
    OMR_HIP(ctx, hipSetDevice(ctx->device));
    const uint8_t* src[kPyrMaxPlanes];
    for (int p = 0; p < n_planes; ++p) src[p] = static_cast<const uint8_t*>(d_planes[p]);
    int32_t W = width, H = height;
    const int per = pyr_levels_per_launch(bpp);
    for (int k = 1; k < n_levels;) {
        const int nl = std::min(per, n_levels - k);
        uint8_t* dst[kPyrMaxLaunchLevels] = {nullptr, nullptr, nullptr, nullptr};
        for (int i = 0; i < nl; ++i) dst[i] = static_cast<uint8_t*>(d_levels_out[k - 1 + i]);
        const omr_status st = enqueue_pyramid(ctx, src, n_planes, pixel_type, big_endian != 0, W, H, row_stride_px, rule,
                                              nl, dst);
        if (st) return st;
        // the next launch reads the last level written (packed)
        k += nl;
        W = width >> (k - 1);
        H = height >> (k - 1);
        row_stride_px = W;
        const int64_t pb = (int64_t)W * H * bpp;
        for (int p = 0; p < n_planes; ++p) src[p] = dst[nl - 1] + pb * p;
    }
    return OMR_OK;
}

}  // extern "C"
