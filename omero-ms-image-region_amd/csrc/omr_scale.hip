// omr_scale.hip — K10: scaled rendering (thumbnails, bird's-eye views).
//
// The rule (include/omr/omr.h, DESIGN.md §4 "K10 scaled render"): an exact area-weighted mean in
// integers, rounded half up.  In units of 1/tw a source column x covers [x*tw, (x+1)*tw) and an
// output column i covers [i*W, (i+1)*W); wx[i][x] is the length of their overlap (0..tw), wy the
// same from H and th, and per ARGB byte
//     out[j][i] = (sum_y sum_x wy[j][y] * wx[i][x] * src[y][x] + (W*H)/2) / (W*H).
// Every sum is an integer and order-free, so the result does not depend on scheduling.
//
//   k_scale_argb     the rule on ARGB in HBM (omr_scale_argb_device, and the unfused route
//                    K2 -> aux -> k_scale_argb of the scaled render)
//   k_render_scale   quantize + composite (K2's helpers, omr_k2.h) + reduce in one pass: the
//                    full-size ARGB never reaches HBM
#include "omr_k2.h"

#include <memory>

namespace omr {

constexpr int kKindRenderScale = 10;   // omr_ctx_kernel_timings kinds
constexpr int kKindScaleArgb = 11;

constexpr int kScaleChunk = 8;         // pixels a lane owns per row (16 B of 16-bit, 8 B of 8-bit pixels)
constexpr int kScaleMaxOutW = 1024;    // fused: out_w limit (LDS accumulators [out_w][3], weights in 11 bits)

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// Overlap of source cell s (length t, at s*t) with output cell o (length S, at o*S): 0..t.
__device__ __forceinline__ uint32_t overlap(int64_t o, int64_t S, int64_t s, int64_t t) {
    const int64_t lo = max(o * S, s * t), hi = min((o + 1) * S, (s + 1) * t);
    return (uint32_t)max(hi - lo, (int64_t)0);
}

template <typename ACC>
__device__ __forceinline__ ACC group16_sum(ACC v) {
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) {
        if constexpr (sizeof(ACC) == 8) {
            const uint32_t lo = __shfl_xor((uint32_t)v, m), hi = __shfl_xor((uint32_t)(v >> 32), m);
            v += ((uint64_t)hi << 32) | lo;
        } else {
            v += __shfl_xor(v, m);
        }
    }
    return v;
}

struct ScaleArgbArgs {
    const uint32_t* src;      // [n][H][row_stride]
    uint32_t* dst;            // [n][th][tw]
    int64_t row_stride, image_stride;   // pixels
    int64_t total;            // n * th * tw output pixels
    int32_t W, H, tw, th;
};

// 16 lanes per output pixel (2 rows x 8 columns of its source box per step), 16 output pixels per
// workgroup; the lanes' partial sums meet in a 16-lane butterfly.  ACC: uint32_t when
// 255*W*H + W*H/2 < 2^32, uint64_t above.
template <typename ACC>
__global__ void __launch_bounds__(256) k_scale_argb(const ScaleArgbArgs A) {
    const int l = threadIdx.x & 15, ly = l >> 3, lx = l & 7;
    const int64_t pix = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    const bool valid = pix < A.total;
    const int64_t W = A.W, H = A.H, tw = A.tw, th = A.th;
    const int64_t q = valid ? pix / tw : 0;
    const int64_t i = valid ? pix - q * tw : 0;
    const int64_t img = q / th, j = q - img * th;
    const int64_t xlo = i * W / tw, xhi = valid ? ((i + 1) * W + tw - 1) / tw : xlo;
    const int64_t ylo = j * H / th, yhi = valid ? ((j + 1) * H + th - 1) / th : ylo;
    const uint32_t* const base = A.src + img * A.image_stride;
    ACC s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    for (int64_t y = ylo + ly; y < yhi; y += 2) {
        const uint32_t wy = overlap(j, H, y, th);
        const uint32_t* const row = base + y * A.row_stride;
        for (int64_t x = xlo + lx; x < xhi; x += 8) {
            const ACC w = (ACC)wy * (ACC)overlap(i, W, x, tw);     // <= tw*th <= W*H < 2^31
            const uint32_t p = row[x];
            s0 += w * (ACC)(p & 0xFFu);
            s1 += w * (ACC)((p >> 8) & 0xFFu);
            s2 += w * (ACC)((p >> 16) & 0xFFu);
            s3 += w * (ACC)(p >> 24);
        }
    }
    s0 = group16_sum(s0); s1 = group16_sum(s1); s2 = group16_sum(s2); s3 = group16_sum(s3);
    if (valid && l == 0) {
        const ACC wh = (ACC)(W * H), half = wh / 2;
        A.dst[pix] = (uint32_t)((s0 + half) / wh) | ((uint32_t)((s1 + half) / wh) << 8) |
                     ((uint32_t)((s2 + half) / wh) << 16) | ((uint32_t)((s3 + half) / wh) << 24);
    }
}

// ---- the fused kernel -------------------------------------------------------------------------
struct RenderScaleArgs {
    FusedRender R;
    const uint8_t* sbase;        // strided batches: plane(t, c) = sbase + t*tile_stride + c*chan_stride
    const void* const* planes;   // pointer-table batches: planes[t*size_c + c]
    int64_t tile_stride, chan_stride, row_stride;   // bytes, bytes, pixels
    int32_t strided, size_c, flip_h, flip_v;
    int32_t W, H, tw, th;
    int32_t k;                   // output rows per workgroup (a band)
    int32_t C;                   // 8-pixel chunks per source row
    int32_t G;                   // C < 256: 256 / C lane groups share a band's source rows; else 1
    FastDiv divW;                // x*tw / W (the host keeps W*tw below 2^31)
    uint32_t* out;               // [n][th][tw]
    int32_t* status;             // optional [n]: OMR_QUANTIZATION for an image with a pixel outside its LUT domain
};

// A workgroup owns output rows [blockIdx.x*k, +k) of image blockIdx.y and walks them one at a
// time.  For output row j a lane keeps one 8-pixel column chunk and sums wy * (r, g, b) of its
// eight pixels over the source rows of j it is dealt (registers, 32 bits: at most 255*H); the
// source row two output rows share is read for both, each with its own wy.  Once per output row
// the lane folds its eight pixel sums with wx into the one or two output columns each pixel
// overlaps (consecutive pixels of one column first, in registers) and adds them to the row's LDS
// accumulators [tw][3] (ACC: uint32_t when 255*W*H + W*H/2 < 2^32, uint64_t above); after a
// barrier the lanes divide, round and store at the flipped position.  Integer sums: the LDS add
// order does not change a bit.
template <int BPP, bool BE, int MODE, int NA, typename ACC>
__global__ void __launch_bounds__(256) k_render_scale(const RenderScaleArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_mem[];
    uint32_t* const s_contrib = s_mem;                                          // [NA][256]
    ACC* const s_acc = reinterpret_cast<ACC*>(s_mem + kFusedMaxActive * 256);   // [tw][3]
    for (int i = threadIdx.x; i < NA * 256; i += 256) s_contrib[i] = A.R.contrib[i];
    const int tile = blockIdx.y;
    const int W = A.W, H = A.H, tw = A.tw, th = A.th, C = A.C, G = A.G;
    const uint8_t* base[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) {
        const int c = A.R.ch[a].index;
        base[a] = A.strided ? A.sbase + (int64_t)tile * A.tile_stride + (int64_t)c * A.chan_stride
                            : static_cast<const uint8_t*>(A.planes[(int64_t)tile * A.size_c + c]);
    }
    // C >= 256: lane t walks chunk columns t, t + 256, ... over every source row; C < 256: lane
    // group g = t / C takes the rows ylo + g, ylo + g + G, ... of chunk column t % C
    const int grp = C >= 256 ? 0 : (int)threadIdx.x / C;
    const int c_first = C >= 256 ? (int)threadIdx.x : (int)threadIdx.x - grp * C;
    const bool active = grp < G;
    const uint32_t sg = (BPP == 2 && A.R.is_signed) ? 0x80008000u : 0u;   // int16 biased to unsigned (host: + 32768)
    bool err = false;
    const int j_end = min((int)(blockIdx.x + 1) * A.k, th);
    for (int j = blockIdx.x * A.k; j < j_end; ++j) {
        for (int i = threadIdx.x; i < tw * 3; i += 256) s_acc[i] = 0;
        __syncthreads();                                  // (first trip: the tables too)
        const int ylo = (int)((int64_t)j * H / th), yhi = (int)((((int64_t)j + 1) * H + th - 1) / th);
        for (int c = c_first; active && c < C; c += 256) {
            // wx of this chunk's pixels: w0 into the column the pixel starts in, tw - w0 into the
            // next; bit 16: the next pixel starts in the next column
            uint32_t wpk[kScaleChunk];
            const uint32_t xt0 = (uint32_t)c * kScaleChunk * (uint32_t)tw;
            const int col0 = (int)fdiv(xt0, A.divW);
#pragma unroll
            for (int p = 0; p < kScaleChunk; ++p) {
                const uint32_t xt = xt0 + (uint32_t)p * (uint32_t)tw;
                const uint32_t edge = (fdiv(xt, A.divW) + 1u) * (uint32_t)W;    // <= W*tw
                const uint32_t w0 = min(edge, xt + (uint32_t)tw) - xt;
                wpk[p] = w0 | (xt + (uint32_t)tw >= edge ? 0x10000u : 0u);
            }
            uint32_t acc[kScaleChunk][3];
#pragma unroll
            for (int p = 0; p < kScaleChunk; ++p) acc[p][0] = acc[p][1] = acc[p][2] = 0;
            for (int y = ylo + grp; y < yhi; y += G) {
                const uint32_t wy = overlap(j, H, y, th);
                // 32-bit byte offsets from the uniform plane base (the host keeps a plane below 4 GiB)
                const uint32_t off = ((uint32_t)y * (uint32_t)A.row_stride + (uint32_t)c * kScaleChunk) * BPP;
                uint32_t raw[NA][4];
#pragma unroll
                for (int a = 0; a < NA; ++a) {
                    if constexpr (BPP == 2) {
                        const u32x4 v = ld_global<u32x4>(base[a] + off);
                        raw[a][0] = v[0]; raw[a][1] = v[1]; raw[a][2] = v[2]; raw[a][3] = v[3];
                    } else {
                        const u32x2 v = ld_global<u32x2>(base[a] + off);
                        raw[a][0] = v[0]; raw[a][1] = v[1]; raw[a][2] = raw[a][3] = 0;
                    }
                }
                uint32_t e[kScaleChunk];
#pragma unroll
                for (int p = 0; p < kScaleChunk; ++p) e[p] = 0;
#pragma unroll
                for (int a = 0; a < NA; ++a) {
                    const uint32_t* tab = s_contrib + a * 256;
                    const K2Chan& ch = A.R.ch[a];
                    if constexpr (BPP == 1) {
#pragma unroll
                        for (int p = 0; p < kScaleChunk; ++p) {
                            const uint32_t t = tab[(raw[a][p >> 2] >> (8 * (p & 3))) & 0xFFu];
                            err |= (t & kErrBit) != 0;
                            e[p] += t & ~kErrBit;
                        }
                    } else {
#pragma unroll
                        for (int d = 0; d < 4; ++d) {
                            uint32_t w = raw[a][d];
                            if constexpr (BE) w = bswap16x2(w);
                            w ^= sg;
                            if (A.R.any_check && ch.check) {     // uniform: QuantizationException, as F1
                                const uint32_t hi2 = A.R.dhi2[a], lo2 = A.R.dlo2[a];
                                err |= ((pk_max_u16(w, hi2) ^ hi2) | (pk_min_u16(w, lo2) ^ lo2)) != 0;
                            }
#pragma unroll
                            for (int h = 0; h < 2; ++h) {
                                const int x = (int)(h ? (w >> 16) : (w & 0xFFFFu));
                                uint32_t v;
                                if constexpr (MODE == kFusedFast16) {
                                    v = fast16(x, ch);
                                } else if constexpr (MODE == kFusedFast16I) {
                                    v = fast16i(x, ch);
                                } else if constexpr (MODE == kFusedFast16F) {
                                    v = fast16f(x, ch.wsi, A.R.fa[a], A.R.fb[a]);
                                } else if (MODE == kFusedLinear16 || ch.mode == kModeLinear16) {   // uniform
                                    v = linear16(x, ch, A.R.cd_start, A.R.cds8, A.R.cde8);
                                } else {
                                    const int xi = min(max(x, ch.gmin), ch.gmax);
                                    v = reinterpret_cast<const uint8_t*>(ch.lut_addr)[(uint32_t)(xi - ch.gmin)];
                                }
                                e[2 * d + h] += tab[v];
                            }
                        }
                    }
                }
#pragma unroll
                for (int p = 0; p < kScaleChunk; ++p) {
                    const uint32_t f = clamp_fields(e[p]);       // K2's composite: 10-bit sums, clamped
                    acc[p][0] += wy * (f >> 20);
                    acc[p][1] += wy * ((f >> 10) & 0xFFu);
                    acc[p][2] += wy * (f & 0xFFu);
                }
            }
            // fold with wx: pixels of one output column first, then one LDS add per column
            ACC run[3] = {0, 0, 0};
            int col = col0;
#pragma unroll
            for (int p = 0; p < kScaleChunk; ++p) {
                const uint32_t w0 = wpk[p] & 0xFFFFu;
#pragma unroll
                for (int k = 0; k < 3; ++k) run[k] += (ACC)w0 * (ACC)acc[p][k];
                if ((wpk[p] >> 16) || p == kScaleChunk - 1) {
                    if (col < tw) {
#pragma unroll
                        for (int k = 0; k < 3; ++k) atomicAdd(&s_acc[col * 3 + k], run[k]);
                    }
                    const uint32_t w1 = (uint32_t)tw - w0;
#pragma unroll
                    for (int k = 0; k < 3; ++k) run[k] = (ACC)w1 * (ACC)acc[p][k];
                    ++col;
                }
            }
            if ((wpk[kScaleChunk - 1] & 0xFFFFu) < (uint32_t)tw && col < tw) {   // the last pixel's second column
#pragma unroll
                for (int k = 0; k < 3; ++k) atomicAdd(&s_acc[col * 3 + k], run[k]);
            }
        }
        __syncthreads();
        const ACC wh = (ACC)((int64_t)W * H), half = wh / 2;
        const int orow = A.flip_v ? th - 1 - j : j;
        uint32_t* const orow_p = A.out + ((int64_t)tile * th + orow) * tw;
        for (int i = threadIdx.x; i < tw; i += 256) {
            const uint32_t r = (uint32_t)((s_acc[i * 3] + half) / wh), g = (uint32_t)((s_acc[i * 3 + 1] + half) / wh),
                           b = (uint32_t)((s_acc[i * 3 + 2] + half) / wh);
            orow_p[A.flip_h ? tw - 1 - i : i] = 0xFF000000u | (r << 16) | (g << 8) | b;
        }
        __syncthreads();                                  // the accumulators are cleared next
    }
    if constexpr (BPP == 2) err |= A.R.dnone != 0;        // a domain that holds no 16-bit value
    if (__ballot(err)) {
        if ((threadIdx.x & 63) == 0) {
            atomicOr(A.R.flag, 1);
            if (A.status) A.status[tile] = OMR_QUANTIZATION;
        }
    }
}

template <int BPP, bool BE, int MODE, typename ACC>
static void launch_render_scale_na(dim3 g, uint32_t lds, hipStream_t st, const RenderScaleArgs& a) {
    switch (a.R.n_active) {
    case 1: omr_launch(k_render_scale<BPP, BE, MODE, 1, ACC>, g, dim3(256), lds, st, a); break;
    case 2: omr_launch(k_render_scale<BPP, BE, MODE, 2, ACC>, g, dim3(256), lds, st, a); break;
    case 3: omr_launch(k_render_scale<BPP, BE, MODE, 3, ACC>, g, dim3(256), lds, st, a); break;
    default: omr_launch(k_render_scale<BPP, BE, MODE, 4, ACC>, g, dim3(256), lds, st, a); break;
    }
}

template <bool BE, typename ACC>
static void launch_render_scale_mode(dim3 g, uint32_t lds, hipStream_t st, const RenderScaleArgs& a) {
    switch (a.R.mode) {
    case kFusedFast16:
        if (a.R.f32) launch_render_scale_na<2, BE, kFusedFast16F, ACC>(g, lds, st, a);
        else if (a.R.ws_int) launch_render_scale_na<2, BE, kFusedFast16I, ACC>(g, lds, st, a);
        else launch_render_scale_na<2, BE, kFusedFast16, ACC>(g, lds, st, a);
        break;
    case kFusedLinear16: launch_render_scale_na<2, BE, kFusedLinear16, ACC>(g, lds, st, a); break;
    default: launch_render_scale_na<2, BE, kFusedMixed16, ACC>(g, lds, st, a); break;
    }
}

template <typename ACC>
static void launch_render_scale(dim3 g, uint32_t lds, hipStream_t st, const RenderScaleArgs& a, int bpp, bool be) {
    if (bpp == 1) launch_render_scale_na<1, false, kFusedTable8, ACC>(g, lds, st, a);
    else if (be) launch_render_scale_mode<true, ACC>(g, lds, st, a);
    else launch_render_scale_mode<false, ACC>(g, lds, st, a);
}

// 32-bit accumulators hold the largest sum plus the rounding term: 255*W*H + W*H/2 < 2^32.
static bool scale_acc32(int64_t W, int64_t H) { return 255 * W * H + W * H / 2 < ((int64_t)1 << 32); }

static omr_status check_scale_dims(Ctx* ctx, int64_t W, int64_t H, int64_t tw, int64_t th) {
    if (W < 1 || H < 1) return fail(ctx, OMR_INVALID_ARGUMENT, "scale: empty source");
    if (W * H >= ((int64_t)1 << 31)) return fail(ctx, OMR_INVALID_ARGUMENT, "scale: source plane of 2^31 pixels or more");
    if (tw < 1 || th < 1 || tw > W || th > H)
        return fail(ctx, OMR_INVALID_ARGUMENT, "scale: output size must be 1..source size (no upscaling)");
    return OMR_OK;
}

static omr_status enqueue_scale_argb(Ctx* ctx, const uint32_t* d_src, int32_t n, int32_t W, int32_t H, int64_t row_stride,
                                     int64_t image_stride, uint32_t* d_dst, int32_t tw, int32_t th) {
    ScaleArgbArgs a;
    a.src = d_src;
    a.dst = d_dst;
    a.row_stride = row_stride;
    a.image_stride = image_stride;
    a.total = (int64_t)n * tw * th;
    a.W = W; a.H = H; a.tw = tw; a.th = th;
    const int64_t blocks = (a.total + 15) / 16;
    if (blocks >= ((int64_t)1 << 31)) return fail(ctx, OMR_INVALID_ARGUMENT, "scale: batch too large for one launch");
    KernelTimer timer(ctx, kKindScaleArgb, true);
    if (scale_acc32(W, H)) omr_launch(k_scale_argb<uint32_t>, dim3((unsigned)blocks), dim3(256), 0u, ctx->stream, a);
    else omr_launch(k_scale_argb<uint64_t>, dim3((unsigned)blocks), dim3(256), 0u, ctx->stream, a);
    OMR_HIP(ctx, hipGetLastError());
    return OMR_OK;
}

omr_status render_scaled(Ctx* ctx, const omr_quantum_def* qdef, const omr_channel_binding* channels, int32_t size_c,
                         const void* d_base, int64_t tile_stride, int64_t chan_stride, const void* const* d_ptrs,
                         int32_t n, int64_t row_stride, int32_t pt, int32_t be, int32_t W, int32_t H, int32_t fh,
                         int32_t fv, uint32_t* d_out, int32_t* d_status, int32_t tw, int32_t th, const ScaledAux* aux) {
    if (!ctx) return OMR_INVALID_ARGUMENT;
    if (n < 1) return fail(ctx, OMR_INVALID_ARGUMENT, "scaled render: n_tiles < 1");
    omr_status st = check_scale_dims(ctx, W, H, tw, th);
    if (st) return st;
    if (!d_base && !d_ptrs) return fail(ctx, OMR_INVALID_ARGUMENT, "null plane batch");
    if (!d_out && !aux) return fail(ctx, OMR_INVALID_ARGUMENT, "null output");
    if (row_stride == 0) row_stride = W;
    if (row_stride < W) return fail(ctx, OMR_INVALID_ARGUMENT, "row stride smaller than width");
    OMR_HIP(ctx, hipSetDevice(ctx->device));
    // aux: the small ARGB and the statuses go to the front of the context's aux buffer (the
    // thumbnail JPEG path), the unfused route's full-size ARGB behind them
    const size_t aux_front = aux ? aux->total : 0;
    auto aux_outputs = [&]() {
        if (!aux) return;
        d_out = static_cast<uint32_t*>(ctx->aux);
        d_status = reinterpret_cast<int32_t*>(static_cast<uint8_t*>(ctx->aux) + aux->status_off);
    };
    omr_ctx* cx = static_cast<omr_ctx*>(ctx);
    const int bpp = bytes_per_pixel(pt);
    bool fused = false;
    std::unique_ptr<FusedPlanBuf, void (*)(FusedPlanBuf*)> fp(fused_plan_new(), fused_plan_free);
    if (ctx->scale_fused) {
        fused = render_fused_plan(ctx, qdef, channels, size_c, pt, fp.get(), &st);
        if (st) return st;
        // whole, aligned 8-pixel chunks per row: 16 bytes of 16-bit pixels, 8 bytes of 8-bit ones
        // (pointer-table planes: the caller's contract, as for omr_render_batch_device); 32-bit byte
        // offsets inside a plane; the per-lane weights (x*tw in 32 bits, 11-bit w0) and the LDS
        // accumulators bound out_w; 255*H in a register sum
        const int64_t cb = (int64_t)kScaleChunk * bpp;
        fused = fused && W % kScaleChunk == 0 && (row_stride * bpp) % cb == 0 &&
                (!d_base || ((uintptr_t)d_base % cb == 0 && tile_stride % cb == 0 && chan_stride % cb == 0)) &&
                (row_stride * (int64_t)(H - 1) + W) * bpp < ((int64_t)1 << 32) && tw <= kScaleMaxOutW &&
                (int64_t)W * tw < ((int64_t)1 << 31) && H <= (1 << 24);
    }
    if (fused) {
        st = ensure_workspace(ctx, render_fused_ws_bytes(fp.get()));
        if (st) return st;
        if (aux) {
            st = ensure_aux(ctx, aux_front);
            if (st) return st;
            aux_outputs();
        }
        if (d_status) OMR_HIP(ctx, hipMemsetAsync(d_status, 0, sizeof(int32_t) * (size_t)n, ctx->stream));
        RenderScaleArgs a;
        std::memset(&a, 0, sizeof(a));
        st = render_fused_stage(ctx, fp.get(), 0, a.R, /*build_contrib=*/true, /*bias_int16=*/true);
        if (st) return st;
        a.sbase = static_cast<const uint8_t*>(d_base);
        a.planes = d_ptrs;
        a.strided = d_base ? 1 : 0;
        a.tile_stride = tile_stride;
        a.chan_stride = chan_stride;
        a.row_stride = row_stride;
        a.size_c = size_c;
        a.flip_h = fh ? 1 : 0;
        a.flip_v = fv ? 1 : 0;
        a.W = W; a.H = H; a.tw = tw; a.th = th;
        a.C = W / kScaleChunk;
        a.G = a.C >= 256 ? 1 : 256 / a.C;
        a.divW = make_fastdiv((uint32_t)W);
        // rows per band: one image still spreads over the device (k = 1 below ~8 workgroups per
        // CU); a large batch amortises the table staging over more rows
        a.k = (int32_t)std::min<int64_t>(th, std::max<int64_t>(1, (int64_t)n * th / (8 * (int64_t)ctx->cu_count)));
        a.out = d_out;
        a.status = d_status;
        const bool a32 = scale_acc32(W, H);
        const uint32_t lds = kFusedMaxActive * 256 * 4 + (uint32_t)tw * 3 * (a32 ? 4 : 8);
        const dim3 g((unsigned)((th + a.k - 1) / a.k), (unsigned)n);
        KernelTimer timer(ctx, kKindRenderScale, true);
        if (a32) launch_render_scale<uint32_t>(g, lds, ctx->stream, a, bpp, be != 0);
        else launch_render_scale<uint64_t>(g, lds, ctx->stream, a, bpp, be != 0);
        OMR_HIP(ctx, hipGetLastError());
        return OMR_OK;
    }
    // unfused: K2 at full size into the context's aux buffer, then the rule on that ARGB
    st = ensure_aux(ctx, aux_front + (size_t)n * W * H * 4);
    if (st) return st;
    aux_outputs();
    uint32_t* argb = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(ctx->aux) + aux_front);
    st = d_base ? omr_render_batch_strided_device(cx, qdef, channels, size_c, d_base, tile_stride, chan_stride, n,
                                                  row_stride, pt, be, W, H, fh, fv, argb, d_status)
                : omr_render_batch_device(cx, qdef, channels, size_c, d_ptrs, n, row_stride, pt, be, W, H, fh, fv, argb,
                                          d_status);
    if (st) return st;
    return enqueue_scale_argb(ctx, argb, n, W, H, W, (int64_t)W * H, d_out, tw, th);
}

}  // namespace omr

using namespace omr;

extern "C" {

omr_status omr_thumbnail_size(int32_t size_x, int32_t size_y, int32_t longest_side, int32_t* out_w, int32_t* out_h) {
    if (size_x < 1 || size_y < 1 || longest_side < 1 || !out_w || !out_h) return OMR_INVALID_ARGUMENT;
    const int64_t big = std::max(size_x, size_y), small = std::min(size_x, size_y);
    int64_t lw = big, sw = small;
    if (big > longest_side) {
        lw = longest_side;
        sw = std::max<int64_t>(1, small * (int64_t)longest_side / big);
    }
    *out_w = (int32_t)(size_x >= size_y ? lw : sw);
    *out_h = (int32_t)(size_x >= size_y ? sw : lw);
    return OMR_OK;
}

omr_status omr_scale_argb_device(omr_ctx* ctx, const uint32_t* d_src, int32_t n, int32_t src_w, int32_t src_h,
                                 int64_t src_row_stride_px, int64_t src_image_stride_px, uint32_t* d_dst,
                                 int32_t dst_w, int32_t dst_h) {
    if (!ctx) return OMR_INVALID_ARGUMENT;
    if (n < 1) return fail(ctx, OMR_INVALID_ARGUMENT, "scale: n < 1");
    omr_status st = check_scale_dims(ctx, src_w, src_h, dst_w, dst_h);
    if (st) return st;
    if (!d_src || !d_dst) return fail(ctx, OMR_INVALID_ARGUMENT, "scale: null buffer");
    if (src_row_stride_px == 0) src_row_stride_px = src_w;
    if (src_row_stride_px < src_w) return fail(ctx, OMR_INVALID_ARGUMENT, "row stride smaller than width");
    if (src_image_stride_px == 0) src_image_stride_px = src_row_stride_px * src_h;
    if (src_image_stride_px < src_row_stride_px * (int64_t)(src_h - 1) + src_w)
        return fail(ctx, OMR_INVALID_ARGUMENT, "scale: image stride smaller than an image");
    OMR_HIP(ctx, hipSetDevice(ctx->device));
    return enqueue_scale_argb(ctx, d_src, n, src_w, src_h, src_row_stride_px, src_image_stride_px, d_dst, dst_w, dst_h);
}

omr_status omr_render_scaled_batch_device(omr_ctx* ctx, const omr_quantum_def* qdef,
                                          const omr_channel_binding* channels, int32_t size_c,
                                          const void* const* d_plane_ptrs, int32_t n_tiles, int64_t row_stride,
                                          int32_t pixel_type, int32_t big_endian, int32_t width, int32_t height,
                                          int32_t flip_h, int32_t flip_v, uint32_t* d_argb_out, int32_t* d_status,
                                          int32_t out_w, int32_t out_h) {
    if (!d_plane_ptrs) return ctx ? fail(ctx, OMR_INVALID_ARGUMENT, "null plane table") : OMR_INVALID_ARGUMENT;
    return render_scaled(ctx, qdef, channels, size_c, nullptr, 0, 0, d_plane_ptrs, n_tiles, row_stride, pixel_type,
                         big_endian, width, height, flip_h, flip_v, d_argb_out, d_status, out_w, out_h, nullptr);
}

omr_status omr_render_scaled_batch_strided_device(omr_ctx* ctx, const omr_quantum_def* qdef,
                                                  const omr_channel_binding* channels, int32_t size_c,
                                                  const void* d_base, int64_t tile_stride_bytes,
                                                  int64_t channel_stride_bytes, int32_t n_tiles, int64_t row_stride,
                                                  int32_t pixel_type, int32_t big_endian, int32_t width,
                                                  int32_t height, int32_t flip_h, int32_t flip_v,
                                                  uint32_t* d_argb_out, int32_t* d_status, int32_t out_w,
                                                  int32_t out_h) {
    if (!d_base) return ctx ? fail(ctx, OMR_INVALID_ARGUMENT, "null batch base") : OMR_INVALID_ARGUMENT;
    return render_scaled(ctx, qdef, channels, size_c, d_base, tile_stride_bytes, channel_stride_bytes, nullptr, n_tiles,
                         row_stride, pixel_type, big_endian, width, height, flip_h, flip_v, d_argb_out, d_status, out_w,
                         out_h, nullptr);
}

}  // extern "C"
