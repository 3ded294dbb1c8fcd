// omr_jpegdec.hip — K17, device half: baseline JPEG segments decoded on the GPU.
//
// The host (jpeg_prepare, omr_jpegdec.cpp) has parsed every segment's header, built its lookup
// tables and listed its restart intervals; jpeg_decode_group here puts that into one descriptor
// table, and three kernels do the rest:
//
//   K17a  k_jpeg_entropy  one wave (a workgroup of 64 threads) per restart interval.  The symbol
//         chain is serial, so the decode runs wave-uniform (every value that steers it goes through
//         readfirstlane); the lanes load the Huffman tables into LDS, refill the bit window -- 64 raw
//         bytes per load, the stuffed 00 behind an FF dropped by a ballot / prefix-count compaction
//         into a 256-byte LDS ring -- and each keeps one coefficient of the current block in a
//         register: lane n holds natural index n, which zeroes the block, places a decoded value
//         (the lane whose own zigzag position is the decoded one takes it) and stores the finished block
//         as one 128-byte row of int16.  The coefficients are stored quantised: times a table entry
//         of up to 255 they would not fit 16 bits; K17b multiplies.
//   K17b  k_jpeg_idct     one lane per 8 x 8 block: dequantise, islow IDCT, 8 stores of 8 bytes
//         into the component's plane.
//   K17c  k_jpeg_pixels   one lane per output pixel: the planes' samples, the chroma upsampled by
//         libjpeg's triangle filter, YCbCr -> RGB, and the chunky store.
//
// Bounds.  K17a reads src only inside [iv.src_off, iv.src_off + iv.len), which the host laid inside
// the segment's uploaded bytes (ring_fill compares every byte's position with len; the byte before
// position p is read only for p > 0).  The ring holds at most 3 + 64 unread bytes of its 256.  A
// Huffman lookup reads lut[peek >> 7] (9 bits), maxcode[10..16] and vals[idx] with idx checked
// against [0, 255]: all inside the table's LDS copy whatever the table holds.  The block index is
// computed from the MCU number, which runs over [first_mcu, first_mcu + n_mcu), inside the
// segment's mcux * mcuy by jpeg_prepare: a block of another interval, let alone another segment, is
// never written, however the entropy-coded bytes are damaged -- they steer only which value lands
// at which of the block's own 64 places (the zigzag index is checked against 63 before it is used)
// and when the interval gives up.  A damaged interval writes OMR_INTERNAL to its segment's status
// and stops.  K17b and K17c take every size from the host's descriptors and none from the stream:
// block t < jpeg_total_blocks reads its own 64 coefficients and writes its own 8 x 8 samples of a
// plane that is whole blocks wide and tall; pixel p < w * h reads plane samples at (x, y), x < w <=
// 8 * mcux * hs, and chroma samples up to column ceil(w / 2) - 1 and row ceil(h / 2) - 1, and writes
// ncomp bytes at dst_off + p * ncomp, inside the w * h * ncomp bytes the segment owns.  After a
// damaged interval they run over coefficients that were never written: any bytes give defined
// arithmetic (omr_jpegdec.h) and the call fails on the status.
//
// K18 (off unless omr_ctx_set_jpeg_split asks for it): a long interval -- a tile without restart
// markers is one -- decoded by a whole workgroup instead of K17a's one wave:
//
//   K18a  k_jpeg_entropy_split  one workgroup of 256 lanes per interval, by the self-synchronising
//         split of the Huffman stream (omr_jpegdec.h has the method and the per-lane decoder, which
//         the host emulation omr_jpeg_decode_host_split shares).  In rounds of 256 subsequences of S
//         bits: lane 0 starts from the true state, the others guess; every lane whose predecessor's
//         exit state differs from the state it started from decodes again from it, until no lane
//         changed; a prefix sum of the finished blocks gives every lane its first block's ordinal; a
//         last decode stores the non-zero AC coefficients and the DC differences into the zeroed
//         coefficient area.
//   K18b  k_jpeg_dc_sum         one wave per (interval, component): differences -> DC values.
//
// Bounds of K18.  The per-lane decoder reads src only at positions it has compared with iv.len
// (JpegLaneBits::open and fill), whatever state it is given, and the tables as K17a does.  Its
// loop ends after at most 8 * len symbols (each takes a bit); the rounds are counted from iv.len, the
// settle loop stops after 256 iterations at the latest, and no workgroup waits for another.  A
// store goes to coef[64 * block + n] with n = zigzag[k], k checked against 63, and block =
// jpeg_block_of_ordinal(o) with o < n_mcu * blocks per MCU -- the write pass is given the room left
// below that total and ends when it is used up -- so the MCU is one of [first_mcu, first_mcu +
// n_mcu) and the block one of the interval's own, as in K17a: the stream's bytes steer which of
// those places get which value, and the status.  K18b walks the same blocks by the host's counts
// alone and keeps its running sum in 64 bits (a difference is an int16).
#include "omr_jpegdec.h"
#include "omr_segread.h"
#include "omr_wave.h"

namespace omr {
namespace {

constexpr int kKindJpegEntropy = 36;   // omr_ctx_kernel_timings kinds (omr.h)
constexpr int kKindJpegIdct = 37;
constexpr int kKindJpegPixels = 38;
constexpr int kKindJpegSplit = 39;     // K18a
constexpr int kKindJpegDcSum = 40;     // K18b

__device__ const uint8_t d_zigzag[64] = OMR_JPEG_ZIGZAG;   // zigzag position -> natural index

struct DBits {               // all members wave-uniform
    const uint8_t* src;      // the interval
    uint32_t len;
    uint32_t raw;            // next raw byte
    uint32_t wr, rd;         // bytes put into and taken out of the ring (rd in steps of 4)
    uint64_t acc;
    int nbits, fake;
};

// 64 raw bytes, FF 00 -> FF, behind the ring's last byte.
__device__ __forceinline__ void ring_fill(DBits& B, uint32_t* ring, int lane) {
    const uint32_t p = B.raw + (uint32_t)lane;
    const bool in = p < B.len;
    const uint32_t b = in ? B.src[p] : 0u;
    const uint32_t prev = (in && p > 0u) ? B.src[p - 1u] : 0u;
    const bool keep = in && !(b == 0u && prev == 0xFFu);
    const uint64_t mask = __ballot(keep);
    const uint32_t idx = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    if (keep) reinterpret_cast<uint8_t*>(ring)[(B.wr + idx) & 255u] = (uint8_t)b;
    B.wr += (uint32_t)__popcll(mask);
    B.raw = min(B.len, B.raw + 64u);
    __syncthreads();                                       // one wave: the ring's stores before its loads
}

// 32 more bits into the window (nbits <= 32); behind the interval's end zeros, counted in fake.
__device__ __forceinline__ void refill(DBits& B, uint32_t* ring, int lane) {
    int avail = (int)(B.wr - B.rd);
    while (avail < 4 && B.raw < B.len) {
        ring_fill(B, ring, lane);
        avail = (int)(B.wr - B.rd);
    }
    uint32_t v = __builtin_bswap32(uni(ring[(B.rd & 255u) >> 2]));
    if (avail < 4) {
        const int a = max(avail, 0);
        v = a ? v & (0xFFFFFFFFu << (8 * (4 - a))) : 0u;
        B.fake += 8 * (4 - a);
    }
    B.acc |= (uint64_t)v << (32 - B.nbits);
    B.nbits += 32;
    B.rd += 4u;
}

__device__ __forceinline__ bool take(DBits& B, uint32_t* ring, int lane, int n, uint32_t& v) {   // n in [0, 16]
    if (B.nbits <= 32) refill(B, ring, lane);
    if (B.nbits - B.fake < n) return false;
    v = n ? (uint32_t)(B.acc >> (64 - n)) : 0u;
    B.acc = n ? B.acc << n : B.acc;
    B.nbits -= n;
    return true;
}

// One symbol of the table at H (LDS); -1: no such code, or the interval ends inside it.
__device__ __forceinline__ int symbol(DBits& B, uint32_t* ring, int lane, const JpegHuff* H) {
    if (B.nbits <= 32) refill(B, ring, lane);
    const uint32_t peek = (uint32_t)(B.acc >> 48);
    int len = 0, sym = 0;
    const uint32_t e = uni(H->lut[peek >> 7]);
    if (e) {
        len = (int)(e >> 8);
        sym = (int)(e & 255u);
    } else {
        for (int l = 10; l <= 16; ++l) {
            const int32_t code = (int32_t)(peek >> (16 - l));
            if (code <= (int32_t)uni((uint32_t)H->maxcode[l])) {
                const int32_t idx = code + (int32_t)uni((uint32_t)H->valoff[l]);
                if (idx < 0 || idx > 255) return -1;
                len = l;
                sym = (int)uni(H->vals[idx]);
                break;
            }
        }
        if (!len) return -1;
    }
    if (B.nbits - B.fake < len) return -1;
    B.acc <<= len;
    B.nbits -= len;
    return sym;
}

__device__ __forceinline__ int32_t extend(uint32_t v, int s) {
    return v < (1u << (s - 1)) ? (int32_t)v - (1 << s) + 1 : (int32_t)v;
}

// K17a.  The bounds argument is at the head of this file.
__global__ void __launch_bounds__(64) k_jpeg_entropy(const uint8_t* __restrict__ src, const JpegSegDesc* __restrict__ segs,
                                                     const JpegIvDesc* __restrict__ ivs,
                                                     const JpegTables* __restrict__ tables, uint8_t* __restrict__ ws,
                                                     int32_t* __restrict__ status) {
    __shared__ uint32_t s_huff[3 * kJpegHuffBytes / 4];
    __shared__ uint32_t s_ring[64];
    const int lane = (int)threadIdx.x;
    const JpegIvDesc iv = ivs[blockIdx.x];
    const uint32_t seg = uni(iv.seg);
    const JpegSegDesc S = segs[seg];
    const int32_t ncomp = (int32_t)uni((uint32_t)S.ncomp), hs = (int32_t)uni((uint32_t)S.hs), vs = (int32_t)uni((uint32_t)S.vs);
    const int32_t mcux = (int32_t)uni((uint32_t)S.mcux), mcuy = (int32_t)uni((uint32_t)S.mcuy);
    {
        const uint32_t* g = reinterpret_cast<const uint32_t*>(tables + uni((uint32_t)S.tables));
        const int n = ncomp * (int)(kJpegHuffBytes / 4);
        for (int i = lane; i < n; i += 64) s_huff[i] = g[i];
    }
    __syncthreads();
    const JpegHuff* huff = reinterpret_cast<const JpegHuff*>(s_huff);
    int myk = 0;                                           // the zigzag position of this lane's natural index: no load per coefficient
    for (int k = 0; k < 64; ++k)
        if ((int)d_zigzag[k] == lane) myk = k;
    int16_t* coef = reinterpret_cast<int16_t*>(ws + S.coef_off);
    DBits B;
    B.src = src + iv.src_off;
    B.len = uni(iv.len);
    B.raw = B.wr = B.rd = 0u;
    B.acc = 0;
    B.nbits = B.fake = 0;
    int32_t pred[3] = {0, 0, 0};
    const uint32_t m0 = uni(iv.first_mcu), m1 = m0 + uni(iv.n_mcu);
    bool good = true;
    for (uint32_t m = m0; m < m1 && good; ++m) {
        const int32_t mx = (int32_t)(m % (uint32_t)mcux), my = (int32_t)(m / (uint32_t)mcux);
        for (int c = 0; c < ncomp && good; ++c) {
            const int32_t H = c == 0 ? hs : 1, V = c == 0 ? vs : 1;
            const int32_t base = jpeg_comp_base(c, hs, vs, mcux, mcuy), bw = mcux * H;
            const JpegHuff* dc = huff + 2 * c;
            const JpegHuff* ac = dc + 1;
            for (int32_t by = 0; by < V && good; ++by)
                for (int32_t bx = 0; bx < H && good; ++bx) {
                    const int32_t block = base + (my * V + by) * bw + mx * H + bx;
                    int s = symbol(B, s_ring, lane, dc);
                    uint32_t v = 0;
                    if (s < 0 || s > 11 || !take(B, s_ring, lane, s, v)) { good = false; break; }
                    pred[c] += s ? extend(v, s) : 0;
                    if (pred[c] < -2048 || pred[c] > 2047) { good = false; break; }
                    int32_t mine = lane == 0 ? pred[c] : 0;      // this lane's coefficient: natural index `lane`
                    int k = 1;
                    while (k < 64) {
                        const int rs = symbol(B, s_ring, lane, ac);
                        if (rs < 0) { good = false; break; }
                        const int r = rs >> 4;
                        s = rs & 15;
                        if (s == 0) {
                            if (r != 15) break;
                            k += 16;
                            if (k > 63) { good = false; break; }
                            continue;
                        }
                        k += r;
                        if (k > 63 || s > 10 || !take(B, s_ring, lane, s, v)) { good = false; break; }
                        if (myk == k) mine = extend(v, s);
                        ++k;
                    }
                    if (!good) break;
                    coef[(size_t)64 * (size_t)block + (size_t)lane] = (int16_t)mine;
                }
        }
    }
    if (!good && lane == 0) status[seg] = OMR_INTERNAL;
}

// K18a.  One workgroup of kJpegSplitLanes lanes per interval; the per-lane decode and its bounds are
// jpeg_lane_decode's (omr_jpegdec.h), the bounds argument of the stores is at the head of this file.
// Every barrier stands in control flow that all 256 lanes take alike: the round count comes from
// iv.len, the settle loop leaves by __syncthreads_or, the early leave of the round loop by values all
// lanes read from LDS behind a barrier.
__global__ void __launch_bounds__(256) k_jpeg_entropy_split(const uint8_t* __restrict__ src, const JpegSegDesc* __restrict__ segs,
                                                            const JpegIvDesc* __restrict__ ivs,
                                                            const JpegTables* __restrict__ tables, uint8_t* __restrict__ ws,
                                                            int32_t* __restrict__ status, uint32_t S) {
    __shared__ uint32_t s_huff[3 * kJpegHuffBytes / 4];
    __shared__ uint32_t s_pos[kJpegSplitLanes], s_meta[kJpegSplitLanes];
    __shared__ uint32_t s_wave[kJpegSplitLanes / 64];
    __shared__ uint8_t s_zz[64];
    const uint32_t lane = threadIdx.x;
    const JpegIvDesc iv = ivs[blockIdx.x];
    const JpegSegDesc D = segs[iv.seg];
    const int32_t ncomp = D.ncomp, hs = ncomp == 1 ? 1 : D.hs, vs = ncomp == 1 ? 1 : D.vs;
    {
        const uint32_t* g = reinterpret_cast<const uint32_t*>(tables + D.tables);
        const uint32_t n = (uint32_t)ncomp * (uint32_t)(kJpegHuffBytes / 4);
        for (uint32_t i = lane; i < n; i += kJpegSplitLanes) s_huff[i] = g[i];
        if (lane < 64u) s_zz[lane] = d_zigzag[lane];
    }
    __syncthreads();
    const JpegHuff* huff = reinterpret_cast<const JpegHuff*>(s_huff);
    const uint8_t* in = src + iv.src_off;
    const uint32_t len = min(iv.len, kJpegSplitMaxLen - 1u);      // the host sends no longer one
    int16_t* coef = reinterpret_cast<int16_t*>(ws + D.coef_off);
    const uint32_t b0 = (uint32_t)(hs * vs), bpm = ncomp == 1 ? 1u : b0 + 2u, total = iv.n_mcu * bpm;
    const uint32_t nsub = (8u * len + S - 1u) / S, rounds = (nsub + kJpegSplitLanes - 1u) / kJpegSplitLanes;
    JpegLaneState carry{0u, 0u};                           // where the earlier rounds ended, and
    uint32_t done = 0;                                     // the blocks they finished
    bool bad = false;
    for (uint32_t r = 0; r < rounds; ++r) {
        // 1. guess
        const uint32_t live = min(kJpegSplitLanes, nsub - r * kJpegSplitLanes);   // lanes with a subsequence: the others sit still
        const uint32_t sub = r * kJpegSplitLanes + lane;
        JpegLaneState start = lane == 0u ? carry : JpegLaneState{sub * S, 0u};
        const uint32_t end = sub < nsub ? min((sub + 1u) * S, 8u * len) : 0u;
        JpegLaneRun run = jpeg_lane_decode<false>(in, len, huff, s_zz, b0, bpm, start, end, 0xFFFFFFFFu, JpegNoPut());
        s_pos[lane] = run.exit.pos;
        s_meta[lane] = run.exit.meta;
        __syncthreads();
        // 2. settle: after iteration j the lanes 0 .. j + 1 have the serial decoder's states
        for (uint32_t it = 0; it < kJpegSplitLanes; ++it) {
            JpegLaneState pred = start;
            if (lane > 0u) pred = JpegLaneState{s_pos[lane - 1u], s_meta[lane - 1u]};
            const bool differ = lane < live && pred != start;
            __syncthreads();                               // every look before any new exit state
            if (differ) {
                start = pred;
                run = jpeg_lane_decode<false>(in, len, huff, s_zz, b0, bpm, start, end, 0xFFFFFFFFu, JpegNoPut());
                s_pos[lane] = run.exit.pos;
                s_meta[lane] = run.exit.meta;
            }
            if (!__syncthreads_or(differ ? 1 : 0)) break;
        }
        // 3. scan
        const uint32_t incl = wave_incl_scan(run.blocks, (int)(lane & 63u));
        if ((lane & 63u) == 63u) s_wave[lane >> 6] = incl;
        __syncthreads();
        uint32_t first = done + incl - run.blocks, sum = 0;
        for (uint32_t w = 0; w < kJpegSplitLanes / 64u; ++w) {
            const uint32_t n = s_wave[w];
            if (w < (lane >> 6)) first += n;
            sum += n;
        }
        // 4. write: ordinals below the interval's total only
        const uint32_t room = total > first ? total - first : 0u;
        const uint32_t fm = iv.first_mcu;
        jpeg_lane_decode<true>(in, len, huff, s_zz, b0, bpm, start, end, room, [&](uint32_t b, uint32_t n, int32_t v) {
            coef[(size_t)64 * (size_t)jpeg_block_of_ordinal(first + b, fm, ncomp, hs, vs, D.mcux, D.mcuy) + n] = (int16_t)v;
        });
        if ((run.exit.meta & kJpegLaneStop) && first + run.blocks < total) bad = true;      // out of bits,
        if (run.err != kJpegLaneNoError && first + run.err < total) bad = true;              // a hard error: below the total
        carry = JpegLaneState{s_pos[live - 1u], s_meta[live - 1u]};
        done += sum;
        __syncthreads();                                   // the round's LDS is read before the next writes it
        if ((carry.meta & kJpegLaneStop) || done >= total) break;
    }
    if (lane == 0u && done < total) bad = true;            // the interval ran out of bits before its last block
    if (bad) status[iv.seg] = OMR_INTERNAL;
}

// K18b: one wave per (interval, component): the DC differences K18a left become values, in the
// component's decode order, by a wave scan of 64 blocks and a 64-bit carry.
__global__ void __launch_bounds__(64) k_jpeg_dc_sum(const JpegSegDesc* __restrict__ segs, const JpegIvDesc* __restrict__ ivs,
                                                    uint8_t* __restrict__ ws, int32_t* __restrict__ status) {
    const int lane = (int)threadIdx.x;
    const JpegIvDesc iv = ivs[blockIdx.x];
    const JpegSegDesc D = segs[iv.seg];
    const int32_t c = (int32_t)blockIdx.y;
    if (c >= D.ncomp) return;
    const int32_t hs = D.ncomp == 1 ? 1 : D.hs, vs = D.ncomp == 1 ? 1 : D.vs;
    int16_t* coef = reinterpret_cast<int16_t*>(ws + D.coef_off);
    const uint32_t n = iv.n_mcu * (c == 0 ? (uint32_t)(hs * vs) : 1u);
    int64_t carry = 0;
    bool bad = false;
    for (uint32_t t0 = 0; t0 < n; t0 += 64u) {
        const uint32_t t = t0 + (uint32_t)lane;
        int16_t* dc = nullptr;
        int32_t d = 0;
        if (t < n) {
            dc = coef + (size_t)64 * (size_t)jpeg_block_of_comp(t, c, iv.first_mcu, hs, vs, D.mcux, D.mcuy);
            d = *dc;
        }
        const int32_t incl = (int32_t)wave_incl_scan((uint32_t)d, lane);
        const int64_t v = carry + incl;
        if (dc) {
            if (v < -2048 || v > 2047) bad = true;
            else *dc = (int16_t)v;
        }
        carry += (int32_t)lane_value((uint32_t)incl, 63u);
    }
    if (bad) status[iv.seg] = OMR_INTERNAL;
}

// K17b: block t of segment blockIdx.y (+ k * gridDim.y).
__global__ void __launch_bounds__(64) k_jpeg_idct(const JpegSegDesc* __restrict__ segs, int32_t n_seg,
                                                  const JpegTables* __restrict__ tables, uint8_t* __restrict__ ws) {
    const int32_t t = (int32_t)(blockIdx.x * 64u + threadIdx.x);
    for (int32_t seg = (int32_t)blockIdx.y; seg < n_seg; seg += (int32_t)gridDim.y) {
        const JpegSegDesc S = segs[seg];
        const int32_t hs = S.ncomp == 1 ? 1 : S.hs, vs = S.ncomp == 1 ? 1 : S.vs;
        if (t >= jpeg_total_blocks(S.ncomp, hs, vs, S.mcux, S.mcuy)) continue;
        const int32_t base1 = jpeg_comp_base(1, hs, vs, S.mcux, S.mcuy);
        const int32_t c = t < base1 ? 0 : 1 + (t - base1) / (S.mcux * S.mcuy);
        const int32_t base = jpeg_comp_base(c, hs, vs, S.mcux, S.mcuy), bw = S.mcux * (c == 0 ? hs : 1), b = t - base;
        const size_t pitch = (size_t)8 * bw;
        jpeg_idct_block(reinterpret_cast<const int16_t*>(ws + S.coef_off) + (size_t)64 * t, tables[S.tables].q[c],
                        ws + S.plane_off + (size_t)64 * base + (size_t)(b / bw) * 8 * pitch + (size_t)(b % bw) * 8, pitch);
    }
}

// K17c: pixel p of segment blockIdx.y (+ k * gridDim.y).
__global__ void __launch_bounds__(256) k_jpeg_pixels(const JpegSegDesc* __restrict__ segs, int32_t n_seg,
                                                     const uint8_t* __restrict__ ws, uint8_t* __restrict__ dst) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    for (int32_t seg = (int32_t)blockIdx.y; seg < n_seg; seg += (int32_t)gridDim.y) {
        JpegSegDesc S = segs[seg];
        if (p >= (int64_t)S.w * S.h) continue;
        if (S.ncomp == 1) S.hs = S.vs = 1;
        uint8_t o[3];
        jpeg_pixel(S, ws + S.plane_off, (int32_t)(p % S.w), (int32_t)(p / S.w), o);
        uint8_t* d = dst + S.dst_off + (uint64_t)p * (uint64_t)S.ncomp;
        d[0] = o[0];
        if (S.ncomp == 3) {
            d[1] = o[1];
            d[2] = o[2];
        }
    }
}

}  // namespace

omr_status launch_jpeg_decode(Ctx* ctx, const uint8_t* src, const JpegSegDesc* segs, int32_t n_seg, const JpegIvDesc* ivs,
                              int32_t n_iv, const JpegTables* tables, uint8_t* ws, uint8_t* dst, int32_t* status,
                              int32_t max_blocks, int64_t max_pixels, int32_t n_split, uint32_t split_bits) {
    if (n_seg <= 0) return OMR_OK;
    const unsigned gy = (unsigned)std::min(n_seg, 65535);
    if (n_iv > 0) {
        KernelTimer timer(ctx, kKindJpegEntropy, true);
        omr_launch(k_jpeg_entropy, dim3((unsigned)n_iv), dim3(64), 0u, ctx->stream, src, segs, ivs, tables, ws, status);
        OMR_HIP(ctx, hipGetLastError());
    }
    if (n_split > 0) {
        {
            KernelTimer timer(ctx, kKindJpegSplit, true);
            omr_launch(k_jpeg_entropy_split, dim3((unsigned)n_split), dim3(kJpegSplitLanes), 0u, ctx->stream, src, segs, ivs + n_iv,
                       tables, ws, status, split_bits);
            OMR_HIP(ctx, hipGetLastError());
        }
        KernelTimer timer(ctx, kKindJpegDcSum, true);
        omr_launch(k_jpeg_dc_sum, dim3((unsigned)n_split, 3u), dim3(64), 0u, ctx->stream, segs, ivs + n_iv, ws, status);
        OMR_HIP(ctx, hipGetLastError());
    }
    {
        KernelTimer timer(ctx, kKindJpegIdct, true);
        omr_launch(k_jpeg_idct, dim3((unsigned)((max_blocks + 63) / 64), gy), dim3(64), 0u, ctx->stream, segs, n_seg, tables, ws);
        OMR_HIP(ctx, hipGetLastError());
    }
    {
        KernelTimer timer(ctx, kKindJpegPixels, true);
        omr_launch(k_jpeg_pixels, dim3((unsigned)((max_pixels + 255) / 256), gy), dim3(256), 0u, ctx->stream, segs, n_seg,
                   static_cast<const uint8_t*>(ws), dst);
        OMR_HIP(ctx, hipGetLastError());
    }
    return OMR_OK;
}

// The descriptor table of one group: [JpegSegDesc m][JpegIvDesc k][JpegTables s] | [status i32 m]:
// everything goes up in one copy (the statuses as OMR_OK), the statuses come back.
CodecLaunched jpeg_decode_group(Ctx* ctx, SegPipe* T, const std::vector<CodecJob>& jobs, const std::vector<JpegPlan>& plans,
                                int32_t samples, bool ycc, const uint8_t* d_src, uint8_t* d_dst, std::vector<int32_t>& status) {
    const size_t n = jobs.size();
    status.assign(n, OMR_OK);
    std::vector<int32_t> live;                             // the jobs that decode: parsed, and not empty
    size_t n_iv = 0;
    for (size_t k = 0; k < n; ++k)
        if (jobs[k].parsed == OMR_OK) {
            live.push_back((int32_t)k);
            n_iv += plans[k].intervals.size();
        } else {
            status[k] = jobs[k].parsed;
        }
    const size_t m = live.size();
    if (!m) return OMR_OK;
    if (n_iv > 0x7FFFFFFFull) return fail(ctx, OMR_INVALID_ARGUMENT, "jpeg: too many restart intervals in one group");
    std::vector<int32_t> table_of(m);
    std::vector<int32_t> sets;                             // live indices whose table set is the first of its kind
    for (size_t j = 0; j < m; ++j) {
        const JpegTables& mine = plans[(size_t)live[j]].tables;
        int32_t found = -1;
        for (size_t s = 0; s < sets.size() && found < 0; ++s)
            if (!std::memcmp(&plans[(size_t)live[(size_t)sets[s]]].tables, &mine, sizeof(JpegTables))) found = (int32_t)s;
        if (found < 0) {
            found = (int32_t)sets.size();
            sets.push_back((int32_t)j);
        }
        table_of[j] = found;
    }
    const size_t o_iv = m * sizeof(JpegSegDesc), o_tab = o_iv + n_iv * sizeof(JpegIvDesc);
    const size_t o_status = o_tab + sets.size() * sizeof(JpegTables), total = o_status + 4 * m;
    omr_status st = grow_pinned(ctx, T->pin_tab, T->d_tab, T->tab_cap, total, "jpeg tables");
    if (st) return st;
    uint8_t* tab = static_cast<uint8_t*>(T->pin_tab);
    uint8_t* dtab = static_cast<uint8_t*>(T->d_tab);
    JpegSegDesc* hs = reinterpret_cast<JpegSegDesc*>(tab);
    JpegIvDesc* hi = reinterpret_cast<JpegIvDesc*>(tab + o_iv);
    // The intervals in two lists, K17a's in front of K18's: one of at least ctx->jpeg_split_min bytes
    // takes the split decode (off by default: then the second list is empty and nothing changes).
    const uint32_t split_min = ctx->jpeg_split_min;
    const uint32_t split_bits = ctx->jpeg_split_bits ? ctx->jpeg_split_bits : kJpegSplitDefaultBits;
    auto splits = [&](const JpegInterval& iv) { return split_min && iv.len >= split_min && iv.len < kJpegSplitMaxLen; };
    size_t n_split = 0;
    for (size_t j = 0; j < m; ++j)
        for (const JpegInterval& iv : plans[(size_t)live[j]].intervals) n_split += splits(iv);
    size_t ws_bytes = 0, iv_at = 0, split_at = n_iv - n_split;
    size_t zero_lo = 0, zero_hi = 0;                       // the workspace from the first to the last segment K18 touches
    int32_t max_blocks = 0;
    int64_t max_pixels = 0;
    for (size_t j = 0; j < m; ++j) {
        const CodecJob& J = jobs[(size_t)live[j]];
        const JpegPlan& P = plans[(size_t)live[j]];
        JpegSegDesc& S = hs[j];
        S.dst_off = J.dst_off;
        S.coef_off = ws_bytes;
        ws_bytes += jpeg_coef_bytes(P);
        S.plane_off = ws_bytes;
        ws_bytes += jpeg_plane_bytes(P);
        S.w = P.w; S.h = P.h; S.ncomp = P.ncomp; S.hs = P.hs; S.vs = P.vs; S.ycc = ycc && samples == 3;
        S.mcux = P.mcux; S.mcuy = P.mcuy;
        S.tables = table_of[j];
        S.pad = 0;
        max_blocks = std::max(max_blocks, jpeg_total_blocks(P.ncomp, P.hs, P.vs, P.mcux, P.mcuy));
        max_pixels = std::max(max_pixels, (int64_t)P.w * P.h);
        for (const JpegInterval& iv : P.intervals) {
            const bool sp = splits(iv);
            hi[sp ? split_at++ : iv_at++] = {J.in_off + iv.off, (uint32_t)iv.len, (uint32_t)j, iv.first_mcu, iv.n_mcu};
            if (sp) {
                if (zero_hi == 0) zero_lo = S.coef_off;
                zero_hi = S.plane_off;
            }
        }
    }
    for (size_t s = 0; s < sets.size(); ++s)
        std::memcpy(tab + o_tab + s * sizeof(JpegTables), &plans[(size_t)live[(size_t)sets[s]]].tables, sizeof(JpegTables));
    std::memset(tab + o_status, 0, 4 * m);                 // OMR_OK
    st = grow_device(ctx, T->d_coef, T->coef_cap, ws_bytes);
    if (st) return st;
    OMR_HIP(ctx, hipMemcpyAsync(dtab, tab, total, hipMemcpyHostToDevice, ctx->stream));
    // K18a stores only what is not zero (the planes between two coefficient areas are zeroed along: one call)
    if (n_split) OMR_HIP(ctx, hipMemsetAsync(static_cast<uint8_t*>(T->d_coef) + zero_lo, 0, zero_hi - zero_lo, ctx->stream));
    st = launch_jpeg_decode(ctx, d_src, reinterpret_cast<const JpegSegDesc*>(dtab), (int32_t)m,
                            reinterpret_cast<const JpegIvDesc*>(dtab + o_iv), (int32_t)(n_iv - n_split),
                            reinterpret_cast<const JpegTables*>(dtab + o_tab), static_cast<uint8_t*>(T->d_coef), d_dst,
                            reinterpret_cast<int32_t*>(dtab + o_status), max_blocks, max_pixels, (int32_t)n_split, split_bits);
    if (st) return st;
    CodecLaunched launched;
    launched.off = o_status;
    launched.live = std::move(live);
    return launched;
}

}  // namespace omr

using namespace omr;

extern "C" omr_status omr_jpeg_decode_batch_device(omr_ctx* ctx, const uint8_t* tables, size_t tables_length,
                                                   const uint8_t* src, const uint64_t* offsets, const uint32_t* lengths,
                                                   const int32_t* widths, const int32_t* heights, int32_t n, int32_t samples,
                                                   int32_t ycbcr, uint8_t* d_dst, const uint64_t* dst_offsets,
                                                   int32_t* status) {
    if (!ctx) return OMR_INVALID_ARGUMENT;
    if (n < 0) return fail(ctx, OMR_INVALID_ARGUMENT, "jpeg: negative stream count");
    if (n == 0) return OMR_OK;
    if (!src || !offsets || !lengths || !widths || !heights || !d_dst || !dst_offsets || !status || (!tables && tables_length))
        return fail(ctx, OMR_INVALID_ARGUMENT, "jpeg: null argument");
    if (samples != 1 && samples != 3) return fail(ctx, OMR_INVALID_ARGUMENT, "jpeg: samples must be 1 or 3");
    OMR_HIP(ctx, hipSetDevice(ctx->device));
    SegPipe* T = seg_pipe(ctx, SegKind::tiff);
    std::vector<CodecJob> jobs((size_t)n);
    std::vector<JpegPlan> plans((size_t)n);
    for (int32_t k = 0; k < n; ++k) {
        CodecJob& J = jobs[(size_t)k];
        J.dst_off = dst_offsets[k];
        if (widths[k] < 1 || heights[k] < 1 || widths[k] > 65535 || heights[k] > 65535 ||
            (uint64_t)widths[k] * (uint64_t)heights[k] * (uint64_t)samples > ((uint64_t)256 << 20)) {
            J.parsed = OMR_INVALID_ARGUMENT;
            continue;
        }
        J.parsed = jpeg_prepare(tables, tables_length, src + offsets[k], lengths[k], widths[k], heights[k], samples,
                                plans[(size_t)k], nullptr);
    }
    return decode_batch_staged(ctx, T, "jpeg", jobs, src, offsets, lengths, [&](std::vector<int32_t>& stv) {
        return jpeg_decode_group(ctx, T, jobs, plans, samples, ycbcr != 0, static_cast<const uint8_t*>(T->d_in), d_dst, stv);
    }, status);
}
