// omr_tiffread.hip — K13: the device half of the tiled TIFF reader (omr_tiffread.cpp).
//
// K13a k_lzw_decode: one wave per TIFF LZW segment (a tile or a strip), many segments per launch.
// K13b k_tiff_place<BPS, PRED, SWAP, CHUNKY>: one wave per segment row: undo the horizontal predictor
//      with a wave prefix sum, crop to the requested region and store into the destination at its
//      pitch; CHUNKY takes one sample out of each interleaved pixel.  k_tiff_place_fp<BPS, BE> does
//      the same for the floating-point predictor (Predictor 3).
//
// TIFF LZW (TIFF 6.0 §13, as libtiff writes and reads it): codes packed MSB first, 9 bits at the
// start, 256 = Clear, 257 = EOI, first entry 258; "early change": the reader takes 10 bits once its
// next free entry is 511, 11 at 1023 and 12 at 2047.  Between two Clears the width of the i-th code
// therefore depends on i alone, and so does its bit offset: that is what lets 64 lanes pick 64
// codes out of the stream at once.
#include "omr_internal.h"

namespace omr {

namespace {

constexpr int kKindLzwDecode = 30;   // omr_ctx_kernel_timings kinds (omr.h)
constexpr int kKindTiffPlace = 31;
constexpr uint32_t kLzwClear = 256, kLzwEoi = 257;
constexpr uint32_t kLzwEntries = 4096;

// Code i since the last Clear (i = 0: the code right behind it) is read while the next free entry
// is 258 for i = 0 and 257 + i after that: 9 bits for i < 254, 10 for i < 766, 11 for i < 1790,
// 12 from there on (the table stops growing at 4096 entries; the width stays).
__device__ __forceinline__ uint32_t lzw_width(uint32_t i) { return i < 254u ? 9u : i < 766u ? 10u : i < 1790u ? 11u : 12u; }
// Bits taken by codes 0 .. i-1.
__device__ __forceinline__ uint64_t lzw_bits_before(uint32_t i) {
    const uint32_t a = min(i, 254u), b = min(max(i, 254u) - 254u, 512u), c = min(max(i, 766u) - 766u, 1024u);
    const uint32_t d = max(i, 1790u) - 1790u;
    return (uint64_t)(9u * a + 10u * b + 11u * c) + 12ull * d;
}

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    return v;
}

// Orders the LDS traffic of a one-wave workgroup: the lanes of a wave run in lockstep and the LDS
// serves a wave's accesses in issue order, so a write by one lane is seen by a later read of
// another once the compiler keeps the two in program order, which this fence (no instruction at
// wavefront scope) makes it do.  Unlike __syncthreads() it does not wait for the global stores in
// flight.
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// K13a.  Grid-stride over the segments, one wave (a workgroup of 64 threads) per segment.
//
// The wave works in batches of 64 codes.  Lane j extracts code i0 + j at its closed-form bit
// offset; a ballot cuts the batch at the first Clear, EOI, bad code or end of the stream.  A code
// that names an entry made inside the batch depends on an earlier lane: entry 257 + i is made when
// code i is read, as string(code i-1) + first byte(code i), so code c read by lane j with
// c - 257 - i0 = j' >= 0 has the length of lane j'-1's string plus one and its first byte (j' = j
// is the code-equals-next-free case; j' = 0 hangs on the last code of the batch before).  Lengths
// and first bytes along these chains are resolved by pointer jumping (at most 7 rounds), an
// exclusive scan of the lengths gives each lane its output position, the new entries go to the
// LDS table, and each lane writes its own string backwards along the prefix chain.  The output is
// written once and never read back.
//
// Bounds, by construction:
//  - table indices are masked to 12 bits (dict, firstb: 4096 entries each);
//  - every output store is guarded by p < expected, so a string that overruns the segment's size
//    is cut and nothing is written behind dst_offsets[seg] + expected[seg];
//  - a code is only taken when all of its bits lie inside the stream (bit + width <= 8 * length),
//    and the stream is read by aligned dword loads of words that hold at least one of its bytes;
//    every turn of the loop consumes at least one code or ends the segment, so the loop is
//    bounded by the stream's bit length;
//  - the string walk is bounded by the string's recorded length (< 4096), not by the table's
//    contents;
//  - a code above the next free entry, a stream that ends before `expected` bytes are out (with or
//    without EOI) and an old-style LSB-first stream set status[seg] = OMR_INTERNAL and end that
//    segment only.
// All loop conditions come from ballots, broadcasts and per-segment scalars, so control flow is
// wave-uniform; one wave per workgroup, so LDS traffic is ordered by wave_lds_fence, not a barrier.
__global__ void __launch_bounds__(64) k_lzw_decode(const uint8_t* __restrict__ src, const uint64_t* __restrict__ offsets,
                                                   const uint32_t* __restrict__ lengths,
                                                   const uint32_t* __restrict__ expected, int n,
                                                   uint8_t* __restrict__ dst, const uint64_t* __restrict__ dst_offsets,
                                                   int32_t* __restrict__ status) {
    __shared__ uint32_t dict[kLzwEntries];    // prefix code [0,12) | suffix byte [12,20) | string length [20,32)
    __shared__ uint8_t firstb[kLzwEntries];   // first byte of the entry's string
    const int lane = (int)threadIdx.x;
    for (int seg = (int)blockIdx.x; seg < n; seg += (int)gridDim.x) {
        const uint8_t* s = src + offsets[seg];
        const uint32_t len = lengths[seg], exp = expected[seg];
        uint8_t* d = dst + dst_offsets[seg];
        const uint64_t nbits = (uint64_t)len * 8u;
        uint64_t base = 0;          // bit position of code 0 since the last Clear
        uint32_t i0 = 0;            // index since the last Clear of lane 0's code
        uint32_t outpos = 0;
        uint32_t prev_code = 0, prev_len = 0, prev_first = 0;   // the code before the batch (i0 >= 1)
        int32_t st = OMR_OK;
        if (len >= 2u && s[0] == 0 && (s[1] & 1u)) st = OMR_INTERNAL;   // old-style (LSB-first) stream
        // The stream is read through a 1 KiB window held in four registers per lane (dword k * 64
        // + lane of the window in rk), loaded with aligned dword loads: positions below are in
        // bytes from sw, the dword that holds s[0].  Only dwords that hold a byte of the stream
        // are loaded, so no load leaves the words the stream itself occupies.
        const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(s) & 3u);
        const uint32_t* sw = reinterpret_cast<const uint32_t*>(s - mis);
        const uint64_t end_pos = (uint64_t)mis + len;
        uint64_t win_lo = 0;
        bool win_valid = false;
        uint32_t r0 = 0, r1 = 0, r2 = 0, r3 = 0;
        while (st == OMR_OK && outpos < exp) {
            wave_lds_fence();       // the walk of the batch before is done with the table
            const uint32_t i = i0 + (uint32_t)lane;
            const uint32_t w = lzw_width(i);
            const uint64_t bit = base + lzw_bits_before(i);
            const bool have = bit + w <= nbits;
            // the batch's 64 codes lie in the 96 bytes from its first one: at most 27 dwords
            const uint64_t fb0 = (uint64_t)mis + ((base + lzw_bits_before(i0)) >> 3);
            if (!win_valid || fb0 < win_lo || fb0 + 112u > win_lo + 1024u) {
                win_lo = fb0 & ~3ull;
                const uint64_t d0 = (win_lo >> 2) + (uint64_t)lane;
                r0 = (d0 << 2) < end_pos ? sw[d0] : 0u;
                r1 = ((d0 + 64u) << 2) < end_pos ? sw[d0 + 64u] : 0u;
                r2 = ((d0 + 128u) << 2) < end_pos ? sw[d0 + 128u] : 0u;
                r3 = ((d0 + 192u) << 2) < end_pos ? sw[d0 + 192u] : 0u;
                win_valid = true;
            }
            // lane l takes the batch's dword l out of the window, then each lane fetches the two
            // dwords around its code from those
            const uint32_t wi = (uint32_t)((fb0 >> 2) - (win_lo >> 2)) + (uint32_t)lane;
            const uint32_t x0 = __shfl(r0, (int)(wi & 63u)), x1 = __shfl(r1, (int)(wi & 63u));
            const uint32_t x2 = __shfl(r2, (int)(wi & 63u)), x3 = __shfl(r3, (int)(wi & 63u));
            const uint32_t sel = (wi >> 6) & 3u;
            const uint32_t bd = sel == 0u ? x0 : sel == 1u ? x1 : sel == 2u ? x2 : x3;
            const uint64_t bpos = (uint64_t)mis + (bit >> 3);
            const uint32_t di = have ? (uint32_t)((bpos >> 2) - (fb0 >> 2)) : 0u;   // <= 25 (see above)
            const uint32_t w0 = __shfl(bd, (int)(di & 63u)), w1 = __shfl(bd, (int)((di + 1u) & 63u));
            uint32_t code = 0;
            if (have) {
                // bytes bpos, bpos + 1, bpos + 2 (little-endian dwords), then MSB first; bits past the
                // stream's end are shifted out, since bit + w <= nbits
                const uint32_t three = (uint32_t)((((uint64_t)w1 << 32) | w0) >> (8u * (uint32_t)(bpos & 3u)));
                const uint32_t v = (three & 0xFFu) << 16 | (three & 0xFF00u) | ((three >> 16) & 0xFFu);
                code = (v >> (24u - w - (uint32_t)(bit & 7u))) & ((1u << w) - 1u);
            }
            // creator lane of entry `code`, when it is made in this batch (>= 0); a code above the
            // next free entry is one whose creator lies behind its reader (this also rejects
            // anything but a literal right behind a Clear)
            const int jp = (int)code - 257 - (int)i0;
            const unsigned long long m_special = __ballot(have && (code == kLzwClear || code == kLzwEoi));
            const unsigned long long m_short = __ballot(!have);
            const unsigned long long m_bad = __ballot(have && code > kLzwEoi && jp > lane);
            const unsigned long long m_stop = m_special | m_short | m_bad;
            const int nvalid = m_stop ? __ffsll((long long)m_stop) - 1 : 64;
            const bool valid = lane < nvalid;

            int dep = -1;                 // lane whose string this one extends (unresolved)
            uint32_t acc = 1;             // resolved: string length; else: bytes on top of dep's
            uint32_t fb = code & 255u;    // first byte of the string
            if (valid && code > kLzwEoi) {
                if (jp < 0) {
                    acc = dict[code & (kLzwEntries - 1u)] >> 20;
                    fb = firstb[code & (kLzwEntries - 1u)];
                } else if (jp == 0) {
                    acc = prev_len + 1u;
                    fb = prev_first;
                } else {
                    dep = jp - 1;
                }
            }
            while (__any(dep >= 0)) {
                const int dl = dep >= 0 ? dep : lane;
                const uint32_t a_d = __shfl(acc, dl), f_d = __shfl(fb, dl);
                const int d_d = __shfl(dep, dl);
                if (dep >= 0) {
                    acc += a_d;
                    fb = f_d;
                    dep = d_d;
                }
            }
            const uint32_t L = valid ? acc : 0u;
            const uint32_t incl = wave_incl_scan(L, lane);
            const uint32_t total = __shfl(incl, 63);
            const uint32_t pos = outpos + incl - L;

            // entry 257 + i: string(code i-1) + first byte(code i); none right behind a Clear, none
            // once the table is full
            uint32_t pc = __shfl_up(code, 1), pl = __shfl_up(acc, 1), pf = __shfl_up(fb, 1);
            if (lane == 0) {
                pc = prev_code;
                pl = prev_len;
                pf = prev_first;
            }
            if (valid && i >= 1u && 257u + i < kLzwEntries) {
                const uint32_t e = (257u + i) & (kLzwEntries - 1u);
                dict[e] = (pc & 0xFFFu) | (fb << 12) | ((pl + 1u) << 20);
                firstb[e] = (uint8_t)pf;
            }
            wave_lds_fence();

            if (valid) {
                uint32_t c = code, p = pos + acc;
                for (uint32_t k = acc; k > 1u; --k) {
                    const uint32_t e = dict[c & (kLzwEntries - 1u)];
                    --p;
                    if (p < exp) d[p] = (uint8_t)(e >> 12);
                    c = e & 0xFFFu;
                }
                --p;
                if (p < exp) d[p] = (uint8_t)c;
            }

            outpos += total;
            if (outpos >= exp) break;
            if (nvalid == 64) {
                prev_code = __shfl(code, 63);
                prev_len = __shfl(acc, 63);
                prev_first = __shfl(fb, 63);
                i0 += 64u;
            } else if (((m_short | m_bad) >> nvalid) & 1ull) {
                st = OMR_INTERNAL;                       // the stream ends early, or a bad code
            } else if (__shfl(code, nvalid) == kLzwEoi) {
                st = OMR_INTERNAL;                       // EOI before the segment is full
            } else {                                     // Clear
                const uint32_t ic = i0 + (uint32_t)nvalid;
                base += lzw_bits_before(ic) + lzw_width(ic);
                i0 = 0;
                prev_code = prev_len = prev_first = 0;
            }
        }
        if (lane == 0) status[seg] = st;
        wave_lds_fence();
    }
}

template <int BPS> struct SampleOf;
template <> struct SampleOf<1> { typedef uint8_t T; };
template <> struct SampleOf<2> { typedef uint16_t T; };
template <> struct SampleOf<4> { typedef uint32_t T; };
template <> struct SampleOf<8> { typedef uint64_t T; };

__device__ __forceinline__ uint8_t bswap_s(uint8_t v) { return v; }
__device__ __forceinline__ uint16_t bswap_s(uint16_t v) { return (uint16_t)(v << 8 | v >> 8); }
__device__ __forceinline__ uint32_t bswap_s(uint32_t v) { return __builtin_bswap32(v); }

// K13b.  blockIdx.y: the placement; the waves of the grid's x dimension stride over its rows.
// Predictor 2: the row's samples are running sums from the segment's first column, in the sample's
// own width with wrap-around (bytes swapped to native around the add when SWAP), so the wave scans
// from column 0 and stores from x0 on.  Every load is inside the segment (x < x1 <= seg_w, y < y1 <=
// the segment's rows) and every store inside the placement's rectangle, which the host clipped to
// the region and the image.
// CHUNKY: the segment holds P.spp samples per pixel and the placement takes sample P.sample of each
// (0 <= sample < spp, set by the planner): pixel x of a row is sample x * spp + sample of its seg_w *
// spp samples, so the same bounds hold (x < x1 <= seg_w gives x * spp + sample < seg_w * spp), and
// predictor 2 runs per component, spp samples apart, which is the scan over this one component.
// Without CHUNKY neither field is read and the kernel is what it was for one sample per pixel.
template <int BPS, int PRED, bool SWAP, bool CHUNKY>
__global__ void __launch_bounds__(256) k_tiff_place(const TiffPlace* __restrict__ places) {
    typedef typename SampleOf<BPS>::T T;
    const TiffPlace P = places[blockIdx.y];
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    const int rows = P.y1 - P.y0;
    const int spp = CHUNKY ? P.spp : 1, sample = CHUNKY ? P.sample : 0;
    for (int r = (int)blockIdx.x * 4 + wave; r < rows; r += (int)gridDim.x * 4) {
        const T* srow = P.src ? reinterpret_cast<const T*>(P.src) + (int64_t)(P.y0 + r) * P.seg_w * spp + sample : nullptr;
        T* drow = reinterpret_cast<T*>(P.dst) + (int64_t)r * P.dst_pitch;
        if constexpr (PRED == 2 && BPS < 8) {
            uint32_t carry = 0;
            for (int xb = 0; xb < P.x1; xb += 64) {
                const int x = xb + lane;
                T v = 0;
                if (srow && x < P.x1) v = srow[(int64_t)x * spp];
                if (SWAP) v = bswap_s(v);
                uint32_t sum = wave_incl_scan((uint32_t)v, lane) + carry;
                carry = __shfl(sum, 63);
                T o = (T)sum;
                if (SWAP) o = bswap_s(o);
                if (x >= P.x0 && x < P.x1) drow[x - P.x0] = o;
            }
        } else {
            for (int x = P.x0 + lane; x < P.x1; x += 64) drow[x - P.x0] = srow ? srow[(int64_t)x * spp] : (T)0;
        }
    }
}

// K13b for the floating-point predictor (Predictor 3, libtiff's fpAcc; one sample per pixel): the
// grid of k_tiff_place, one wave per segment row.  A row of n = seg_w samples of BPS bytes is stored
// as BPS planes of n bytes, the most significant byte of every sample first (in either byte order
// of the file), and the n * BPS bytes are running differences (mod 256) across the whole row, planes
// included.  So byte x of plane b is the sum of the row's bytes up to b * n + x: the totals of the
// planes in front (pass 1: over all n columns, whatever the crop) plus a wave scan along the plane
// (pass 2: in steps of 64 columns up to x1, the carry of each plane kept mod 256).  The lane puts
// its BPS bytes together in the file's byte order (BE: plane b is byte b of the sample) and stores.
// No LDS, and no limit on n.
// Bounds: a load reads byte b * n + x of the row with b < BPS and x < n (pass 1) or x < x1 <= n
// (pass 2), inside the row's n * BPS bytes, and the row y0 + r < y1 is one of the segment's rows;
// a store goes to column x - x0 with x0 <= x < x1 of row r < y1 - y0: inside the placement's
// rectangle, as in k_tiff_place.  The loops' bounds are per-placement scalars, so every shuffle
// runs with all 64 lanes.
template <int BPS, bool BE>
__global__ void __launch_bounds__(256) k_tiff_place_fp(const TiffPlace* __restrict__ places) {
    typedef typename SampleOf<BPS>::T T;
    const TiffPlace P = places[blockIdx.y];
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    const int rows = P.y1 - P.y0;
    const int n = P.seg_w;
    for (int r = (int)blockIdx.x * 4 + wave; r < rows; r += (int)gridDim.x * 4) {
        T* drow = reinterpret_cast<T*>(P.dst) + (int64_t)r * P.dst_pitch;
        if (!P.src) {
            for (int x = P.x0 + lane; x < P.x1; x += 64) drow[x - P.x0] = (T)0;
            continue;
        }
        const uint8_t* srow = P.src + (int64_t)(P.y0 + r) * n * BPS;
        uint32_t carry[BPS];                                // into plane b: the bytes in front of it, mod 256
        carry[0] = 0;
#pragma unroll
        for (int b = 0; b + 1 < BPS; ++b) {
            const uint8_t* plane = srow + (int64_t)b * n;
            uint32_t t = 0;
            for (int x = lane; x < n; x += 64) t += plane[x];
            t = __shfl(wave_incl_scan(t, lane), 63);
            carry[b + 1] = (carry[b] + t) & 255u;
        }
        for (int xb = 0; xb < P.x1; xb += 64) {
            const int x = xb + lane;
            T o = 0;
#pragma unroll
            for (int b = 0; b < BPS; ++b) {
                uint32_t v = 0;
                if (x < P.x1) v = srow[(int64_t)b * n + x];
                const uint32_t sum = wave_incl_scan(v, lane) + carry[b];
                carry[b] = __shfl(sum, 63) & 255u;
                o |= (T)(sum & 255u) << (8 * (BE ? b : BPS - 1 - b));
            }
            if (x >= P.x0 && x < P.x1) drow[x - P.x0] = o;
        }
    }
}

template <int BPS, bool CHUNKY>
void launch_place_bps(const dim3& g, hipStream_t s, const TiffPlace* d_places, int pred, bool swap) {
    if (pred == 2) {
        if (swap) omr_launch(k_tiff_place<BPS, 2, true, CHUNKY>, g, dim3(256), 0u, s, d_places);
        else omr_launch(k_tiff_place<BPS, 2, false, CHUNKY>, g, dim3(256), 0u, s, d_places);
    } else {
        omr_launch(k_tiff_place<BPS, 1, false, CHUNKY>, g, dim3(256), 0u, s, d_places);
    }
}

template <int BPS>
void launch_place_fp(const dim3& g, hipStream_t s, const TiffPlace* d_places, bool big) {
    if (big) omr_launch(k_tiff_place_fp<BPS, true>, g, dim3(256), 0u, s, d_places);
    else omr_launch(k_tiff_place_fp<BPS, false>, g, dim3(256), 0u, s, d_places);
}

}  // namespace

omr_status launch_lzw_decode(Ctx* ctx, const StreamTable& t) {
    if (t.n <= 0) return OMR_OK;
    // 20 KiB of LDS per wave: 8 waves per CU
    const int blocks = std::min(t.n, std::max(1, ctx->cu_count) * 8);
    KernelTimer timer(ctx, kKindLzwDecode, true);
    omr_launch(k_lzw_decode, dim3((unsigned)blocks), dim3(64), 0u, ctx->stream, t.src, t.offsets, t.lengths, t.expected,
               (int)t.n, t.dst, t.dst_offsets, t.status);
    OMR_HIP(ctx, hipGetLastError());
    return OMR_OK;
}

omr_status launch_tiff_place(Ctx* ctx, const TiffPlace* d_places, int32_t n, int32_t max_rows, int32_t bps,
                             int32_t predictor, bool swap, int32_t spp) {
    if (n <= 0 || max_rows <= 0) return OMR_OK;
    if (predictor == 2 && bps == 8) return fail(ctx, OMR_INVALID_ARGUMENT, "tiff: predictor 2 with 64-bit samples");
    if (predictor == 3 && ((bps != 4 && bps != 8) || spp != 1))
        return fail(ctx, OMR_INVALID_ARGUMENT, "tiff: predictor 3 needs float or double samples, one per pixel");
    if (spp < 1) return fail(ctx, OMR_INVALID_ARGUMENT, "tiff: bad samples per pixel");
    const bool host_little = [] { const uint16_t one = 1; uint8_t b; std::memcpy(&b, &one, 1); return b == 1; }();
    KernelTimer timer(ctx, kKindTiffPlace, true);
    for (int32_t p0 = 0; p0 < n; p0 += 65535) {           // grid y limit
        const dim3 g((unsigned)std::min(64, (max_rows + 3) / 4), (unsigned)std::min(65535, n - p0));
        if (predictor == 3) {                              // swap: the file's order is the other one
            if (bps == 4) launch_place_fp<4>(g, ctx->stream, d_places + p0, swap == host_little);
            else launch_place_fp<8>(g, ctx->stream, d_places + p0, swap == host_little);
        } else if (spp == 1) {
            switch (bps) {
            case 1: launch_place_bps<1, false>(g, ctx->stream, d_places + p0, predictor, false); break;
            case 2: launch_place_bps<2, false>(g, ctx->stream, d_places + p0, predictor, swap); break;
            case 4: launch_place_bps<4, false>(g, ctx->stream, d_places + p0, predictor, swap); break;
            case 8: launch_place_bps<8, false>(g, ctx->stream, d_places + p0, 1, false); break;
            default: return fail(ctx, OMR_INVALID_ARGUMENT, "tiff: bad sample width");
            }
        } else {
            switch (bps) {
            case 1: launch_place_bps<1, true>(g, ctx->stream, d_places + p0, predictor, false); break;
            case 2: launch_place_bps<2, true>(g, ctx->stream, d_places + p0, predictor, swap); break;
            case 4: launch_place_bps<4, true>(g, ctx->stream, d_places + p0, predictor, swap); break;
            case 8: launch_place_bps<8, true>(g, ctx->stream, d_places + p0, 1, false); break;
            default: return fail(ctx, OMR_INVALID_ARGUMENT, "tiff: bad sample width");
            }
        }
    }
    OMR_HIP(ctx, hipGetLastError());
    return OMR_OK;
}

}  // namespace omr

using namespace omr;

extern "C" omr_status omr_lzw_decode_batch_device(omr_ctx* ctx, const uint8_t* d_src, const uint64_t* d_offsets,
                                                  const uint32_t* d_lengths, const uint32_t* d_expected, int32_t n,
                                                  uint8_t* d_dst, const uint64_t* d_dst_offsets, int32_t* d_status) {
    if (!ctx) return OMR_INVALID_ARGUMENT;
    if (n < 0) return fail(ctx, OMR_INVALID_ARGUMENT, "lzw: negative segment count");
    if (n == 0) return OMR_OK;
    if (!d_src || !d_offsets || !d_lengths || !d_expected || !d_dst || !d_dst_offsets || !d_status)
        return fail(ctx, OMR_INVALID_ARGUMENT, "lzw: null argument");
    OMR_HIP(ctx, hipSetDevice(ctx->device));
    return launch_lzw_decode(ctx, {d_src, d_offsets, d_lengths, d_expected, nullptr, n, d_dst, d_dst_offsets, d_status});
}
