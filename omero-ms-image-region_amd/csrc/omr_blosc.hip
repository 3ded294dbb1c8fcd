// omr_blosc.hip — K15: the device half of the Blosc reader of OME-Zarr chunks (omr_zarr.cpp,
// omr_blosc.cpp).
//
// K15a k_lz4_decode: one wave per stream, many streams per launch.  An LZ4 block is byte-aligned
// sequences -- token, literals, offset, match -- with no bit reader and no tables, so the wave
// parses with wave-uniform (scalar) code through a 256-byte register window over the stream and
// collects up to 64 sequences, lane j keeping sequence j.  Then it emits the round in parallel: a
// scan of the sequences' sizes gives the output positions, the literal runs are copied from the
// input (short ones by their lanes, long ones wave-wide), one fence makes everything stored so far
// readable, the matches that read nothing a match of this round writes are copied next (short ones
// by their lanes, all at once; long ones wave-wide), and the others wave-wide in sequence order,
// behind a further fence only when their source reaches into what was stored since the last one.
// A stream flagged raw (a Blosc split that did not compress) is one wave-wide copy.
//
// K15b k_blosc_place: K13b's crop with Blosc's byte un-shuffle folded into the load: each output
// sample gathers its bytes from the still shuffled chunk, so only the requested region is read back
// and no pass over whole chunks exists.
#include "omr_internal.h"
#include "omr_wave.h"

namespace omr {

namespace {

constexpr int kKindLz4Decode = 33;    // omr_ctx_kernel_timings kinds (omr.h)
constexpr int kKindBloscPlace = 34;
constexpr uint32_t kLaneLit = 16;     // literal runs up to this long are copied by their own lane
constexpr uint32_t kLaneMatch = 32;   // and matches up to this long
constexpr uint32_t kNoDirty = 0xFFFFFFFFu;

// K15a.  Grid-stride over the streams, one wave (a workgroup of 64 threads) per stream.
//
// Bounds, by construction:
//  - input: a byte is read only at a position the parser has compared with the stream's length
//    (token, every extension byte, the two offset bytes); a literal run is checked against the
//    bytes left (lit <= len - ip) before its sequence is accepted, so the literal copies read
//    inside [0, len); the window and wave_copy load whole aligned dwords, only ones that hold a
//    byte of the stream;
//  - output: a sequence is accepted only when lit + mlen <= expected - (bytes produced, this round
//    included), and only accepted sequences are emitted, each at the position the scan of the
//    accepted sizes gives, so nothing is written behind dst_offsets[i] + expected[i]; an offset is
//    accepted only when 1 <= offset <= bytes produced before the match, so every load of a match
//    lies at or above the stream's own first output byte and below the match's store position;
//  - a raw stream is copied only when lengths[i] == expected[i];
//  - every turn of the parse loop consumes at least the token byte or ends the stream, every turn
//    of an extension loop one byte, so the work is bounded by the stream's length plus the bytes
//    produced; the copy loops are bounded by their sizes;
//  - a bad stream sets status[i] = OMR_INTERNAL and ends that stream only; the sequences accepted
//    before the bad one may have been stored (inside the slot).
// The parse and all loop conditions outside the per-lane copies come from wave-uniform values
// (readfirstlane, readlane, ballots, per-stream scalars).  One wave per workgroup: the output's
// read-after-write across lanes is ordered by wave_global_fence, at most twice per round of 64
// sequences unless matches chain on one another within the round.
__global__ void __launch_bounds__(64) k_lz4_decode(const uint8_t* __restrict__ src, const uint64_t* __restrict__ offsets,
                                                   const uint32_t* __restrict__ lengths,
                                                   const uint32_t* __restrict__ expected, const uint8_t* __restrict__ raw,
                                                   int n, uint8_t* dst, const uint64_t* __restrict__ dst_offsets,
                                                   int32_t* __restrict__ status) {
    const int lane = (int)threadIdx.x;
    for (int seg = (int)blockIdx.x; seg < n; seg += (int)gridDim.x) {
        const uint8_t* s = src + offsets[seg];
        const uint32_t len = uni(lengths[seg]), exp = uni(expected[seg]);
        uint8_t* d = dst + dst_offsets[seg];
        if (raw && uni(raw[seg])) {
            if (len == exp) wave_copy(d, s, exp, lane);
            if (lane == 0) status[seg] = len == exp ? OMR_OK : OMR_INTERNAL;
            continue;
        }
        ByteWindow in;
        in.mis = (uint32_t)(reinterpret_cast<uintptr_t>(s) & 3u);
        in.sw = reinterpret_cast<const uint32_t*>(s - in.mis);
        in.end_pos = (uint64_t)in.mis + len;
        in.r0 = in.win_lo = 0;
        in.win_valid = false;
        in.lane = lane;
        int32_t st = OMR_OK;
        uint32_t ip = 0, outpos = 0;
        bool done = false;
        while (st == OMR_OK && !done) {
            // one round: up to 64 sequences, lane j keeps sequence j
            uint32_t my_src = 0, my_lit = 0, my_mlen = 0, my_dist = 0;
            uint32_t nseq = 0, bytes = 0;
            while (nseq < 64u) {
                if (ip >= len) {                          // empty, or the input ends after a match
                    st = OMR_INTERNAL;
                    break;
                }
                const uint32_t token = in.byte(ip++);
                uint32_t lit = token >> 4;
                if (lit == 15u) {
                    uint32_t b = 255u;
                    while (b == 255u && ip < len) {
                        b = in.byte(ip++);
                        lit += b;
                        if (lit > len) break;             // more than the input holds (and no overflow)
                    }
                    if (b == 255u) {                      // the extension ran past the input
                        st = OMR_INTERNAL;
                        break;
                    }
                }
                if (lit > len - ip || lit > exp - outpos - bytes) {
                    st = OMR_INTERNAL;
                    break;
                }
                const uint32_t lsrc = ip;
                ip += lit;
                uint32_t mlen = 0, dist = 0;
                if (ip == len) {
                    done = true;                          // the last sequence: literals only
                } else {
                    if (len - ip < 2u) {
                        st = OMR_INTERNAL;
                        break;
                    }
                    dist = in.byte(ip) | in.byte(ip + 1u) << 8;
                    ip += 2u;
                    if (dist == 0u || dist > outpos + bytes + lit) {
                        st = OMR_INTERNAL;
                        break;
                    }
                    mlen = (token & 15u) + 4u;
                    if ((token & 15u) == 15u) {
                        uint32_t b = 255u;
                        while (b == 255u && ip < len) {
                            b = in.byte(ip++);
                            mlen += b;
                            if (mlen > exp) break;        // more than the output holds (and no overflow)
                        }
                        if (b == 255u) {                  // ran past the input, or past `expected`
                            st = OMR_INTERNAL;
                            break;
                        }
                    }
                    if (mlen > exp - outpos - bytes - lit) {
                        st = OMR_INTERNAL;
                        break;
                    }
                }
                const bool me = (uint32_t)lane == nseq;
                my_src = me ? lsrc : my_src;
                my_lit = me ? lit : my_lit;
                my_mlen = me ? mlen : my_mlen;
                my_dist = me ? dist : my_dist;
                ++nseq;
                bytes += lit + mlen;
                if (done) break;
            }
            if (st != OMR_OK) break;
            // emit: positions by a scan; the literals come from the input and wait for nothing
            const bool valid = (uint32_t)lane < nseq;
            const uint32_t size = valid ? my_lit + my_mlen : 0u;
            const uint32_t pos = outpos + wave_incl_scan(size, lane) - size;
            const uint32_t mpos = pos + my_lit;
            if (valid && my_lit <= kLaneLit)
                for (uint32_t k = 0; k < my_lit; ++k) d[pos + k] = s[my_src + k];
            unsigned long long mm = __ballot(valid && my_lit > kLaneLit);
            while (mm) {
                const uint32_t j = (uint32_t)__ffsll((long long)mm) - 1u;
                mm &= mm - 1ull;
                wave_copy(d + lane_value(pos, j), s + lane_value(my_src, j), lane_value(my_lit, j), lane);
            }
            const bool is_match = valid && my_mlen != 0u;
            const unsigned long long all = __ballot(is_match);
            if (all) {
                // One fence per round with a match: the rounds before and this round's literals
                // are readable behind it.  A match is free when its source lies below the round's
                // first match or inside its own sequence's literals: it reads nothing a match of
                // this round stores.  [start, start + min(length, distance)) is the whole source: a
                // match with distance < length repeats its period.
                wave_global_fence();
                const uint32_t first = lane_value(mpos, (uint32_t)__ffsll((long long)all) - 1u);
                const uint32_t start = mpos - my_dist, send = start + min(my_mlen, my_dist);
                const bool free_m = is_match && (send <= first || start >= pos);
                if (free_m && my_mlen <= kLaneMatch) {
                    uint32_t q = 0;
                    for (uint32_t k = 0; k < my_mlen; ++k) {
                        d[mpos + k] = d[start + q];
                        q = q + 1u == my_dist ? 0u : q + 1u;
                    }
                }
                mm = __ballot(free_m && my_mlen > kLaneMatch);
                while (mm) {
                    const uint32_t j = (uint32_t)__ffsll((long long)mm) - 1u;
                    mm &= mm - 1ull;
                    wave_match(d, lane_value(mpos, j), lane_value(my_mlen, j), lane_value(my_dist, j), lane);
                }
                // the others in sequence order; [dirty_lo, dirty_hi) spans the match output stored since
                // the last fence: a source that touches it waits for a fence, one among literals and
                // fenced output does not.  The round's first match is always free (its source ends at
                // or below itself), so free matches were just stored, all at or above `first`.
                uint32_t dirty_lo = first, dirty_hi = kNoDirty;
                mm = __ballot(is_match && !free_m);
                while (mm) {
                    const uint32_t j = (uint32_t)__ffsll((long long)mm) - 1u;
                    mm &= mm - 1ull;
                    const uint32_t mp = lane_value(mpos, j), ml = lane_value(my_mlen, j), md = lane_value(my_dist, j);
                    if (mp - md < dirty_hi && mp - md + min(ml, md) > dirty_lo) {
                        wave_global_fence();
                        dirty_lo = kNoDirty;
                        dirty_hi = 0u;
                    }
                    wave_match(d, mp, ml, md, lane);
                    dirty_lo = min(dirty_lo, mp);
                    dirty_hi = max(dirty_hi, mp + ml);
                }
            }
            outpos += bytes;
        }
        if (st == OMR_OK && outpos != exp) st = OMR_INTERNAL;
        if (lane == 0) status[seg] = st;
    }
}

template <int BPS> struct SampleOf;
template <> struct SampleOf<1> { typedef uint8_t T; };
template <> struct SampleOf<2> { typedef uint16_t T; };
template <> struct SampleOf<4> { typedef uint32_t T; };
template <> struct SampleOf<8> { typedef uint64_t T; };

// K15b.  blockIdx.y: the placement; the waves of the grid's x dimension stride over its rows.
// Decoded byte o of the chunk lies in block b = o / blocksize of nb = min(blocksize, nbytes - b
// blocksize) bytes, q = nb / typesize elements: at i = (o - b blocksize) / typesize below q, byte j
// of element i is the block's byte j q + i; the nb mod typesize bytes behind the elements stay in
// place.  Every load is inside [0, nbytes): j q + i < typesize q <= nb, and the sample lies inside
// the chunk (x < x1 <= seg_w, y < y1 <= the chunk's rows, nbytes == rows seg_w BPS: the host
// checked the header against the chunk's size); every store is inside the placement's rectangle,
// which the host clipped to the region and the image.  Not shuffled, or typesize 1: a plain crop.
template <int BPS>
__global__ void __launch_bounds__(256) k_blosc_place(const BloscPlace* __restrict__ places) {
    typedef typename SampleOf<BPS>::T T;
    const BloscPlace P = places[blockIdx.y];
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    const int rows = P.y1 - P.y0;
    // the usual case: samples are the shuffled elements and blocks hold whole ones
    const bool element = P.typesize == (uint32_t)BPS && P.blocksize % (uint32_t)BPS == 0u;
    for (int r = (int)blockIdx.x * 4 + wave; r < rows; r += (int)gridDim.x * 4) {
        T* drow = reinterpret_cast<T*>(P.dst) + (int64_t)r * P.dst_pitch;
        const uint32_t row0 = (uint32_t)(P.y0 + r) * (uint32_t)P.seg_w;      // samples; below nbytes / BPS < 2^31
        if (!P.src) {
            for (int x = P.x0 + lane; x < P.x1; x += 64) drow[x - P.x0] = (T)0;
        } else if (!P.shuffled) {
            const T* srow = reinterpret_cast<const T*>(P.src) + row0;
            for (int x = P.x0 + lane; x < P.x1; x += 64) drow[x - P.x0] = srow[x];
        } else if (element) {
            for (int x = P.x0 + lane; x < P.x1; x += 64) {
                const uint32_t o = (row0 + (uint32_t)x) * (uint32_t)BPS;
                const uint32_t b0 = o / P.blocksize * P.blocksize;
                const uint32_t q = min(P.blocksize, P.nbytes - b0) / (uint32_t)BPS, i = (o - b0) / (uint32_t)BPS;
                const uint8_t* blk = P.src + b0;
                T v = 0;                                  // i < q: blocks and the chunk hold whole samples
#pragma unroll
                for (int j = 0; j < BPS; ++j) v |= (T)((T)blk[(uint32_t)j * q + i] << (8 * j));
                drow[x - P.x0] = v;
            }
        } else {
            for (int x = P.x0 + lane; x < P.x1; x += 64) {
                T v = 0;
#pragma unroll
                for (int j = 0; j < BPS; ++j) {
                    const uint32_t o = (row0 + (uint32_t)x) * (uint32_t)BPS + (uint32_t)j;
                    const uint32_t b0 = o / P.blocksize * P.blocksize, ob = o - b0;
                    const uint32_t q = min(P.blocksize, P.nbytes - b0) / P.typesize, i = ob / P.typesize;
                    const uint32_t at = i < q ? (ob - i * P.typesize) * q + i : ob;
                    v |= (T)((T)P.src[b0 + at] << (8 * j));
                }
                drow[x - P.x0] = v;
            }
        }
    }
}

}  // namespace

omr_status launch_lz4_decode(Ctx* ctx, const StreamTable& t) {
    if (t.n <= 0) return OMR_OK;
    // no LDS; 103 SGPRs (52 VGPRs would allow 8) hold the kernel to 7 waves per SIMD, so 28 of the 32
    // one-wave workgroups launched per CU are resident at once and the rest follow by the grid stride
    const int blocks = std::min(t.n, std::max(1, ctx->cu_count) * 32);
    KernelTimer timer(ctx, kKindLz4Decode, true);
    omr_launch(k_lz4_decode, dim3((unsigned)blocks), dim3(64), 0u, ctx->stream, t.src, t.offsets, t.lengths, t.expected,
               t.raw, (int)t.n, t.dst, t.dst_offsets, t.status);
    OMR_HIP(ctx, hipGetLastError());
    return OMR_OK;
}

omr_status launch_blosc_place(Ctx* ctx, const BloscPlace* d_places, int32_t n, int32_t max_rows, int32_t bps) {
    if (n <= 0 || max_rows <= 0) return OMR_OK;
    if (bps != 1 && bps != 2 && bps != 4 && bps != 8) return fail(ctx, OMR_INVALID_ARGUMENT, "blosc: bad sample width");
    KernelTimer timer(ctx, kKindBloscPlace, true);
    for (int32_t p0 = 0; p0 < n; p0 += 65535) {           // grid y limit
        const dim3 g((unsigned)std::min(64, (max_rows + 3) / 4), (unsigned)std::min(65535, n - p0));
        switch (bps) {
        case 1: omr_launch(k_blosc_place<1>, g, dim3(256), 0u, ctx->stream, d_places + p0); break;
        case 2: omr_launch(k_blosc_place<2>, g, dim3(256), 0u, ctx->stream, d_places + p0); break;
        case 4: omr_launch(k_blosc_place<4>, g, dim3(256), 0u, ctx->stream, d_places + p0); break;
        default: omr_launch(k_blosc_place<8>, g, dim3(256), 0u, ctx->stream, d_places + p0); break;
        }
    }
    OMR_HIP(ctx, hipGetLastError());
    return OMR_OK;
}

}  // namespace omr

using namespace omr;

extern "C" omr_status omr_lz4_decode_batch_device(omr_ctx* ctx, const uint8_t* d_src, const uint64_t* d_offsets,
                                                  const uint32_t* d_lengths, const uint32_t* d_expected, int32_t n,
                                                  uint8_t* d_dst, const uint64_t* d_dst_offsets, int32_t* d_status) {
    if (!ctx) return OMR_INVALID_ARGUMENT;
    if (n < 0) return fail(ctx, OMR_INVALID_ARGUMENT, "lz4: negative stream count");
    if (n == 0) return OMR_OK;
    if (!d_src || !d_offsets || !d_lengths || !d_expected || !d_dst || !d_dst_offsets || !d_status)
        return fail(ctx, OMR_INVALID_ARGUMENT, "lz4: null argument");
    OMR_HIP(ctx, hipSetDevice(ctx->device));
    return launch_lz4_decode(ctx, {d_src, d_offsets, d_lengths, d_expected, nullptr, n, d_dst, d_dst_offsets, d_status});
}
