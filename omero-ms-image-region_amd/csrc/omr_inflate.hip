// omr_inflate.hip — K14a: zlib (RFC 1950 / 1951) streams inflated on the device, the decoder of
// the OME-Zarr reader (omr_zarr.cpp).
//
// k_inflate: one wave per stream, many streams per launch.  Huffman decoding is serial in the
// stream, so the wave decodes with wave-uniform (scalar) code -- a 64-bit bit buffer refilled from a
// register window over the stream, two-level tables in LDS -- and collects up to 64 symbols, lane
// j keeping symbol j.  Then the wave emits the batch in parallel: an exclusive scan of the symbols'
// lengths gives the output positions, the literals are stored by their lanes, the matches that
// depend on nothing of the batch are copied by their lanes, and the others wave-wide in symbol order.
#include "omr_internal.h"

namespace omr {

namespace {

constexpr int kKindInflate = 32;   // omr_ctx_kernel_timings kind (omr.h)
constexpr int kLitFast = 10;       // bits of the first-level literal/length table
constexpr int kDistFast = 9;       // and of the distance table (also holds the 7-bit code-length table)
constexpr uint32_t kBadSymbol = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint32_t lane_value(uint32_t v, uint32_t l) {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)uni(l & 63u));
}

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    return v;
}

// Orders the LDS traffic of a one-wave workgroup (as in omr_tiffread.hip): no instruction, the
// compiler keeps the accesses in program order and the LDS serves a wave's accesses in issue order.
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Orders this wave's global stores before its later global loads of the same bytes from other
// lanes: a match copies output that other lanes of the wave stored (up to 32 KiB back, possibly in
// the same batch), and the Adler-32 pass reads all of it.  The mechanism chosen is the output
// buffer itself as the window, with a workgroup-scope acquire-release fence between the stores and
// the loads.  It is sufficient because the workgroup is this one wave on one CU: a workgroup-scope
// release makes the wave wait until its stores have been performed at the CU's (write-through)
// vector L1 and the L2 behind it (s_waitcnt vmcnt(0)), and the loads that follow go through that
// same L1, which a store of its own CU never leaves stale; nothing of another CU is involved, so no
// agent-scope write-back or invalidate is needed.  The explicit wait is there because the fence's
// own wait may be dropped by the compiler when it sees no store it must wait for.  A 32 KiB LDS
// window instead would cost occupancy: 160 KiB / (32 KiB + tables) = 4 waves per CU against the 8
// and more this form allows.
__device__ __forceinline__ void wave_global_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

// The stream, LSB first.  It is read through a 256-byte window held in one register per lane (dword
// win_lo + lane), loaded with one aligned dword load counted from sw, the dword that holds s[0];
// only dwords that hold a byte of the stream are loaded, the others read as zero.  (One register,
// not K13a's four: a choice among four registers by a wave-uniform index made the compiler keep the
// whole reader in scratch memory.)  All members but the window register are wave-uniform.  bitpos
// counts the bits consumed from s[0]; the decoder compares it with the stream's length after every
// symbol, so zeros read behind the end are never taken for data.
struct BitReader {
    const uint32_t* sw;
    uint64_t end_pos;     // bytes from sw to the end of the stream
    uint32_t mis;         // bytes from sw to s[0]
    uint32_t r0, win_lo;
    bool win_valid;
    uint32_t dw;          // next dword to append to the bit buffer
    uint64_t bb;
    uint32_t bcnt;
    uint64_t bitpos;
    int lane;

    __device__ __forceinline__ uint32_t fetch(uint32_t k) {
        if (!win_valid || k < win_lo || k - win_lo >= 64u) {
            win_lo = k;
            const uint64_t d0 = (uint64_t)k + (uint64_t)lane;
            r0 = (d0 << 2) < end_pos ? sw[d0] : 0u;
            win_valid = true;
        }
        return lane_value(r0, k - win_lo);
    }
    // at least 33 bits in the buffer
    __device__ __forceinline__ void refill() {
        while (bcnt <= 32u) {
            bb |= (uint64_t)fetch(dw) << bcnt;
            ++dw;
            bcnt += 32u;
        }
    }
    __device__ __forceinline__ void skip(uint32_t n) {     // n <= bcnt
        bb >>= n;
        bcnt -= n;
        bitpos += n;
    }
    __device__ __forceinline__ uint32_t take(uint32_t n) {  // n <= 16, n <= bcnt
        const uint32_t v = (uint32_t)bb & ((1u << n) - 1u);
        skip(n);
        return v;
    }
    __device__ __forceinline__ void seek(uint64_t byte) {   // byte <= the stream's length
        const uint64_t p = (uint64_t)mis + byte;
        dw = (uint32_t)(p >> 2);
        bb = 0;
        bcnt = 0;
        refill();
        const uint32_t drop = 8u * (uint32_t)(p & 3u);
        bb >>= drop;
        bcnt -= drop;
        bitpos = byte * 8u;
    }
};

// A canonical Huffman code for `n` symbols with the lengths lens[0, n) (LDS), built by the wave:
// fast[code reversed, padded to FB bits] = symbol | length << 9 for the codes of up to FB bits (0:
// no such code), count[l] = codes of length l and sorted[] = the symbols by (length, value) for
// the bit-by-bit decode of the longer ones.  The rank of a symbol among those of its length comes
// from ballots, so no lane waits for another.  false: the set is over-subscribed, or incomplete
// with anything but codes of one bit (zlib's rule: a single one-bit code, or none, may stay
// incomplete).  Indices: fast[] by a code below 2^FB (the set is not over-subscribed, so a code of
// l bits is below 2^l) and a loop bound; sorted[] clamped to nsorted.
template <int FB>
__device__ bool build_table(const uint8_t* lens, int n, uint16_t* fast, uint16_t* count, uint16_t* sorted, int nsorted,
                            int lane) {
    for (int i = lane; i < (1 << FB); i += 64) fast[i] = 0;
    uint32_t cnt[16];
#pragma unroll
    for (int l = 0; l < 16; ++l) cnt[l] = 0;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        const uint32_t ml = i < n ? (uint32_t)(lens[i] & 15u) : 0u;
#pragma unroll
        for (int l = 1; l < 16; ++l) cnt[l] += (uint32_t)__popcll(__ballot(ml == (uint32_t)l));
    }
    int left = 1;
    bool over = false;
    uint32_t used = 0;
#pragma unroll
    for (int l = 1; l < 16; ++l) {
        left = left * 2 - (int)cnt[l];
        over = over || left < 0;
        used += cnt[l];
    }
    if (over || (left > 0 && used != cnt[1])) return false;
#pragma unroll
    for (int l = 0; l < 16; ++l) count[l] = (uint16_t)cnt[l];    // every lane the same value
    uint32_t run[16];
#pragma unroll
    for (int l = 0; l < 16; ++l) run[l] = 0;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        const uint32_t ml = i < n ? (uint32_t)(lens[i] & 15u) : 0u;
        uint32_t my_idx = 0, my_code = 0, offs = 0, first = 0;
#pragma unroll
        for (int l = 1; l < 16; ++l) {
            if (l > 1) first = (first + cnt[l - 1]) << 1;         // first code of length l
            const unsigned long long m = __ballot(ml == (uint32_t)l);
            if (ml == (uint32_t)l) {
                const uint32_t r = run[l] + (uint32_t)__popcll(m & below);
                my_idx = offs + r;
                my_code = first + r;
            }
            run[l] += (uint32_t)__popcll(m);
            offs += cnt[l];
        }
        if (ml) {
            sorted[min(my_idx, (uint32_t)nsorted - 1u)] = (uint16_t)i;
            if (ml <= (uint32_t)FB) {
                const uint32_t rev = __brev(my_code) >> (32u - ml);
                for (uint32_t e = rev; e < (1u << FB); e += 1u << ml) fast[e] = (uint16_t)((uint32_t)i | ml << 9);
            }
        }
    }
    wave_lds_fence();
    return true;
}

// One symbol: the first-level table, else bit by bit along the canonical code (as Mark Adler's
// puff does).  kBadSymbol: no such code.  Needs 15 bits in the buffer.
template <int FB>
__device__ __forceinline__ uint32_t decode_symbol(BitReader& br, const uint16_t* fast, const uint16_t* count,
                                                  const uint16_t* sorted, int nsorted) {
    const uint32_t e = uni(fast[(uint32_t)br.bb & ((1u << FB) - 1u)]);
    if (e >> 9) {
        br.skip(e >> 9);
        return e & 511u;
    }
    int code = 0, first = 0, index = 0;
    for (uint32_t l = 1; l < 16u; ++l) {
        code |= (int)((br.bb >> (l - 1u)) & 1u);
        const int c = (int)uni(count[l]);
        if (code - c < first) {
            const uint32_t at = (uint32_t)(index + (code - first));
            br.skip(l);
            return uni(sorted[min(at, (uint32_t)nsorted - 1u)]);
        }
        index += c;
        first += c;
        first <<= 1;
        code <<= 1;
    }
    return kBadSymbol;
}

// K14a.  Grid-stride over the streams, one wave (a workgroup of 64 threads) per stream.
//
// Bounds, by construction:
//  - table indices: fast[] by the low FB bits of the bit buffer, count[] by a loop counter below
//    16, sorted[] clamped to its size, lens[] by a position checked against HLIT + HDIST (at most
//    316 of 352 entries) before the store;
//  - every output store is guarded by p < expected, so nothing is written behind dst_offsets[i] +
//    expected[i]; every output load of a match is below its own store position;
//  - a symbol (a block header, a code length) is only taken when all its bits lie inside the
//    stream: bitpos <= 8 * length is checked after each, and the words behind the stream read as
//    zero without being loaded; a stored block's bytes are checked against the stream's length
//    before the copy;
//  - a distance larger than the bytes produced so far is an error;
//  - every turn of every loop consumes at least one bit of the stream or ends the stream, so the
//    work is bounded by the stream's bit length (the table builders and the copies are bounded by
//    their sizes);
//  - a bad stream sets status[i] = OMR_INTERNAL and ends that stream only.
// All loop conditions come from wave-uniform values (readfirstlane, readlane, ballots, per-stream
// scalars), so control flow never diverges outside the guarded stores and the per-lane match copy; one wave per workgroup, so
// LDS traffic is ordered by wave_lds_fence and the output's read-after-write by wave_global_fence.
__global__ void __launch_bounds__(64) k_inflate(const uint8_t* __restrict__ src, const uint64_t* __restrict__ offsets,
                                                const uint32_t* __restrict__ lengths,
                                                const uint32_t* __restrict__ expected, int n, uint8_t* dst,
                                                const uint64_t* __restrict__ dst_offsets, int32_t* __restrict__ status) {
    __shared__ uint16_t litfast[1 << kLitFast];
    __shared__ uint16_t distfast[1 << kDistFast];
    __shared__ uint16_t litsorted[288], distsorted[32];
    __shared__ uint16_t litcount[16], distcount[16];
    __shared__ uint8_t lens[352];                 // [0, 320): literal/length + distance; [320, 339): code-length code
    const int lane = (int)threadIdx.x;
    for (int seg = (int)blockIdx.x; seg < n; seg += (int)gridDim.x) {
        const uint8_t* s = src + offsets[seg];
        const uint32_t len = lengths[seg], exp = expected[seg];
        uint8_t* d = dst + dst_offsets[seg];
        const uint64_t nbits = (uint64_t)len * 8u;
        int32_t st = OMR_OK;
        uint32_t outpos = 0;
        uint32_t fenced = 0;        // output below this was stored before the last wave_global_fence
        int tables = 0;             // 1: the fixed code is in the tables
        BitReader br;
        br.mis = (uint32_t)(reinterpret_cast<uintptr_t>(s) & 3u);
        br.sw = reinterpret_cast<const uint32_t*>(s - br.mis);
        br.end_pos = (uint64_t)br.mis + len;
        br.r0 = br.win_lo = 0;
        br.win_valid = false;
        br.lane = lane;
        br.dw = 0; br.bb = 0; br.bcnt = 0; br.bitpos = 0;
        if (len < 2u) {
            st = OMR_INTERNAL;
        } else {
            br.seek(0);
            const uint32_t cmf = br.take(8), flg = br.take(8);
            if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u != 0u || (flg & 0x20u)) st = OMR_INTERNAL;
        }
        bool last = false;
        while (st == OMR_OK && !last) {
            br.refill();
            last = br.take(1) != 0u;
            const uint32_t type = br.take(2);
            if (br.bitpos > nbits || type == 3u) {
                st = OMR_INTERNAL;
                break;
            }
            if (type == 0u) {
                br.skip((uint32_t)(0u - (uint32_t)br.bitpos) & 7u);
                br.refill();
                const uint32_t cnt = br.take(16), ncnt = br.take(16);
                const uint64_t from = br.bitpos >> 3;
                if (br.bitpos > nbits || (cnt ^ 0xFFFFu) != ncnt || from + cnt > (uint64_t)len || cnt > exp - outpos) {
                    st = OMR_INTERNAL;
                    break;
                }
                for (uint32_t k = (uint32_t)lane; k < cnt; k += 64u) {
                    const uint32_t p = outpos + k;
                    if (p < exp) d[p] = s[from + k];
                }
                outpos += cnt;
                br.seek(from + cnt);
                continue;
            }
            wave_lds_fence();       // the block before is done with the tables
            if (type == 1u) {
                if (tables != 1) {
                    for (int k = lane; k < 320; k += 64)
                        lens[k] = k < 144 ? 8 : k < 256 ? 9 : k < 280 ? 7 : k < 288 ? 8 : 5;
                    wave_lds_fence();
                    build_table<kLitFast>(lens, 288, litfast, litcount, litsorted, 288, lane);
                    build_table<kDistFast>(lens + 288, 32, distfast, distcount, distsorted, 32, lane);
                    tables = 1;
                }
            } else {
                tables = 2;
                const uint32_t hlit = br.take(5) + 257u, hdist = br.take(5) + 1u, hclen = br.take(4) + 4u;
                if (br.bitpos > nbits || hlit > 286u || hdist > 30u) {
                    st = OMR_INTERNAL;
                    break;
                }
                if (lane < 19) lens[320 + lane] = 0;
                wave_lds_fence();
                for (uint32_t k = 0; k < hclen; ++k) {
                    br.refill();
                    const uint32_t v = br.take(3);
                    // the order of RFC 1951 3.2.7: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
                    const uint32_t at = k < 3u ? 16u + k : k == 3u ? 0u : (k & 1u) ? (19u - k) / 2u : 6u + k / 2u;
                    if (lane == 0) lens[320u + min(at, 18u)] = (uint8_t)v;
                }
                if (br.bitpos > nbits) {
                    st = OMR_INTERNAL;
                    break;
                }
                wave_lds_fence();
                if (!build_table<7>(lens + 320, 19, distfast, distcount, distsorted, 32, lane)) {
                    st = OMR_INTERNAL;
                    break;
                }
                const uint32_t total = hlit + hdist;      // <= 316
                uint32_t k = 0, prev = 0;
                while (k < total) {
                    br.refill();
                    const uint32_t sym = decode_symbol<7>(br, distfast, distcount, distsorted, 32);
                    if (sym == kBadSymbol || sym > 18u) {
                        st = OMR_INTERNAL;
                        break;
                    }
                    uint32_t v = sym, rep = 1;
                    if (sym == 16u) {
                        if (k == 0u) {                    // nothing to repeat
                            st = OMR_INTERNAL;
                            break;
                        }
                        v = prev;
                        rep = 3u + br.take(2);
                    } else if (sym == 17u) {
                        v = 0;
                        rep = 3u + br.take(3);
                    } else if (sym == 18u) {
                        v = 0;
                        rep = 11u + br.take(7);
                    }
                    if (br.bitpos > nbits || rep > total - k) {
                        st = OMR_INTERNAL;
                        break;
                    }
                    for (uint32_t j = (uint32_t)lane; j < rep; j += 64u) lens[k + j] = (uint8_t)v;   // k + j < total <= 316
                    k += rep;
                    prev = v;
                }
                if (st != OMR_OK) break;
                wave_lds_fence();
                if (uni(lens[256]) == 0u) {               // no end-of-block code
                    st = OMR_INTERNAL;
                    break;
                }
                if (!build_table<kLitFast>(lens, (int)hlit, litfast, litcount, litsorted, 288, lane) ||
                    !build_table<kDistFast>(lens + hlit, (int)hdist, distfast, distcount, distsorted, 32, lane)) {
                    st = OMR_INTERNAL;
                    break;
                }
            }
            // the block's symbols, in batches of up to 64: packed = length | distance << 9 for a match,
            // 0 | byte << 9 for a literal
            bool eob = false;
            while (st == OMR_OK && !eob) {
                uint32_t mine = 0, nsym = 0, bytes = 0;
                while (nsym < 64u) {
                    br.refill();
                    const uint32_t sym = decode_symbol<kLitFast>(br, litfast, litcount, litsorted, 288);
                    if (sym == kBadSymbol || br.bitpos > nbits) {
                        st = OMR_INTERNAL;
                        break;
                    }
                    uint32_t packed, L;
                    if (sym < 256u) {
                        packed = sym << 9;
                        L = 1;
                    } else if (sym == 256u) {
                        eob = true;
                        break;
                    } else if (sym > 285u) {
                        st = OMR_INTERNAL;
                        break;
                    } else {
                        const uint32_t i = sym - 257u;
                        if (i < 8u) {
                            L = 3u + i;
                        } else if (i == 28u) {
                            L = 258u;
                        } else {
                            const uint32_t x = (i - 4u) >> 2;
                            L = 3u + ((4u + (i & 3u)) << x) + br.take(x);
                        }
                        br.refill();
                        const uint32_t ds = decode_symbol<kDistFast>(br, distfast, distcount, distsorted, 32);
                        if (ds == kBadSymbol || ds > 29u) {
                            st = OMR_INTERNAL;
                            break;
                        }
                        uint32_t dist;
                        if (ds < 4u) {
                            dist = 1u + ds;
                        } else {
                            const uint32_t x = (ds - 2u) >> 1;
                            dist = 1u + ((2u + (ds & 1u)) << x) + br.take(x);
                        }
                        if (br.bitpos > nbits || dist > outpos + bytes) {
                            st = OMR_INTERNAL;
                            break;
                        }
                        packed = L | dist << 9;
                    }
                    if (L > exp - outpos - bytes) {       // more than `expected`
                        st = OMR_INTERNAL;
                        break;
                    }
                    mine = (uint32_t)lane == nsym ? packed : mine;
                    ++nsym;
                    bytes += L;
                }
                if (st != OMR_OK) break;
                // emit: positions by a scan, literals by their lanes, then the matches
                const bool valid = (uint32_t)lane < nsym;
                const uint32_t mlen_l = mine & 511u;
                const bool is_lit = mlen_l == 0u;
                const uint32_t L = valid ? (is_lit ? 1u : mlen_l) : 0u;
                const uint32_t pos = outpos + wave_incl_scan(L, lane) - L;
                if (valid && is_lit && pos < exp) d[pos] = (uint8_t)(mine >> 9);
                const bool is_match = valid && !is_lit;
                unsigned long long mm = __ballot(is_match);
                if (mm) {
                    // One fence per batch with a match: the stores of the batches before have had the
                    // time of this batch's serial decode to complete, so the wait is short, and it makes
                    // everything below the batch's start safe to read.  A match whose source lies
                    // wholly below the start depends on nothing of this batch: those are copied first,
                    // each by its own lane, all lanes at once (the only divergent loop of the kernel,
                    // bounded by the match length).  The source is [start, start + min(length,
                    // distance)): a match with distance < length replicates its period, so no byte of
                    // it is read from the match's own output.
                    wave_global_fence();
                    fenced = outpos;
                    const uint32_t mdist_l = mine >> 9, start_l = pos - mdist_l;   // mdist <= bytes before the symbol: checked above
                    const bool indep = is_match && start_l + min(mlen_l, mdist_l) <= outpos;
                    if (indep) {
                        for (uint32_t k = 0; k < mlen_l; ++k) {
                            const uint32_t p = pos + k;
                            if (p < exp) d[p] = d[start_l + (k >= mdist_l ? k % mdist_l : k)];
                        }
                    }
                    mm = __ballot(is_match && !indep);
                }
                // the other matches wave-wide, in symbol order, behind a fence of their own when their
                // source reaches above the last one
                while (mm) {
                    const uint32_t j = (uint32_t)__ffsll((long long)mm) - 1u;
                    mm &= mm - 1ull;
                    const uint32_t mpos = lane_value(pos, j), mlen = lane_value(mlen_l, j), mdist = lane_value(mine >> 9, j);
                    const uint32_t start = mpos - mdist;
                    if (start + min(mlen, mdist) > fenced) {
                        wave_global_fence();
                        fenced = mpos;
                    }
                    for (uint32_t k = (uint32_t)lane; k < mlen; k += 64u) {
                        const uint32_t p = mpos + k;
                        if (p < exp) d[p] = d[start + (k >= mdist ? k % mdist : k)];
                    }
                }
                outpos += bytes;
            }
        }
        if (st == OMR_OK && outpos != exp) st = OMR_INTERNAL;
        if (st == OMR_OK) {
            br.skip((uint32_t)(0u - (uint32_t)br.bitpos) & 7u);
            br.refill();
            const uint32_t want = __builtin_bswap32((uint32_t)br.bb);
            br.skip(32);
            if (br.bitpos > nbits) {
                st = OMR_INTERNAL;
            } else {
                // Adler-32 of the output, a second pass by the wave over what it wrote: a = 1 + sum d[i],
                // b = n + sum (n - i) d[i], both mod 65521 (the sums stay below 2^63 for n <= 256 MiB)
                wave_global_fence();
                uint64_t sa = 0, sb = 0;
                for (uint32_t i = (uint32_t)lane; i < exp; i += 64u) {
                    const uint64_t v = d[i];
                    sa += v;
                    sb += v * (uint64_t)(exp - i);
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    sa += (uint64_t)__shfl_xor((unsigned long long)sa, o);
                    sb += (uint64_t)__shfl_xor((unsigned long long)sb, o);
                }
                const uint32_t a = (uint32_t)((1u + sa) % 65521u), b = (uint32_t)((exp % 65521u + sb % 65521u) % 65521u);
                if (want != (b << 16 | a)) st = OMR_INTERNAL;
            }
        }
        if (lane == 0) status[seg] = st;
        wave_lds_fence();
    }
}

}  // namespace

omr_status launch_inflate(Ctx* ctx, const StreamTable& t) {
    if (t.n <= 0) return OMR_OK;
    // about 5 KiB of LDS per wave, so registers and the 32-wave limit set the residency; 16 waves per CU
    const int blocks = std::min(t.n, std::max(1, ctx->cu_count) * 16);
    KernelTimer timer(ctx, kKindInflate, true);
    omr_launch(k_inflate, dim3((unsigned)blocks), dim3(64), 0u, ctx->stream, t.src, t.offsets, t.lengths, t.expected,
               (int)t.n, t.dst, t.dst_offsets, t.status);
    OMR_HIP(ctx, hipGetLastError());
    return OMR_OK;
}

}  // namespace omr

using namespace omr;

extern "C" omr_status omr_inflate_batch_device(omr_ctx* ctx, const uint8_t* d_src, const uint64_t* d_offsets,
                                               const uint32_t* d_lengths, const uint32_t* d_expected, int32_t n,
                                               uint8_t* d_dst, const uint64_t* d_dst_offsets, int32_t* d_status) {
    if (!ctx) return OMR_INVALID_ARGUMENT;
    if (n < 0) return fail(ctx, OMR_INVALID_ARGUMENT, "inflate: negative stream count");
    if (n == 0) return OMR_OK;
    if (!d_src || !d_offsets || !d_lengths || !d_expected || !d_dst || !d_dst_offsets || !d_status)
        return fail(ctx, OMR_INVALID_ARGUMENT, "inflate: null argument");
    OMR_HIP(ctx, hipSetDevice(ctx->device));
    return launch_inflate(ctx, {d_src, d_offsets, d_lengths, d_expected, nullptr, n, d_dst, d_dst_offsets, d_status});
}
