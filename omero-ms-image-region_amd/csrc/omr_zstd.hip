// omr_zstd.hip — K16: the device half of the Zstandard reader of OME-Zarr chunks (omr_zstd.cpp is
// the host half and the rule; omr_zarr.cpp stages the chunks).
//
// K16a k_zstd_decode: one wave per frame, many frames per launch.  The blocks of a frame depend on
// one another through the repeat offsets, the repeat and treeless tables and the window, so a frame
// is the unit of independence; inside it the wave divides the work by what each part allows:
//  - headers and the FSE table descriptions are read by lane 0 in ordinary per-lane code (a few
//    hundred dependent steps per block) and its results are broadcast with readlane; the FSE tables
//    (2^9, 2^8, 2^9 entries) and the Huffman table (2^11) live in LDS, 11 KiB per wave;
//  - the Huffman table is filled by all lanes: four symbols per lane, one scan of the packed
//    per-weight counts gives every symbol its first entry, short ranges are stored by their lane and
//    long ones wave-wide;
//  - the one or four Huffman streams of a block are decoded by one or four lanes, each with its own
//    backward bit reader (a 64-bit window over its stream), into the workgroup's literal buffer;
//  - the three-state FSE chain of the sequences is serial: lane 0 decodes a round of up to 64
//    sequences, resolves the repeat offsets and checks every length against the literals and the
//    output left, then the wave emits the round as K15a does (omr_blosc.hip): a scan gives the
//    positions, the literal runs are copied, one fence, the matches that read nothing this round's
//    matches write are copied together and the others in order;
//  - raw and RLE blocks and the literals behind the last sequence are wave-wide copies and fills;
//  - the content checksum, when flagged, is taken behind a fence by four lanes, one per XXH64
//    accumulator, striding the output in 32-byte stripes.
//
// Bounds, by construction:
//  - input: lane 0 compares every header position with the block's or the frame's end before it
//    reads there; the bit readers load a byte only at an index inside [0, length of their stream)
//    and read zeros elsewhere, and a Huffman symbol is taken only while bits of its stream are left;
//    raw literals are checked against the block's end before they are used; wave_copy loads whole
//    aligned dwords, only ones that hold a byte of its source;
//  - tables: every index is masked to its table's size; an FSE description is accepted only when it
//    sums to its table's size with symbols below the alphabet's, Huffman weights only when they are
//    at most 11 and complete a power of two of at most 2^11, so every ranged store ends inside;
//  - literal buffer: a block's literals are at most 128 KiB, the size of the workgroup's slot, and
//    a stream's lane stores only below its own count;
//  - output: lane 0 accepts a sequence only when its literals are left in the block and literals
//    plus match fit in expected - (bytes produced, this round included), and only when 1 <= offset
//    <= bytes produced before the match; only accepted rounds are emitted, each sequence at the
//    position the scan of the accepted sizes gives; raw and RLE blocks and trailing literals are
//    checked against expected - produced first.  So every store lies below dst_offsets[i] +
//    expected[i] and every load of a match at or above the frame's first output byte;
//  - every loop consumes input (a block header, a sequence, a symbol, a stripe) or ends the frame;
//  - control flow around fences and loop exits is wave-uniform: it comes from per-frame scalars,
//    readlane broadcasts of lane 0's results and ballots;
//  - a bad frame sets status[i] = OMR_INTERNAL and ends that frame only; what was accepted before
//    may have been stored (inside the slot).
#include "omr_segread.h"
#include "omr_wave.h"

namespace omr {

namespace {

constexpr int kKindZstdDecode = 35;   // omr_ctx_kernel_timings kinds (omr.h)
constexpr uint32_t kZBlockMax = 128u << 10;
constexpr uint32_t kLaneLit = 16;     // as K15a
constexpr uint32_t kLaneMatch = 32;
constexpr uint32_t kNoDirty = 0xFFFFFFFFu;
constexpr uint32_t kLaneFill = 32;    // Huffman table ranges up to this long are stored by their lane

__device__ const int16_t kLLDefault[36] = {4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1};
__device__ const int16_t kOFDefault[29] = {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1};
__device__ const int16_t kMLDefault[53] = {1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                                           1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1};
__device__ const uint32_t kLLBase[36] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 18, 20, 22, 24, 28, 32, 40,
                                         48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536};
__device__ const uint8_t kLLBits[36] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
__device__ const uint32_t kMLBase[53] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29,
                                         30, 31, 32, 33, 34, 35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099,
                                         8195, 16387, 32771, 65539};
__device__ const uint8_t kMLBits[53] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                                        0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};

// The tables of one wave.  An FSE entry is symbol | bits << 8 | base << 16, a Huffman entry symbol | bits << 8.
struct ZShared {
    uint16_t huf[2048];
    uint32_t ll[512], of[256], ml[512];
    uint32_t wt[64];              // the FSE table of the Huffman weights
    uint8_t w[256];               // Huffman weights
    int16_t freq[64];
    uint16_t next[64];
    uint32_t seq_ll[64], seq_ml[64], seq_dist[64];
};

// Orders the LDS traffic of a one-wave workgroup (as in omr_tiffread.hip): no instruction, the
// compiler keeps the accesses in program order and the LDS serves a wave's accesses in issue order.
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ uint32_t bcast0(uint32_t v) { return (uint32_t)__builtin_amdgcn_readlane((int)v, 0); }
__device__ __forceinline__ uint32_t high_bit(uint32_t v) { return 31u - (uint32_t)__clz((int)v); }   // v != 0

// n times the byte b at dst by the whole wave (wave-uniform arguments); no byte outside dst[0, n).
__device__ __forceinline__ void wave_fill(uint8_t* dst, uint32_t b, uint32_t n, int lane) {
    const uint32_t head = min(n, (uint32_t)(0u - (uint32_t)reinterpret_cast<uintptr_t>(dst)) & 3u);
    if ((uint32_t)lane < head) dst[lane] = (uint8_t)b;
    const uint32_t body = (n - head) >> 2, tail = (n - head) & 3u;
    uint32_t* dw = reinterpret_cast<uint32_t*>(dst + head);
    for (uint32_t i = (uint32_t)lane; i < body; i += 64u) dw[i] = b * 0x01010101u;
    const uint32_t t0 = head + 4u * body;
    if ((uint32_t)lane < tail) dst[t0 + lane] = (uint8_t)b;
}

// Backward bits of one lane: the stream's bits [0, pos) are unread, a read takes the n below pos,
// through a 64-bit window over bits [wbase, wbase + 64).  Bits below the stream's first read as zero
// and leave pos negative; a byte is loaded only at an index inside [0, len).
struct DBack {
    const uint8_t* s;
    int32_t len, pos, wbase;
    uint64_t win;
    __device__ __forceinline__ void reload() {
        wbase = (pos - 57) & ~7;                           // pos - wbase in [57, 64], also below zero
        const int32_t b0 = wbase >> 3;
        uint64_t v = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int32_t i = b0 + k;
            if (i >= 0 && i < len) v |= (uint64_t)s[i] << (8 * k);
        }
        win = v;
    }
    __device__ __forceinline__ bool init(const uint8_t* p, uint32_t n) {   // n <= 128 KiB
        if (n == 0u) return false;
        const uint32_t last = p[n - 1u];
        if (last == 0u) return false;
        s = p;
        len = (int32_t)n;
        pos = (int32_t)(n - 1u) * 8 + (int32_t)high_bit(last);
        reload();
        return true;
    }
    __device__ __forceinline__ uint32_t take(uint32_t n) {   // n <= 32
        if (n == 0u) return 0u;
        if (pos - (int32_t)n < wbase) reload();
        pos -= (int32_t)n;
        return (uint32_t)(win >> (pos - wbase)) & (uint32_t)((1ull << n) - 1ull);
    }
};

// n <= 16 forward bits at bit position `bit` of s[0, len), LSB first; bits behind the end read as zero and set `over`.
__device__ __forceinline__ uint32_t fwd_take(const uint8_t* s, uint32_t len, uint32_t& bit, uint32_t n, bool& over) {
    const uint32_t b = bit >> 3;
    uint32_t v = 0;
#pragma unroll
    for (uint32_t k = 0; k < 3u; ++k)
        if (b + k < len) v |= (uint32_t)s[b + k] << (8u * k);
    v = (v >> (bit & 7u)) & ((1u << n) - 1u);
    bit += n;
    if (bit > len * 8u) over = true;
    return v;
}

// One lane: the decoding table of the distribution S.freq[0, n) (n <= 64) into t[0, 1 << log), log <= 9.
__device__ bool fse_build(ZShared& S, uint32_t n, uint32_t log, uint32_t* t) {
    const uint32_t size = 1u << log, mask = size - 1u;
    uint32_t high = size;
    for (uint32_t s = 0; s < n; ++s)
        if (S.freq[s] == -1) {
            t[--high & mask] = s;
            S.next[s] = 1;
        }
    const uint32_t step = (size >> 1) + (size >> 3) + 3u;
    uint32_t pos = 0;
    for (uint32_t s = 0; s < n; ++s) {
        const int32_t f = S.freq[s];
        if (f <= 0) continue;
        S.next[s] = (uint16_t)f;
        for (int32_t k = 0; k < f; ++k) {                  // the frequencies sum to size: at most size steps in all
            t[pos & mask] = s;
            do pos = (pos + step) & mask;
            while (pos >= high);
        }
    }
    if (pos != 0u) return false;
    for (uint32_t i = 0; i < size; ++i) {
        const uint32_t s = t[i] & 63u;
        const uint32_t x = S.next[s];
        S.next[s] = (uint16_t)(x + 1u);
        const uint32_t nb = log - high_bit(x | 1u);
        t[i] = s | nb << 8 | (((x << nb) - size) & 0xFFFFu) << 16;
    }
    return true;
}

// One lane: an FSE table description at s[0, len) into t; *used = its bytes.
__device__ bool fse_read(ZShared& S, const uint8_t* s, uint32_t len, uint32_t max_log, uint32_t max_sym, uint32_t* t,
                         uint32_t* used, uint32_t* log_out) {
    uint32_t bit = 0;
    bool over = false;
    const uint32_t log = fwd_take(s, len, bit, 4u, over) + 5u;
    if (over || log > max_log) return false;
    int32_t remaining = 1 << log;
    uint32_t n = 0;
    while (remaining > 0 && n < max_sym) {
        const uint32_t bits = high_bit((uint32_t)remaining + 1u) + 1u;
        uint32_t v = fwd_take(s, len, bit, bits, over);
        const uint32_t lower = (1u << (bits - 1u)) - 1u, threshold = (1u << bits) - 1u - ((uint32_t)remaining + 1u);
        if ((v & lower) < threshold) {
            --bit;
            v &= lower;
        } else if (v > lower) {
            v -= threshold;
        }
        const int32_t p = (int32_t)v - 1;
        remaining -= p < 0 ? 1 : p;
        S.freq[n++ & 63u] = (int16_t)p;
        if (p == 0) {
            uint32_t rep;
            do {
                rep = fwd_take(s, len, bit, 2u, over);
                for (uint32_t k = 0; k < rep && n < max_sym; ++k) S.freq[n++ & 63u] = 0;
            } while (rep == 3u && !over);
        }
        if (over) return false;
    }
    if (remaining != 0 || over) return false;
    *used = (bit + 7u) >> 3;
    if (*used > len) return false;
    *log_out = log;
    return fse_build(S, n, log, t);
}

// One lane: a sequence table by its mode (0 predefined, 1 RLE, 2 FSE description, 3 repeat).
// kind: 0 no table yet, 1 the predefined one is built, 2 another.
__device__ bool seq_table(ZShared& S, uint32_t mode, uint32_t* t, uint32_t& log, uint32_t& kind, const int16_t* def,
                          uint32_t ndef, uint32_t def_log, uint32_t max_log, uint32_t max_sym, const uint8_t* s, uint32_t& ip,
                          uint32_t end) {
    if (mode == 0u) {
        if (kind != 1u) {
            for (uint32_t k = 0; k < ndef; ++k) S.freq[k] = def[k];
            if (!fse_build(S, ndef, def_log, t)) return false;
        }
        log = def_log;
        kind = 1u;
        return true;
    }
    if (mode == 1u) {
        if (ip >= end) return false;
        const uint32_t sym = s[ip++];
        if (sym >= max_sym) return false;
        t[0] = sym;
        log = 0u;
        kind = 2u;
        return true;
    }
    if (mode == 2u) {
        uint32_t used = 0;
        kind = 0u;
        if (!fse_read(S, s + ip, end - ip, max_log, max_sym, t, &used, &log)) return false;
        ip += used;
        kind = 2u;
        return true;
    }
    return kind != 0u;
}

// Three packed words of per-weight counts: weight w (1 .. 11) is ten bits at 10 ((w - 1) % 3) of word (w - 1) / 3.
struct WCount {
    uint32_t q0, q1, q2, q3;
    __device__ __forceinline__ void add(uint32_t w) {
        if (!w) return;
        const uint32_t f = (w - 1u) / 3u, inc = 1u << (10u * ((w - 1u) % 3u));
        q0 += f == 0u ? inc : 0u;
        q1 += f == 1u ? inc : 0u;
        q2 += f == 2u ? inc : 0u;
        q3 += f == 3u ? inc : 0u;
    }
    __device__ __forceinline__ uint32_t get(uint32_t w) const {   // w >= 1
        const uint32_t f = (w - 1u) / 3u;
        const uint32_t v = f == 0u ? q0 : f == 1u ? q1 : f == 2u ? q2 : q3;
        return (v >> (10u * ((w - 1u) % 3u))) & 1023u;
    }
};

// The whole wave: the Huffman table from S.w[0, nw), nw <= 255 (entries at and above nw are zero).
// Returns the table's log, 0 when the weights are refused.
__device__ uint32_t huf_build(ZShared& S, uint32_t nw, int lane) {
    uint32_t w[4];
    uint32_t part = 0;
    bool bad = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        w[k] = S.w[4 * lane + k];
        bad = bad || w[k] > 11u;
        part += w[k] ? 1u << ((w[k] - 1u) & 15u) : 0u;
    }
    if (__ballot(bad)) return 0u;
    const uint32_t sum = lane_value(wave_incl_scan(part, lane), 63u);   // at most 255 * 2^10
    if (sum == 0u) return 0u;
    const uint32_t log = high_bit(sum) + 1u;
    if (log > 11u) return 0u;
    const uint32_t left = (1u << log) - sum;               // >= 1
    if (left & (left - 1u)) return 0u;
    const uint32_t lastw = high_bit(left) + 1u;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if ((uint32_t)(4 * lane + k) == nw) w[k] = lastw;
    // entries sorted by (weight, symbol), a symbol of weight w taking 1 << (w - 1) of them
    WCount own = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 4; ++k) own.add(w[k]);
    WCount incl = {wave_incl_scan(own.q0, lane), wave_incl_scan(own.q1, lane), wave_incl_scan(own.q2, lane),
                   wave_incl_scan(own.q3, lane)};
    const WCount total = {lane_value(incl.q0, 63u), lane_value(incl.q1, 63u), lane_value(incl.q2, 63u), lane_value(incl.q3, 63u)};
    WCount before = {incl.q0 - own.q0, incl.q1 - own.q1, incl.q2 - own.q2, incl.q3 - own.q3};
    uint32_t start[4], cnt[4], val[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        start[k] = cnt[k] = val[k] = 0;
        if (!w[k]) continue;
        uint32_t base = 0;
        for (uint32_t v = 1; v < w[k]; ++v) base += total.get(v) << (v - 1u);
        start[k] = base + (before.get(w[k]) << (w[k] - 1u));
        cnt[k] = 1u << (w[k] - 1u);
        val[k] = (uint32_t)(4 * lane + k) | (log + 1u - w[k]) << 8;
        before.add(w[k]);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (cnt[k] && cnt[k] <= kLaneFill)
            for (uint32_t i = 0; i < cnt[k]; ++i) S.huf[(start[k] + i) & 2047u] = (uint16_t)val[k];
        unsigned long long mm = __ballot(cnt[k] > kLaneFill);
        while (mm) {
            const uint32_t j = (uint32_t)__ffsll((long long)mm) - 1u;
            mm &= mm - 1ull;
            const uint32_t st = lane_value(start[k], j), c = lane_value(cnt[k], j), v = lane_value(val[k], j);
            for (uint32_t i = (uint32_t)lane; i < c; i += 64u) S.huf[(st + i) & 2047u] = (uint16_t)v;
        }
    }
    wave_lds_fence();
    return log;
}

// One lane: n symbols of the stream p[0, m) into out[0, n); the stream must end exactly at its first bit.
__device__ bool huf_stream(const ZShared& S, uint32_t log, const uint8_t* p, uint32_t m, uint8_t* out, uint32_t n) {
    DBack b;
    if (!b.init(p, m)) return false;
    const uint32_t mask = (1u << log) - 1u;
    uint32_t state = b.take(log);
    int32_t bits_left = b.pos + (int32_t)log;              // a symbol may only begin inside the stream
    for (uint32_t k = 0; k < n; ++k) {
        if (bits_left <= 0) return false;
        const uint32_t e = S.huf[state & 2047u], nb = e >> 8;
        out[k] = (uint8_t)e;
        state = ((state << nb) | b.take(nb)) & mask;
        bits_left -= (int32_t)nb;
    }
    return bits_left == 0;
}

__device__ __forceinline__ uint64_t rotl64(uint64_t v, int r) { return v << r | v >> (64 - r); }
constexpr uint64_t kP1 = 0x9E3779B185EBCA87ull, kP2 = 0xC2B2AE3D27D4EB4Full, kP3 = 0x165667B19E3779F9ull,
                   kP4 = 0x85EBCA77C2B2AE63ull, kP5 = 0x27D4EB2F165667C5ull;
__device__ __forceinline__ uint64_t xxh_round(uint64_t acc, uint64_t in) { return rotl64(acc + in * kP2, 31) * kP1; }
// Eight bytes at p, which all lie in the buffer: from the two or three aligned dwords that hold them.
__device__ __forceinline__ uint64_t load64(const uint8_t* p) {
    const uint32_t mis = (uint32_t)reinterpret_cast<uintptr_t>(p) & 3u;
    const uint32_t* a = reinterpret_cast<const uint32_t*>(p - mis);
    const uint64_t lo = (uint64_t)a[1] << 32 | a[0];
    if (mis == 0u) return lo;
    return lo >> (8u * mis) | (uint64_t)a[2] << (64u - 8u * mis);
}
__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src) {
    return (uint64_t)(uint32_t)__shfl((int)(uint32_t)(v >> 32), src) << 32 | (uint32_t)__shfl((int)(uint32_t)v, src);
}

// The whole wave: XXH64 (seed 0) of d[0, n); the result is lane 0's.
__device__ uint64_t wave_xxh64(const uint8_t* d, uint32_t n, int lane) {
    uint64_t v = lane == 0 ? kP1 + kP2 : lane == 1 ? kP2 : lane == 2 ? 0ull : 0ull - kP1;
    const uint32_t stripes = n >> 5;
    if (lane < 4)
        for (uint32_t i = 0; i < stripes; ++i) v = xxh_round(v, load64(d + 32u * i + 8u * (uint32_t)lane));
    const uint64_t v1 = shfl64(v, 1), v2 = shfl64(v, 2), v3 = shfl64(v, 3);
    uint64_t h = 0;
    if (lane == 0) {
        if (stripes) {
            h = rotl64(v, 1) + rotl64(v1, 7) + rotl64(v2, 12) + rotl64(v3, 18);
            h = (h ^ xxh_round(0, v)) * kP1 + kP4;
            h = (h ^ xxh_round(0, v1)) * kP1 + kP4;
            h = (h ^ xxh_round(0, v2)) * kP1 + kP4;
            h = (h ^ xxh_round(0, v3)) * kP1 + kP4;
        } else {
            h = kP5;
        }
        h += (uint64_t)n;
        uint32_t i = stripes << 5;
        for (; i + 8u <= n; i += 8u) {
            uint64_t w = 0;
            for (uint32_t k = 0; k < 8u; ++k) w |= (uint64_t)d[i + k] << (8u * k);
            h = rotl64(h ^ xxh_round(0, w), 27) * kP1 + kP4;
        }
        if (i + 4u <= n) {
            uint64_t w = 0;
            for (uint32_t k = 0; k < 4u; ++k) w |= (uint64_t)d[i + k] << (8u * k);
            h = rotl64(h ^ w * kP1, 23) * kP2 + kP3;
            i += 4u;
        }
        for (; i < n; ++i) h = rotl64(h ^ d[i] * kP5, 11) * kP1;
        h ^= h >> 33;
        h *= kP2;
        h ^= h >> 29;
        h *= kP3;
        h ^= h >> 32;
    }
    return h;
}

// What lane 0 keeps over the blocks of a frame.
struct ZState {
    uint32_t rep0 = 1, rep1 = 4, rep2 = 8;
    uint32_t ll_log = 0, of_log = 0, ml_log = 0;
    uint32_t ll_kind = 0, of_kind = 0, ml_kind = 0;
};

// The whole wave: the compressed block s[ip, end) at d + op; false: corrupt.  huf_log (wave-uniform):
// the log of the Huffman table in S.huf, 0 when there is none.
__device__ bool zstd_block(ZShared& S, ZState& Z, uint32_t& huf_log, const uint8_t* s, uint32_t ip, const uint32_t end,
                           uint8_t* d, uint32_t& op, const uint32_t exp, const uint32_t bmax, uint8_t* litbuf, int lane) {
    const uint32_t op0 = op;
    // ---- literals: lane 0 reads the header (and FSE-compressed weights into S.w)
    uint32_t ok = 0, type = 0, sf = 0, nlit = 0, lit_at = 0, csize = 0, nw = 0, direct = 0, tree_at = 0;
    if (lane == 0) {
        do {
            if (end - ip < 1u) break;
            const uint32_t b0 = s[ip];
            type = b0 & 3u;
            sf = (b0 >> 2) & 3u;
            if (type < 2u) {
                const uint32_t hdr = sf == 1u ? 2u : sf == 3u ? 3u : 1u;
                if (end - ip < hdr) break;
                nlit = sf == 1u ? (b0 >> 4) + ((uint32_t)s[ip + 1u] << 4)
                     : sf == 3u ? (b0 >> 4) + ((uint32_t)s[ip + 1u] << 4) + ((uint32_t)s[ip + 2u] << 12) : b0 >> 3;
                ip += hdr;
                const uint32_t take = type == 0u ? nlit : 1u;
                if (nlit > kZBlockMax || end - ip < take) break;
                lit_at = ip;
                ip += take;
            } else {
                const uint32_t hdr = sf < 2u ? 3u : sf == 2u ? 4u : 5u;
                if (end - ip < hdr) break;
                uint64_t v = 0;
                for (uint32_t k = 0; k < hdr; ++k) v |= (uint64_t)s[ip + k] << (8u * k);
                v >>= 4;
                const uint32_t nb = sf < 2u ? 10u : sf == 2u ? 14u : 18u;
                nlit = (uint32_t)v & ((1u << nb) - 1u);
                csize = (uint32_t)(v >> nb) & ((1u << nb) - 1u);
                ip += hdr;
                if (nlit > kZBlockMax || csize > end - ip) break;
                lit_at = ip;
                ip += csize;
                if (type == 2u) {
                    if (csize < 1u) break;
                    const uint32_t hb = s[lit_at];
                    tree_at = lit_at + 1u;
                    if (hb >= 128u) {
                        nw = hb - 127u;
                        const uint32_t bytes = (nw + 1u) / 2u;
                        if (bytes > csize - 1u) break;
                        direct = 1u;
                        lit_at += 1u + bytes;
                        csize -= 1u + bytes;
                    } else {
                        if (hb > csize - 1u) break;
                        uint32_t tu = 0, wlog = 0;
                        if (!fse_read(S, s + tree_at, hb, 6u, 13u, S.wt, &tu, &wlog)) break;
                        DBack b;
                        if (tu >= hb || !b.init(s + tree_at + tu, hb - tu)) break;
                        uint32_t s1 = b.take(wlog), s2 = b.take(wlog);
                        if (b.pos < 0) break;
                        bool fine = true;
                        for (;;) {                         // two states by turns, until the bits run out
                            if (nw > 253u) {
                                fine = false;
                                break;
                            }
                            uint32_t e = S.wt[s1 & 63u];
                            S.w[nw++] = (uint8_t)e;
                            s1 = (e >> 16) + b.take((e >> 8) & 255u);
                            if (b.pos < 0) {
                                S.w[nw++] = (uint8_t)S.wt[s2 & 63u];
                                break;
                            }
                            e = S.wt[s2 & 63u];
                            S.w[nw++] = (uint8_t)e;
                            s2 = (e >> 16) + b.take((e >> 8) & 255u);
                            if (b.pos < 0) {
                                S.w[nw++] = (uint8_t)S.wt[s1 & 63u];
                                break;
                            }
                        }
                        if (!fine || nw > 255u) break;
                        lit_at += 1u + hb;
                        csize -= 1u + hb;
                    }
                }
            }
            ok = 1u;
        } while (false);
    }
    wave_lds_fence();
    if (!bcast0(ok)) return false;
    type = bcast0(type); sf = bcast0(sf); nlit = bcast0(nlit); lit_at = bcast0(lit_at); csize = bcast0(csize);
    nw = bcast0(nw); direct = bcast0(direct); tree_at = bcast0(tree_at); ip = bcast0(ip);
    const uint8_t* lit = s + lit_at;                       // raw literals, or the byte of RLE literals
    if (type >= 2u) {
        if (type == 2u) {
            // the weights: direct ones are read by their lanes, four symbols each
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t sym = (uint32_t)(4 * lane + k);
                if (direct) {
                    uint32_t w = 0;
                    if (sym < nw) {                        // tree_at + sym / 2 < tree_at + (nw + 1) / 2: checked
                        const uint32_t b = s[tree_at + (sym >> 1)];
                        w = sym & 1u ? b & 15u : b >> 4;
                    }
                    S.w[sym] = (uint8_t)w;
                } else if (sym >= nw) {
                    S.w[sym] = 0;
                }
            }
            wave_lds_fence();
            huf_log = huf_build(S, nw, lane);
        }
        if (huf_log == 0u) return false;                   // treeless without a table, or refused weights
        // the streams, one lane each
        uint32_t c1 = 0, c2 = 0, c3 = 0, q = nlit;
        const uint32_t streams = sf == 0u ? 1u : 4u;
        if (streams == 4u) {
            if (csize < 6u) return false;
            c1 = uni((uint32_t)lit[0] | (uint32_t)lit[1] << 8);
            c2 = uni((uint32_t)lit[2] | (uint32_t)lit[3] << 8);
            c3 = uni((uint32_t)lit[4] | (uint32_t)lit[5] << 8);
            q = (nlit + 3u) / 4u;
            if (c1 + c2 + c3 > csize - 6u || 3u * q > nlit) return false;
            lit += 6;
            csize -= 6u;
        }
        bool fine = true;
        if ((uint32_t)lane < streams) {
            const uint32_t at = lane == 0 ? 0u : lane == 1 ? c1 : lane == 2 ? c1 + c2 : c1 + c2 + c3;
            const uint32_t m = streams == 1u ? csize : lane == 0 ? c1 : lane == 1 ? c2 : lane == 2 ? c3 : csize - c1 - c2 - c3;
            const uint32_t n = streams == 1u ? nlit : lane < 3 ? q : nlit - 3u * q;
            fine = huf_stream(S, huf_log, lit + at, m, litbuf + (uint32_t)lane * q, n);   // lane q + n <= nlit <= 128 KiB
        }
        if (__ballot(!fine)) return false;
        wave_global_fence();                               // the literals are read by other lanes
        lit = litbuf;
    }
    const bool rle = type == 1u;
    const uint32_t rle_byte = rle ? uni(lit[0]) : 0u;
    // ---- sequences: lane 0 reads the header and the tables
    uint32_t nseq = 0;
    DBack b;
    b.s = s; b.len = 0; b.pos = 0; b.wbase = 0; b.win = 0;
    uint32_t sl = 0, so = 0, sm = 0;
    ok = 0;
    if (lane == 0) {
        do {
            if (end - ip < 1u) break;
            nseq = s[ip++];
            if (nseq >= 128u) {
                if (nseq < 255u) {
                    if (end - ip < 1u) break;
                    nseq = ((nseq - 128u) << 8) + s[ip++];
                } else {
                    if (end - ip < 2u) break;
                    nseq = (uint32_t)s[ip] + ((uint32_t)s[ip + 1u] << 8) + 0x7F00u;
                    ip += 2u;
                }
            }
            if (nseq == 0u) {
                if (ip != end) break;
            } else {
                if (end - ip < 1u) break;
                const uint32_t modes = s[ip++];
                if (modes & 3u) break;
                if (!seq_table(S, modes >> 6, S.ll, Z.ll_log, Z.ll_kind, kLLDefault, 36u, 6u, 9u, 36u, s, ip, end) ||
                    !seq_table(S, (modes >> 4) & 3u, S.of, Z.of_log, Z.of_kind, kOFDefault, 29u, 5u, 8u, 32u, s, ip, end) ||
                    !seq_table(S, (modes >> 2) & 3u, S.ml, Z.ml_log, Z.ml_kind, kMLDefault, 53u, 6u, 9u, 53u, s, ip, end))
                    break;
                if (ip >= end || !b.init(s + ip, end - ip)) break;
                sl = b.take(Z.ll_log);
                so = b.take(Z.of_log);
                sm = b.take(Z.ml_log);
            }
            ok = 1u;
        } while (false);
    }
    wave_lds_fence();
    if (!bcast0(ok)) return false;
    nseq = bcast0(nseq);
    uint32_t lp = 0;                                       // literals used (wave-uniform, as op)
    for (uint32_t done = 0; done < nseq; done += 64u) {
        const uint32_t cnt = min(64u, nseq - done);
        // one round: lane 0 decodes cnt sequences and accepts them against the literals and the output left
        ok = 0;
        if (lane == 0) {
            uint32_t lp0 = lp, op1 = op, k = 0;
            for (; k < cnt; ++k) {
                const uint32_t el = S.ll[sl & 511u], eo = S.of[so & 255u], em = S.ml[sm & 511u];
                const uint32_t oc = eo & 31u, mc = min(em & 255u, 52u), lc = min(el & 255u, 35u);
                const uint32_t ov = (1u << oc) + b.take(oc);
                const uint32_t mlen = kMLBase[mc] + b.take(kMLBits[mc]);
                const uint32_t llen = kLLBase[lc] + b.take(kLLBits[lc]);
                if (b.pos < 0) break;
                uint32_t off;
                if (ov > 3u) {
                    off = ov - 3u;
                    Z.rep2 = Z.rep1; Z.rep1 = Z.rep0; Z.rep0 = off;
                } else {
                    const uint32_t idx = ov - 1u + (llen == 0u ? 1u : 0u);
                    if (idx == 0u) {
                        off = Z.rep0;
                    } else {
                        off = idx == 1u ? Z.rep1 : idx == 2u ? Z.rep2 : Z.rep0 - 1u;
                        if (off == 0u) break;
                        if (idx > 1u) Z.rep2 = Z.rep1;
                        Z.rep1 = Z.rep0;
                        Z.rep0 = off;
                    }
                }
                if (llen > nlit - lp0 || llen > exp - op1) break;
                lp0 += llen;
                op1 += llen;
                if (off > op1 || mlen > exp - op1) break;
                op1 += mlen;
                S.seq_ll[k] = llen;
                S.seq_ml[k] = mlen;
                S.seq_dist[k] = off;
                if (done + k + 1u < nseq) {
                    sl = (el >> 16) + b.take((el >> 8) & 255u);
                    sm = (em >> 16) + b.take((em >> 8) & 255u);
                    so = (eo >> 16) + b.take((eo >> 8) & 255u);
                    if (b.pos < 0) break;
                } else if (b.pos != 0) {
                    break;                                 // the bit stream is consumed exactly
                }
            }
            ok = k == cnt ? 1u : 0u;
        }
        wave_lds_fence();
        if (!bcast0(ok)) return false;
        // emit, as K15a: positions by scans; the literals wait for nothing
        const bool valid = (uint32_t)lane < cnt;
        const uint32_t my_lit = valid ? S.seq_ll[lane] : 0u, my_mlen = valid ? S.seq_ml[lane] : 0u;
        const uint32_t my_dist = valid ? S.seq_dist[lane] : 1u;
        wave_lds_fence();                                  // the next round overwrites the three arrays
        const uint32_t size = my_lit + my_mlen;
        const uint32_t size_scan = wave_incl_scan(size, lane), lit_scan = wave_incl_scan(my_lit, lane);
        const uint32_t pos = op + size_scan - size, my_src = lp + lit_scan - my_lit;
        const uint32_t mpos = pos + my_lit;
        const uint32_t bytes = lane_value(size_scan, 63u), lits = lane_value(lit_scan, 63u);
        if (valid && my_lit <= kLaneLit)
            for (uint32_t k = 0; k < my_lit; ++k) d[pos + k] = rle ? (uint8_t)rle_byte : lit[my_src + k];
        unsigned long long mm = __ballot(valid && my_lit > kLaneLit);
        while (mm) {
            const uint32_t j = (uint32_t)__ffsll((long long)mm) - 1u;
            mm &= mm - 1ull;
            if (rle) wave_fill(d + lane_value(pos, j), rle_byte, lane_value(my_lit, j), lane);
            else wave_copy(d + lane_value(pos, j), lit + lane_value(my_src, j), lane_value(my_lit, j), lane);
        }
        // every sequence has a match (at least three bytes).  One fence: the blocks and rounds before
        // and this round's literals are readable behind it.  A match is free when its source lies
        // below the round's first match or inside its own sequence's literals.
        wave_global_fence();
        const bool is_match = valid;
        const uint32_t first = lane_value(mpos, 0u);
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
        op += bytes;
        lp += lits;
    }
    // the literals behind the last sequence
    const uint32_t rest = nlit - lp;                       // lane 0 accepted only lp <= nlit
    if (rest > exp - op) return false;
    if (rle) wave_fill(d + op, rle_byte, rest, lane);
    else wave_copy(d + op, lit + lp, rest, lane);
    op += rest;
    return op - op0 <= bmax;
}

// The whole wave: one frame s[0, len) into d[0, exp).
__device__ bool zstd_frame(ZShared& S, const uint8_t* s, const uint32_t len, uint8_t* d, const uint32_t exp, uint8_t* litbuf,
                           int lane) {
    uint32_t ok = 0, ip = 5, bmax = 0, checksum = 0;
    if (lane == 0) {
        do {
            if (len < 6u) break;
            if (s[0] != 0x28 || s[1] != 0xB5 || s[2] != 0x2F || s[3] != 0xFD) break;
            const uint32_t fhd = s[4];
            if (fhd & 0x08u) break;
            const bool single = fhd & 0x20u;
            checksum = (fhd >> 2) & 1u;
            uint64_t window = 0;
            if (!single) {
                const uint32_t wd = s[ip++], wlog = 10u + (wd >> 3);   // ip = 5 < len
                if (wlog > 31u) break;
                window = (1ull << wlog) + ((1ull << wlog) >> 3) * (wd & 7u);
            }
            const uint32_t did = fhd & 3u, did_bytes = did == 3u ? 4u : did;
            if (len - ip < did_bytes) break;
            uint32_t dict = 0;
            for (uint32_t k = 0; k < did_bytes; ++k) dict |= s[ip++];
            if (dict) break;
            const uint32_t fcs_flag = fhd >> 6, fcs_bytes = fcs_flag == 0u ? (single ? 1u : 0u) : 1u << fcs_flag;
            if (len - ip < fcs_bytes) break;
            uint64_t fcs = 0;
            for (uint32_t k = 0; k < fcs_bytes; ++k) fcs |= (uint64_t)s[ip++] << (8u * k);
            if (fcs_bytes == 2u) fcs += 256u;
            if (fcs_bytes && fcs != (uint64_t)exp) break;
            if (single) window = fcs;
            bmax = (uint32_t)(window < (uint64_t)kZBlockMax ? window : (uint64_t)kZBlockMax);
            ok = 1u;
        } while (false);
    }
    if (!bcast0(ok)) return false;
    ip = bcast0(ip); bmax = bcast0(bmax); checksum = bcast0(checksum);
    ZState Z;
    uint32_t huf_log = 0, op = 0;
    for (;;) {
        if (len - ip < 3u) return false;
        const uint32_t bh = uni((uint32_t)s[ip] | (uint32_t)s[ip + 1u] << 8 | (uint32_t)s[ip + 2u] << 16);
        ip += 3u;
        const uint32_t type = (bh >> 1) & 3u, size = bh >> 3;
        if (type == 3u || size > bmax) return false;
        if (type == 0u) {
            if (size > len - ip || size > exp - op) return false;
            wave_copy(d + op, s + ip, size, lane);
            op += size;
            ip += size;
        } else if (type == 1u) {
            if (len - ip < 1u || size > exp - op) return false;
            wave_fill(d + op, uni(s[ip]), size, lane);
            op += size;
            ip += 1u;
        } else {
            if (size > len - ip) return false;
            if (!zstd_block(S, Z, huf_log, s, ip, ip + size, d, op, exp, bmax, litbuf, lane)) return false;
            ip += size;
        }
        if (bh & 1u) break;
    }
    if (op != exp) return false;
    if (checksum) {
        if (len - ip < 4u) return false;
        const uint32_t want = uni((uint32_t)s[ip] | (uint32_t)s[ip + 1u] << 8 | (uint32_t)s[ip + 2u] << 16 | (uint32_t)s[ip + 3u] << 24);
        ip += 4u;
        wave_global_fence();                               // the frame's output, stored by all lanes
        const uint32_t got = bcast0((uint32_t)wave_xxh64(d, exp, lane));
        if (got != want) return false;
    }
    return ip == len;
}

// K16a.  Grid-stride over the frames, one wave (a workgroup of 64 threads) per frame; lit: one
// 128 KiB literal buffer per workgroup of the grid.  The bounds argument is at the head of this file.
__global__ void __launch_bounds__(64) k_zstd_decode(const uint8_t* __restrict__ src, const uint64_t* __restrict__ offsets,
                                                    const uint32_t* __restrict__ lengths,
                                                    const uint32_t* __restrict__ expected, const uint8_t* __restrict__ raw,
                                                    int n, uint8_t* dst, const uint64_t* __restrict__ dst_offsets,
                                                    int32_t* __restrict__ status, uint8_t* lit) {
    __shared__ ZShared S;
    const int lane = (int)threadIdx.x;
    uint8_t* litbuf = lit + (size_t)blockIdx.x * kZBlockMax;
    for (int seg = (int)blockIdx.x; seg < n; seg += (int)gridDim.x) {
        const uint8_t* s = src + offsets[seg];
        const uint32_t len = uni(lengths[seg]), exp = uni(expected[seg]);
        uint8_t* d = dst + dst_offsets[seg];
        if (raw && uni(raw[seg])) {
            if (len == exp) wave_copy(d, s, exp, lane);
            if (lane == 0) status[seg] = len == exp ? OMR_OK : OMR_INTERNAL;
            continue;
        }
        const bool fine = zstd_frame(S, s, len, d, exp, litbuf, lane);
        if (lane == 0) status[seg] = fine ? OMR_OK : OMR_INTERNAL;
        wave_global_fence();                               // the next frame reuses the tables and the literal buffer
    }
}

}  // namespace

omr_status launch_zstd_decode(Ctx* ctx, const StreamTable& t, void** lit, size_t* lit_cap) {
    if (t.n <= 0) return OMR_OK;
    // 11 KiB of LDS per wave would admit 14 workgroups per CU; 8 keep the literal buffers (128 KiB
    // each) at 256 MiB for a full grid
    const int blocks = std::min(t.n, std::max(1, ctx->cu_count) * 8);
    const size_t need = (size_t)blocks * kZBlockMax;
    if (need > *lit_cap) {
        if (*lit) OMR_HIP(ctx, hipFree(*lit));
        *lit = nullptr;
        *lit_cap = 0;
        OMR_HIP(ctx, hipMalloc(lit, need));
        *lit_cap = need;
    }
    KernelTimer timer(ctx, kKindZstdDecode, true);
    omr_launch(k_zstd_decode, dim3((unsigned)blocks), dim3(64), 0u, ctx->stream, t.src, t.offsets, t.lengths, t.expected,
               t.raw, (int)t.n, t.dst, t.dst_offsets, t.status, static_cast<uint8_t*>(*lit));
    OMR_HIP(ctx, hipGetLastError());
    return OMR_OK;
}

}  // namespace omr

using namespace omr;

extern "C" omr_status omr_zstd_decode_batch_device(omr_ctx* ctx, const uint8_t* d_src, const uint64_t* d_offsets,
                                                   const uint32_t* d_lengths, const uint32_t* d_expected, int32_t n,
                                                   uint8_t* d_dst, const uint64_t* d_dst_offsets, int32_t* d_status) {
    if (!ctx) return OMR_INVALID_ARGUMENT;
    if (n < 0) return fail(ctx, OMR_INVALID_ARGUMENT, "zstd: negative stream count");
    if (n == 0) return OMR_OK;
    if (!d_src || !d_offsets || !d_lengths || !d_expected || !d_dst || !d_dst_offsets || !d_status)
        return fail(ctx, OMR_INVALID_ARGUMENT, "zstd: null argument");
    OMR_HIP(ctx, hipSetDevice(ctx->device));
    SegPipe* T = seg_pipe(ctx, SegKind::zarr);             // its literal buffer serves this entry too
    return launch_zstd_decode(ctx, {d_src, d_offsets, d_lengths, d_expected, nullptr, n, d_dst, d_dst_offsets, d_status},
                              &T->d_lit, &T->lit_cap);
}
