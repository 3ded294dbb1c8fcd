// omr_wave.h — what one wave does with bytes, shared by the LZ4 decoder (K15a, omr_blosc.hip) and
// the Zstandard decoder (K16a, omr_zstd.hip): wave-wide copies and matches into an output buffer
// that is its own window, the fence that orders them, an inclusive scan and a register window over a
// byte stream.  Device code for one-wave workgroups (64 threads); all arguments named wave-uniform
// must be so.
#ifndef OMR_WAVE_H
#define OMR_WAVE_H
#include "omr_internal.h"

namespace omr {
namespace {

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

// Orders this wave's global stores before its later global loads of the same bytes from other
// lanes (the output buffer is the window of the matches), by the argument of K14a's fence of the
// same name (omr_inflate.hip): the workgroup is this one wave on one CU, a workgroup-scope release
// waits until the wave's stores have been performed at the CU's write-through vector L1 and the L2
// behind it, and the loads that follow go through that same L1.
__device__ __forceinline__ void wave_global_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

// The stream's bytes through a 256-byte window held in one register per lane (dword win_lo + lane
// counted from sw, the aligned dword that holds s[0]); only dwords that hold a byte of the stream
// are loaded, the others read as zero.  All members but the window register are wave-uniform.  The
// parser compares every position with the stream's length before it reads there.
struct ByteWindow {
    const uint32_t* sw;
    uint64_t end_pos;     // bytes from sw to the end of the stream
    uint32_t mis;         // bytes from sw to s[0]
    uint32_t r0, win_lo;
    bool win_valid;
    int lane;

    __device__ __forceinline__ uint32_t byte(uint32_t pos) {
        const uint32_t p = mis + pos, k = p >> 2;
        if (!win_valid || k < win_lo || k - win_lo >= 64u) {
            win_lo = k;
            const uint64_t d0 = (uint64_t)k + (uint64_t)lane;
            r0 = (d0 << 2) < end_pos ? sw[d0] : 0u;
            win_valid = true;
        }
        return (lane_value(r0, k - win_lo) >> (8u * (p & 3u))) & 255u;
    }
};

// n bytes from src to dst by the whole wave (all arguments wave-uniform): the head up to dst's
// dword boundary and the tail byte by byte, the body in dword stores whose value comes from the
// one or two aligned source dwords that hold it.  Every source dword loaded holds at least one of
// the n bytes (sh > 0: dword i + 1 begins at byte 4 i + 4 - sh < 4 body); no byte outside
// dst[0, n) is stored.
__device__ __forceinline__ void wave_copy(uint8_t* dst, const uint8_t* src, uint32_t n, int lane) {
    const uint32_t head = min(n, (uint32_t)(0u - (uint32_t)reinterpret_cast<uintptr_t>(dst)) & 3u);
    if ((uint32_t)lane < head) dst[lane] = src[lane];
    const uint32_t body = (n - head) >> 2, tail = (n - head) & 3u;
    uint32_t* dw = reinterpret_cast<uint32_t*>(dst + head);
    const uint8_t* sb = src + head;
    const uint32_t sh = (uint32_t)reinterpret_cast<uintptr_t>(sb) & 3u;
    const uint32_t* sw = reinterpret_cast<const uint32_t*>(sb - sh);
    if (sh == 0u) {
        for (uint32_t i = (uint32_t)lane; i < body; i += 64u) dw[i] = sw[i];
    } else {
        for (uint32_t i = (uint32_t)lane; i < body; i += 64u) {
            const uint32_t lo = sw[i], hi = sw[i + 1u];
            dw[i] = (uint32_t)(((uint64_t)hi << 32 | lo) >> (8u * sh));
        }
    }
    const uint32_t t0 = head + 4u * body;
    if ((uint32_t)lane < tail) dst[t0 + lane] = src[t0 + lane];
}

// A match of mlen bytes at d + mpos from `dist` back, by the whole wave (wave-uniform arguments,
// 1 <= dist <= mpos): byte k is d[mpos - dist + k mod dist], so every source byte lies in
// [mpos - dist, mpos), wholly before the match.  dist >= mlen is a plain copy; a shorter distance
// repeats its period: each lane keeps its phase k mod dist (one division, then steps of 256 mod dist).
__device__ __forceinline__ void wave_match(uint8_t* d, uint32_t mpos, uint32_t mlen, uint32_t dist, int lane) {
    uint8_t* dst = d + mpos;
    const uint8_t* src = dst - dist;
    if (dist >= mlen) {
        wave_copy(dst, src, mlen, lane);
        return;
    }
    const uint32_t head = min(mlen, (uint32_t)(0u - (uint32_t)reinterpret_cast<uintptr_t>(dst)) & 3u);
    if ((uint32_t)lane < head) dst[lane] = src[(uint32_t)lane % dist];
    const uint32_t body = (mlen - head) >> 2, tail = (mlen - head) & 3u;
    uint32_t* dw = reinterpret_cast<uint32_t*>(dst + head);
    uint32_t r = (head + 4u * (uint32_t)lane) % dist;
    const uint32_t step = 256u % dist;
    for (uint32_t i = (uint32_t)lane; i < body; i += 64u) {
        uint32_t v = 0, q = r;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            v |= (uint32_t)src[q] << (8 * b);             // q < dist
            q = q + 1u == dist ? 0u : q + 1u;
        }
        dw[i] = v;
        r += step;
        if (r >= dist) r -= dist;
    }
    const uint32_t t0 = head + 4u * body;
    if ((uint32_t)lane < tail) dst[t0 + lane] = src[(t0 + (uint32_t)lane) % dist];
}

}  // namespace
}  // namespace omr
#endif  // OMR_WAVE_H
