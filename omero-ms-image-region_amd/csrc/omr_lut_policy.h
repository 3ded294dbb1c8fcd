// omr_lut_policy.h — which entries of the context's device LUT cache (Ctx::dev_luts) leave before
// a new LUT is admitted.  Host-only and free of HIP calls, so the policy is checked on the CPU
// (tests/test_lut_cache_policy.py); device_quant_lut (omr_render.hip) frees what it returns.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace omr {

// Byte budget of the cache: OMR_LUT_CACHE_KB at context creation, clamped to these bounds.
constexpr size_t kLutCacheMinBytes = (size_t)64 << 10;     // one 16-bit-domain LUT
constexpr size_t kLutCacheMaxBytes = (size_t)256 << 20;    // the default: 16 LUTs of 2^24 entries
inline size_t lut_cache_budget(long long kb) {
    if (kb < (long long)(kLutCacheMinBytes >> 10)) return kLutCacheMinBytes;
    if (kb > (long long)(kLutCacheMaxBytes >> 10)) return kLutCacheMaxBytes;
    return (size_t)kb << 10;
}

struct LutSlot {
    size_t bytes;      // size of the entry's LUT
    uint64_t used;     // the cache clock at its last hit or upload
};

// Victims for admitting `incoming` bytes, appended to `out` as indices into e[0..n) in the order
// they leave (least recently used first): entries go while the cache holds max_entries or more, or
// its bytes plus `incoming` pass max_bytes.  An entry with used > pin is never chosen: the plan
// being prepared took it (prepare_plan notes the clock on entry, and every hit or upload of the
// plan stamps above that), and its address already sits in the plan.  When only such entries are
// left the loop stops and the cache overshoots its caps for this plan; a later plan's miss, with a
// later pin, trims it back.
inline void lut_cache_victims(const LutSlot* e, size_t n, uint64_t pin, size_t incoming, size_t max_entries,
                              size_t max_bytes, std::vector<size_t>& out) {
    size_t count = n, bytes = 0;
    for (size_t i = 0; i < n; ++i) bytes += e[i].bytes;
    std::vector<char> gone(n, 0);
    while (count > 0 && (count >= max_entries || bytes + incoming > max_bytes)) {
        size_t lru = n;
        for (size_t i = 0; i < n; ++i)
            if (!gone[i] && e[i].used <= pin && (lru == n || e[i].used < e[lru].used)) lru = i;
        if (lru == n) break;                           // everything left belongs to this plan
        gone[lru] = 1;
        --count;
        bytes -= e[lru].bytes;
        out.push_back(lru);
    }
}

}  // namespace omr
