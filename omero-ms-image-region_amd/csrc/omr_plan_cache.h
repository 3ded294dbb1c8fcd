// omr_plan_cache.h — key and replacement policy of the context's device cache of staged render
// settings (Ctx::plan_slots; omr_render.hip plan_tables).  Host-only and free of HIP so that it
// can be checked on the CPU against a brute-force model, like omr_lut_policy.h.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace omr {

constexpr int kPlanCacheSlots = 16;       // default; env OMR_PLAN_CACHE_SLOTS = 1 .. kPlanCacheMaxSlots
constexpr int kPlanCacheMaxSlots = 64;

inline int plan_cache_slot_count(long long env) {
    return env >= 1 && env <= kPlanCacheMaxSlots ? (int)env : kPlanCacheSlots;
}

// Everything the table builders read: the staged plan bytes (the channel parameters, the codomain,
// the OMR_SEM_* flags and the byte-LUT addresses are inside them), the pixel type (K1 decodes int8
// table indices, the host thresholds depend on the key space) and the launch's bucket count.
inline void plan_cache_key(const void* plan, size_t plan_bytes, int32_t pixel_type, int32_t buckets,
                           std::vector<uint8_t>& key) {
    key.resize(plan_bytes + 8);
    std::memcpy(key.data(), &pixel_type, 4);
    std::memcpy(key.data() + 4, &buckets, 4);
    if (plan_bytes) std::memcpy(key.data() + 8, plan, plan_bytes);
}

// One slot's host-side record.  `key` empty: the slot is free.
struct PlanSlot {
    std::vector<uint8_t> key;
    uint64_t used = 0;          // cache clock of the last lookup that returned the slot
};

// The slot holding `key`, or -1.
inline int plan_cache_find(const std::vector<PlanSlot>& slots, const std::vector<uint8_t>& key) {
    for (size_t i = 0; i < slots.size(); ++i)
        if (slots[i].key.size() == key.size() && std::memcmp(slots[i].key.data(), key.data(), key.size()) == 0)
            return (int)i;
    return -1;
}

// The slot a miss refills: the first free one, else the least recently used.  A call takes one
// slot and launches its kernels before the next lookup, and the slot just taken carries the
// highest clock, so it is never the victim while another slot exists.
inline int plan_cache_victim(const std::vector<PlanSlot>& slots) {
    int v = -1;
    for (size_t i = 0; i < slots.size(); ++i) {
        if (slots[i].key.empty()) return (int)i;
        if (v < 0 || slots[i].used < slots[v].used) v = (int)i;
    }
    return v;
}

}  // namespace omr
