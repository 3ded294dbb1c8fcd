// Drives the plan cache's key and replacement policy (csrc/omr_plan_cache.h) the way
// omr_render.hip's plan_tables does, against a brute-force model: a list of keys in order of last
// use.  Seeded random request streams over a few settings, slot counts 1..64.  Prints "ok: ..." and
// exits 0, or the first disagreement and exits 1.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "omr_plan_cache.h"

using namespace omr;

int main() {
    std::mt19937_64 rng(20261019);
    long lookups = 0, hits = 0;
    for (int round = 0; round < 400; ++round) {
        const int n_slots = 1 + (int)(rng() % kPlanCacheMaxSlots);
        const int n_settings = 1 + (int)(rng() % (2 * n_slots + 2));
        std::vector<PlanSlot> slots((size_t)n_slots);
        uint64_t clock = 0;
        std::vector<std::vector<uint8_t>> model;          // least recently used first
        for (int step = 0; step < 300; ++step) {
            // a "plan": a few bytes that differ per setting, keyed with a pixel type and a bucket count
            const int s = (int)(rng() % n_settings);
            uint8_t plan[24];
            for (int i = 0; i < 24; ++i) plan[i] = (uint8_t)(s * 7 + i);
            const size_t plan_bytes = 8 + (size_t)(s % 3) * 8;   // same prefix, different length: different key
            std::vector<uint8_t> key;
            plan_cache_key(plan, plan_bytes, s % 4, s % 2 ? 1024 : 2048, key);
            int i = plan_cache_find(slots, key);
            const auto m = std::find(model.begin(), model.end(), key);
            const bool want_hit = m != model.end();
            ++lookups;
            if ((i >= 0) != want_hit) { std::printf("round %d step %d: hit %d, model %d\n", round, step, i >= 0, want_hit); return 1; }
            if (i < 0) {
                i = plan_cache_victim(slots);
                if (i < 0 || i >= n_slots) { std::printf("victim %d of %d slots\n", i, n_slots); return 1; }
                if ((int)model.size() == n_slots) {
                    // the model evicts its least recently used key: the victim slot must hold it
                    if (slots[(size_t)i].key != model.front()) { std::printf("round %d step %d: victim is not the LRU\n", round, step); return 1; }
                    model.erase(model.begin());
                } else if (!slots[(size_t)i].key.empty()) {
                    std::printf("round %d step %d: evicted with a free slot left\n", round, step);
                    return 1;
                }
                slots[(size_t)i] = PlanSlot();
                slots[(size_t)i].key = key;
            } else {
                ++hits;
                model.erase(m);
            }
            slots[(size_t)i].used = ++clock;
            model.push_back(key);
        }
    }
    if (plan_cache_slot_count(0) != kPlanCacheSlots || plan_cache_slot_count(65) != kPlanCacheSlots ||
        plan_cache_slot_count(-3) != kPlanCacheSlots || plan_cache_slot_count(1) != 1 || plan_cache_slot_count(64) != 64) {
        std::printf("slot count clamp\n");
        return 1;
    }
    std::printf("ok: %ld lookups, %ld hits\n", lookups, hits);
    return 0;
}
