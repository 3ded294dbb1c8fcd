// Host check of the device LUT cache's eviction policy (csrc/omr_lut_policy.h), built and run by
// tests/test_lut_cache_policy.py.  A cache of (key, bytes, used) entries is driven the way
// prepare_plan / device_quant_lut drive Ctx::dev_luts -- note the clock when a plan starts, stamp
// every hit and upload with the next tick, ask the policy for victims on a miss -- and every
// answer is checked against a brute-force model that tracks the plan's own keys in a set of its
// own (not through the stamps):
//   * no entry the current plan has touched is chosen;
//   * the victims are the least recently used of the others, in that order, and exactly as many
//     as it takes to be under both caps (all of them when that cannot be reached);
//   * after a plan with a miss the cache is within both caps whenever the plan's own set fits,
//     and otherwise holds exactly that set (a plan of hits only leaves the cache as it was: only
//     a miss trims an overshoot);
//   * the policy returns (at most one victim per entry).
// `--old-rule` runs the same checks against the selection rule this policy replaced (evict the
// least recently used entry, whoever holds it): it must fail, on the first scenario already
// (seventeen 16 MiB LUTs in one plan against 256 MiB).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <set>
#include <vector>

#include "omr_lut_policy.h"

namespace {

struct Entry { uint32_t key; size_t bytes; uint64_t used; };
struct Chan { uint32_t key; size_t bytes; };

bool g_old_rule = false;

// the rule before the pin: least recently used first, nothing spared
void old_rule_victims(const omr::LutSlot* e, size_t n, size_t incoming, size_t max_entries, size_t max_bytes,
                      std::vector<size_t>& out) {
    size_t count = n, bytes = 0;
    for (size_t i = 0; i < n; ++i) bytes += e[i].bytes;
    std::vector<char> gone(n, 0);
    while (count > 0 && (count >= max_entries || bytes + incoming > max_bytes)) {
        size_t lru = n;
        for (size_t i = 0; i < n; ++i)
            if (!gone[i] && (lru == n || e[i].used < e[lru].used)) lru = i;
        gone[lru] = 1;
        --count;
        bytes -= e[lru].bytes;
        out.push_back(lru);
    }
}

struct Cache {
    std::vector<Entry> e;
    uint64_t clock = 0;
    size_t max_entries, max_bytes;
    size_t bytes() const { size_t b = 0; for (auto& x : e) b += x.bytes; return b; }
};

#define FAIL(...)                                 \
    do {                                          \
        std::printf("FAIL (%s): ", where);        \
        std::printf(__VA_ARGS__);                 \
        std::printf("\n");                        \
        return false;                             \
    } while (0)

// One plan through the cache; false on the first violated property.
bool run_plan(Cache& c, const std::vector<Chan>& plan, const char* where) {
    const uint64_t pin = c.clock;
    std::set<uint32_t> touched;               // the model's own record of this plan's keys
    bool missed = false;
    for (const Chan& ch : plan) {
        bool hit = false;
        for (auto& x : c.e)
            if (x.key == ch.key && x.bytes == ch.bytes) { x.used = ++c.clock; hit = true; break; }
        touched.insert(ch.key);
        if (hit) continue;
        missed = true;
        std::vector<omr::LutSlot> slots;
        for (auto& x : c.e) slots.push_back({x.bytes, x.used});
        std::vector<size_t> victims;
        if (g_old_rule) old_rule_victims(slots.data(), slots.size(), ch.bytes, c.max_entries, c.max_bytes, victims);
        else omr::lut_cache_victims(slots.data(), slots.size(), pin, ch.bytes, c.max_entries, c.max_bytes, victims);
        // the model: the others by age, and the shortest prefix that gets under both caps
        // (a key always has the same size here, so a miss means no entry carries ch.key)
        std::vector<size_t> others;
        for (size_t i = 0; i < c.e.size(); ++i)
            if (!touched.count(c.e[i].key)) others.push_back(i);
        std::sort(others.begin(), others.end(), [&](size_t a, size_t b) { return c.e[a].used < c.e[b].used; });
        size_t count = c.e.size(), bytes = c.bytes(), need = 0;
        while (need < others.size() && (count >= c.max_entries || bytes + ch.bytes > c.max_bytes)) {
            --count;
            bytes -= c.e[others[need]].bytes;
            ++need;
        }
        if (victims.size() > c.e.size()) FAIL("%zu victims from %zu entries", victims.size(), c.e.size());
        std::set<size_t> seen;
        for (size_t v : victims) {
            if (v >= c.e.size() || !seen.insert(v).second) FAIL("victim index %zu out of range or repeated", v);
            if (touched.count(c.e[v].key))
                FAIL("evicted key %u (%zu bytes), which this plan already holds", c.e[v].key, c.e[v].bytes);
        }
        if (victims.size() != need) FAIL("%zu victims, the model needs %zu", victims.size(), need);
        for (size_t k = 0; k < need; ++k)
            if (victims[k] != others[k]) FAIL("victim %zu is entry %zu, least recently used is %zu", k, victims[k], others[k]);
        std::vector<Entry> keep;
        for (size_t i = 0; i < c.e.size(); ++i)
            if (!seen.count(i)) keep.push_back(c.e[i]);
        c.e.swap(keep);
        c.e.push_back({ch.key, ch.bytes, ++c.clock});
    }
    // every key of the plan is resident when the plan is complete
    for (const Chan& ch : plan) {
        bool found = false;
        for (auto& x : c.e) found |= x.key == ch.key && x.bytes == ch.bytes;
        if (!found) FAIL("key %u of the finished plan is not resident", ch.key);
    }
    if (missed) {
        size_t pinned_n = 0, pinned_b = 0;
        for (auto& x : c.e)
            if (x.used > pin) { ++pinned_n; pinned_b += x.bytes; }
        const bool fits = pinned_n <= c.max_entries && pinned_b <= c.max_bytes;
        const bool within = c.e.size() <= c.max_entries && c.bytes() <= c.max_bytes;
        if (fits && !within)
            FAIL("plan's set fits (%zu entries, %zu bytes) but the cache holds %zu entries, %zu bytes", pinned_n,
                 pinned_b, c.e.size(), c.bytes());
        if (!fits && pinned_n != c.e.size())
            FAIL("plan's set overshoots, yet %zu other entries stayed", c.e.size() - pinned_n);
    }
    return true;
}

struct Rng {                                   // splitmix64: the same sequences on every host
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    size_t below(size_t n) { return (size_t)(next() % n); }
};

}  // namespace

int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i) g_old_rule |= std::strcmp(argv[i], "--old-rule") == 0;
    // budget clamp (OMR_LUT_CACHE_KB)
    if (!g_old_rule) {
        if (omr::lut_cache_budget(0) != (size_t)64 << 10 || omr::lut_cache_budget(-5) != (size_t)64 << 10 ||
            omr::lut_cache_budget(64) != (size_t)64 << 10 || omr::lut_cache_budget(128) != (size_t)128 << 10 ||
            omr::lut_cache_budget(262144) != (size_t)256 << 20 || omr::lut_cache_budget(1ll << 40) != (size_t)256 << 20) {
            std::printf("FAIL (budget clamp)\n");
            return 1;
        }
    }
    {   // seventeen wide-domain LUTs in one plan against the default caps, after a plan that fills the cache
        Cache c;
        c.max_entries = 64;
        c.max_bytes = (size_t)256 << 20;
        std::vector<Chan> warm, plan;
        for (uint32_t k = 0; k < 10; ++k) warm.push_back({100 + k, (size_t)16 << 20});
        for (uint32_t k = 0; k < 17; ++k) plan.push_back({k, ((size_t)16 << 20) - k});
        if (!run_plan(c, warm, "warm-up plan") || !run_plan(c, plan, "17 x 16 MiB in one plan")) return 1;
        if (c.e.size() != 17) { std::printf("FAIL: 17-LUT plan left %zu entries\n", c.e.size()); return 1; }
        std::vector<Chan> small = {{500, 65536}};           // the next plan's miss trims the overshoot
        if (!run_plan(c, small, "trim after overshoot")) return 1;
        if (c.bytes() > c.max_bytes) { std::printf("FAIL: overshoot not trimmed\n"); return 1; }
    }
    const size_t caps_n[] = {1, 2, 4, 8, 33, 64};
    const size_t caps_b[] = {(size_t)64 << 10, (size_t)128 << 10, (size_t)256 << 10, (size_t)1 << 20, (size_t)256 << 20};
    const size_t sizes[] = {65536, 65536, 65536, 100000, (size_t)1 << 20, (size_t)16 << 20, 1, 300};
    Rng rng{20261019};
    long plans = 0;
    for (int seq = 0; seq < 3000; ++seq) {
        Cache c;
        c.max_entries = caps_n[rng.below(6)];
        c.max_bytes = caps_b[rng.below(5)];
        const size_t universe = 2 + rng.below(80);
        std::vector<size_t> key_bytes(universe);
        const bool uniform = rng.below(3) == 0;            // all 64 KiB: the 16-bit-domain case
        for (auto& b : key_bytes) b = uniform ? 65536 : sizes[rng.below(8)];
        const int n_plans = 1 + (int)rng.below(40);
        char where[96];
        for (int p = 0; p < n_plans; ++p) {
            std::vector<Chan> plan(1 + rng.below(32));
            const size_t local = 1 + rng.below(universe);   // small: many repeats inside the plan
            for (auto& ch : plan) {
                ch.key = (uint32_t)rng.below(local);
                ch.bytes = key_bytes[ch.key];
            }
            std::snprintf(where, sizeof(where), "sequence %d plan %d, caps %zu entries / %zu bytes", seq, p,
                          c.max_entries, c.max_bytes);
            if (!run_plan(c, plan, where)) return 1;
            ++plans;
        }
    }
    std::printf("ok: %ld plans\n", plans);
    return 0;
}
