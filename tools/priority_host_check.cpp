// priority_host_check.cpp — a stand-alone host program over qtttgym_amd/csrc/qttt_replay_priority_host.h
// (include/qttt_replay_priority.h): the table's layout, the plan of the sum launches, the sync rule, the guard of the
// write-back, the quantiser and the descent, meant to be built with the host sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Iqtttgym_amd/csrc
//       tools/priority_host_check.cpp -o priority_host_check && ./priority_host_check
// No GPU and no HIP.  It walks the offsets up to the size limit, replays every launch's index arithmetic (lane t of
// workgroup b of a sum launch, the 64 x 4 children of a descent step) into exactly-sized arrays — an index past a level's
// end is a heap overflow the sanitizer reports — compares the descent with a brute-force running sum, and calls the checks
// with every class of bad argument.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>
#include "qttt_replay_priority_host.h"

static int failures = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);             \
            ++failures;                                                       \
        }                                                                     \
    } while (0)

static void check_layout(int64_t capacity, int levels) {
    const PriorityLayout l = priority_layout(capacity);
    EXPECT(l.levels == levels);
    int64_t at = QTTT_PRIORITY_HEADER_BYTES, n = capacity;
    for (int k = 0; k <= l.levels; ++k) {
        EXPECT(l.n[k] == n && l.off[k] == at && at % 64 == 0);
        at += replay_align64((k == 0 ? 4 : 8) * n);
        n = (n + QTTT_REPLAY_SCAN_BLOCK - 1) / QTTT_REPLAY_SCAN_BLOCK;
    }
    EXPECT(l.bytes == at && l.n[l.levels] == 1);
    for (int k = 1; k < l.levels; ++k) EXPECT(l.n[k] > 1);
}

// a table in host memory, every level an exactly-sized vector
struct HostTable {
    PriorityLayout l;
    uint64_t seen = 0, written = 0;
    uint32_t pmax = 0;
    std::vector<uint32_t> q;
    std::vector<std::vector<uint64_t>> sum;
    explicit HostTable(int64_t capacity) : l(priority_layout(capacity)), q((size_t)capacity, 0u) {
        for (int k = 1; k <= l.levels; ++k) sum.emplace_back((size_t)l.n[k], 0ull);
    }
    // the sum launches: grid n[k + 1], SCAN_BLOCK lanes, lane t of workgroup b reads child priority_child(b, t) when below n[k]
    void rebuild(bool assign) {
        const uint64_t cap = (uint64_t)l.n[0];
        for (int k = 0; k < l.levels; ++k)
            for (int64_t b = 0; b < l.n[k + 1]; ++b) {
                uint64_t all = 0;
                for (uint32_t t = 0; t < (uint32_t)QTTT_REPLAY_SCAN_BLOCK; ++t) {
                    const int64_t i = priority_child(b, t);
                    if (i >= l.n[k]) continue;
                    if (k == 0) {
                        if (assign && priority_slot_is_new((uint64_t)i, seen, written, cap)) q[(size_t)i] = priority_pmax(pmax);
                        all += q[(size_t)i];
                    } else {
                        all += sum[(size_t)k - 1][(size_t)i];
                    }
                }
                sum[(size_t)k][(size_t)b] = all;
            }
        if (assign) seen = written;
    }
    // the descent as the kernel walks it: level by level, 64 lanes x 4 children, those past the level's end count 0
    uint64_t descend(uint64_t t) const {
        uint64_t idx = 0;
        for (int lv = l.levels - 1; lv >= 0; --lv) {
            uint64_t x[QTTT_REPLAY_SCAN_BLOCK];
            for (uint32_t lane = 0; lane < 64u; ++lane)
                for (uint32_t m = 0; m < 4u; ++m) {
                    const uint64_t c = idx * QTTT_REPLAY_SCAN_BLOCK + 4u * lane + m;
                    x[4u * lane + m] = c < (uint64_t)l.n[lv] ? (lv == 0 ? (uint64_t)q[(size_t)c] : sum[(size_t)lv - 1][(size_t)c]) : 0ull;
                }
            const int64_t child = priority_first_past(x, QTTT_REPLAY_SCAN_BLOCK, t);
            const uint64_t to = idx * QTTT_REPLAY_SCAN_BLOCK + (uint64_t)child;
            idx = to < (uint64_t)l.n[lv] ? to : (uint64_t)l.n[lv] - 1u;
        }
        return idx;
    }
};

static void check_table(int64_t capacity) {
    HostTable tab(capacity);
    uint64_t rng = 0x9E3779B97F4A7C15ull + (uint64_t)capacity;
    const auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
    const uint64_t cap = (uint64_t)capacity;
    const uint64_t appends[] = {cap / 2, 1, cap, 3 * cap + 1, 0, 2};
    for (uint64_t a : appends) {
        const uint64_t seen0 = tab.seen;
        tab.written += a;
        std::vector<uint32_t> before = tab.q;
        tab.rebuild(true);
        const uint64_t F = tab.written < cap ? tab.written : cap;
        for (uint64_t s = 0; s < cap; ++s) {                     // the sync rule, slot by slot
            const bool is_new = s < F && replay_holder(s, tab.written, cap) >= seen0;
            EXPECT(tab.q[(size_t)s] == (is_new ? priority_pmax(tab.pmax) : before[(size_t)s]));
            if (s >= F) EXPECT(tab.q[(size_t)s] == 0u);
        }
        // a write-back of random entries, duplicates and stale numbers included
        std::vector<uint32_t> best((size_t)capacity, 0u);
        for (int e = 0; e < 64 && F; ++e) {
            const int32_t s = (int32_t)(next() % (cap + 2)) - 1;
            int64_t number = s >= 0 && (uint64_t)s < F ? (int64_t)replay_holder((uint64_t)s, tab.written, cap) : 0;
            if (next() % 4 == 0) number -= (int64_t)cap;         // a stale draw
            const bool pass = priority_entry_passes(s, number, tab.seen, tab.written, cap);
            EXPECT(pass == (s >= 0 && (uint64_t)s < F && number == (int64_t)replay_holder((uint64_t)s, tab.written, cap)));
            if (!pass) continue;
            const uint32_t v = priority_quantise((float)(next() % 1000) / 64.0f);
            if (v > best[(size_t)s]) best[(size_t)s] = v;
        }
        for (uint64_t s = 0; s < cap; ++s)
            if (best[(size_t)s]) {
                tab.q[(size_t)s] = best[(size_t)s];
                if (best[(size_t)s] > priority_pmax(tab.pmax)) tab.pmax = best[(size_t)s];
            }
        tab.rebuild(false);
        uint64_t total = 0;
        std::vector<uint64_t> cum((size_t)capacity);
        for (uint64_t s = 0; s < cap; ++s) cum[(size_t)s] = total += tab.q[(size_t)s];
        EXPECT(tab.sum.back()[0] == total);
        if (!total) continue;
        for (int e = 0; e < 200; ++e) {                          // the descent against the running sum
            uint64_t t = e == 0 ? 0 : e == 1 ? total - 1 : next() % total;
            if (e >= 2 && e < 40) t = cum[(size_t)(next() % cap)] - (e & 1u);   // on and just below a prefix boundary
            if (t >= total) t = total - 1;
            uint64_t want = 0;
            while (cum[(size_t)want] <= t) ++want;
            EXPECT(tab.descend(t) == want);
        }
    }
}

int main() {
    const int64_t MAX = QTTT_REPLAY_MAX_CAPACITY;
    check_layout(1, 1);
    check_layout(255, 1);
    check_layout(256, 1);
    check_layout(257, 2);
    check_layout(65536, 2);
    check_layout(65537, 3);
    check_layout((1 << 24), 3);
    check_layout((1 << 24) + 257, 4);
    check_layout(MAX, 4);
    EXPECT(priority_layout(MAX).bytes < (int64_t)5 << 30);      // 4 GiB of priorities and 1/255 of that in sums
    for (int64_t c : {1, 2, 255, 256, 257, 300, 65537, 70000}) check_table(c);

    // the quantiser
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    EXPECT(priority_quantise(0.0f) == 1u && priority_quantise(-1.0f) == 1u && priority_quantise(nan) == 1u);
    EXPECT(priority_quantise(inf) == 0xFFFFFFFFu && priority_quantise(3.4e38f) == 0xFFFFFFFFu);
    EXPECT(priority_quantise(std::ldexp(1.0f, -17)) == 1u);
    EXPECT(priority_quantise(std::ldexp(1.5f, -16)) == 2u && priority_quantise(std::ldexp(2.5f, -16)) == 2u);
    EXPECT(priority_quantise(65536.0f) == 0xFFFFFFFFu && priority_quantise(65535.0f) == 0xFFFF0000u);
    EXPECT(priority_quantise(1.0f) == (uint32_t)QTTT_PRIORITY_ONE && priority_quantise(std::numeric_limits<float>::denorm_min()) == 1u);
    EXPECT(priority_pmax(0) == (uint32_t)QTTT_PRIORITY_ONE && priority_pmax(7) == 7u);

    // the sync rule and the guard at the limits
    EXPECT(!priority_slot_is_new(0, 0, 0, 8) && priority_slot_is_new(0, 0, 1, 8) && !priority_slot_is_new(1, 0, 1, 8));
    EXPECT(priority_slot_is_new((uint64_t)MAX - 1, 5, (1ull << 63) + 6, (uint64_t)MAX));
    EXPECT(!priority_slot_is_new(3, (1ull << 63) + 6, (1ull << 63) + 6, (uint64_t)MAX));
    EXPECT(!priority_entry_passes(-1, 0, 9, 9, 8) && !priority_entry_passes(8, 8, 9, 9, 8) && priority_entry_passes(0, 8, 9, 9, 8));
    EXPECT(!priority_entry_passes(0, 8, 8, 9, 8) && !priority_entry_passes(0, 0, 9, 9, 8) && !priority_entry_passes(0, -8, 9, 9, 8));

    // the checks, with addresses that are never dereferenced
    alignas(64) static char ring[256], tab[256], a[256], b[256], c[256];
    const int32_t *slot = reinterpret_cast<const int32_t *>(a);
    const int64_t *number = reinterpret_cast<const int64_t *>(b);
    const float *pr = reinterpret_cast<const float *>(c);
    bool work = true;
    EXPECT(priority_sync_check(nullptr, nullptr, 0) == QTTT_ERR_SIZE && priority_sync_check(ring, tab, MAX + 1) == QTTT_ERR_SIZE);
    EXPECT(priority_sync_check(nullptr, tab, 8) == QTTT_ERR_NULL && priority_sync_check(ring + 1, nullptr, 8) == QTTT_ERR_NULL);
    EXPECT(priority_sync_check(ring + 32, tab, 8) == QTTT_ERR_ACTION && priority_sync_check(ring, tab + 8, 8) == QTTT_ERR_ACTION);
    EXPECT(priority_sync_check(ring, tab, MAX) == 0);
    EXPECT(priority_update_check(nullptr, nullptr, 0, 1, nullptr, nullptr, nullptr, work) == QTTT_ERR_SIZE && !work);
    EXPECT(priority_update_check(ring, tab, 8, -1, slot, number, pr, work) == QTTT_ERR_SIZE);
    EXPECT(priority_update_check(ring, tab, 8, MAX + 1, slot, number, pr, work) == QTTT_ERR_SIZE);
    EXPECT(priority_update_check(nullptr, nullptr, 8, 0, nullptr, nullptr, nullptr, work) == 0 && !work);
    EXPECT(priority_update_check(nullptr, tab, 8, 1, slot, number, pr, work) == QTTT_ERR_NULL);
    EXPECT(priority_update_check(ring + 1, nullptr, 8, 1, slot, number, pr, work) == QTTT_ERR_NULL);
    EXPECT(priority_update_check(ring + 1, tab, 8, 1, nullptr, number, pr, work) == QTTT_ERR_NULL);
    EXPECT(priority_update_check(ring, tab, 8, 1, slot, nullptr, pr, work) == QTTT_ERR_NULL);
    EXPECT(priority_update_check(ring, tab, 8, 1, slot, number, nullptr, work) == QTTT_ERR_NULL);
    EXPECT(priority_update_check(ring + 32, tab, 8, 1, slot, number, pr, work) == QTTT_ERR_ACTION);
    EXPECT(priority_update_check(ring, tab + 32, 8, 1, slot, number, pr, work) == QTTT_ERR_ACTION);
    EXPECT(priority_update_check(ring, tab, 8, 1, reinterpret_cast<const int32_t *>(a + 2), number, pr, work) == QTTT_ERR_ACTION);
    EXPECT(priority_update_check(ring, tab, 8, 1, slot, reinterpret_cast<const int64_t *>(b + 4), pr, work) == QTTT_ERR_ACTION);
    EXPECT(priority_update_check(ring, tab, 8, 1, slot, number, reinterpret_cast<const float *>(c + 2), work) == QTTT_ERR_ACTION && !work);
    EXPECT(priority_update_check(ring, tab, MAX, MAX, slot + 1, number + 1, pr + 1, work) == 0 && work);

    float *s_out = reinterpret_cast<float *>(a);
    double *pi_out = reinterpret_cast<double *>(b);
    uint8_t *u8 = reinterpret_cast<uint8_t *>(c);
    int32_t *i32 = reinterpret_cast<int32_t *>(a);
    int64_t *i64 = reinterpret_cast<int64_t *>(b);
    uint32_t *u32p = reinterpret_cast<uint32_t *>(c);
    uint64_t *u64p = reinterpret_cast<uint64_t *>(b);
    const auto sample = [&](const void *r, const void *p, int64_t cap, int64_t n, uint32_t draw, const float *so, const int64_t *num,
                            const uint32_t *q, const uint64_t *tot) {
        return priority_sample_check(r, p, cap, n, draw, so, pi_out, u8, s_out, u8, i32, num, q, tot, work);
    };
    EXPECT(sample(nullptr, nullptr, 0, 1, 0, s_out, i64, u32p, u64p) == QTTT_ERR_SIZE && !work);
    EXPECT(sample(ring, tab, 8, -1, 0, s_out, i64, u32p, u64p) == QTTT_ERR_SIZE);
    EXPECT(sample(ring, tab, 8, 1, 0x80000000u, s_out, i64, u32p, u64p) == QTTT_ERR_SIZE);
    EXPECT(sample(nullptr, nullptr, 8, 0, 0, nullptr, nullptr, nullptr, nullptr) == 0 && !work);
    EXPECT(sample(nullptr, tab, 8, 1, 0, s_out, i64, u32p, u64p) == QTTT_ERR_NULL);
    EXPECT(sample(ring + 1, nullptr, 8, 1, 0, s_out, i64, u32p, u64p) == QTTT_ERR_NULL);
    EXPECT(sample(ring + 1, tab, 8, 1, 0, nullptr, i64, u32p, u64p) == QTTT_ERR_NULL);
    EXPECT(sample(ring + 32, tab, 8, 1, 0, s_out, i64, u32p, u64p) == QTTT_ERR_ACTION);
    EXPECT(sample(ring, tab + 32, 8, 1, 0, s_out, i64, u32p, u64p) == QTTT_ERR_ACTION);
    EXPECT(sample(ring, tab, 8, 1, 0, s_out + 2, i64, u32p, u64p) == QTTT_ERR_ACTION);
    EXPECT(sample(ring, tab, 8, 1, 0, s_out, reinterpret_cast<const int64_t *>(b + 4), u32p, u64p) == QTTT_ERR_ACTION);
    EXPECT(sample(ring, tab, 8, 1, 0, s_out, i64, reinterpret_cast<const uint32_t *>(c + 2), u64p) == QTTT_ERR_ACTION);
    EXPECT(sample(ring, tab, 8, 1, 0, s_out, i64, u32p, reinterpret_cast<const uint64_t *>(b + 4)) == QTTT_ERR_ACTION && !work);
    EXPECT(sample(ring, tab, MAX, MAX, 0x7FFFFFFFu, s_out, nullptr, nullptr, nullptr) == 0 && work);
    std::printf(failures ? "priority_host_check: %d FAILED\n" : "priority_host_check: ok\n", failures);
    return failures ? 1 : 0;
}
