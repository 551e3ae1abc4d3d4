// replay_reanalyse_host_check.cpp — a stand-alone host program over the reanalysis part of
// qtttgym_amd/csrc/qttt_replay_host.h (include/qttt_replay_reanalyse.h): holder, the window's slots and start, and the
// argument checks of qttt_replay_gather and qttt_replay_update, meant to be built with the host sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Iqtttgym_amd/csrc
//       tools/replay_reanalyse_host_check.cpp -o replay_reanalyse_host_check && ./replay_reanalyse_host_check
// No GPU and no HIP.  It replays appends into a ring of sample numbers and compares holder with what the ring holds, walks
// windows into exactly-sized arrays (a slot past F is a heap overflow the sanitizer reports), goes to the limits of
// capacity and `written` (where a 32-bit or a signed intermediate would overflow), and calls the checks with every class
// of bad argument.
#include <cstdio>
#include <vector>
#include "qttt_replay_host.h"

static int failures = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);             \
            ++failures;                                                       \
        }                                                                     \
    } while (0)

// sample number w lives in slot w % capacity: after every append holder(s) is what slot s holds
static void check_holder(uint64_t capacity) {
    std::vector<uint64_t> ring((size_t)capacity, ~0ull);
    for (uint64_t written = 0; written <= 3 * capacity; ++written) {
        const uint64_t F = written < capacity ? written : capacity;
        for (uint64_t s = 0; s < F; ++s) EXPECT(replay_holder(s, written, capacity) == ring[(size_t)s]);
        ring[(size_t)(written % capacity)] = written;
    }
}

// a window of n samples into a ring that holds F: every slot once, consecutive, inside [0, F)
static void check_window(uint64_t F, int64_t start, uint64_t hash) {
    std::vector<int> seen((size_t)F, 0);
    const uint64_t s0 = replay_window_start(start, hash, F);
    EXPECT(s0 < F);
    if (start >= 0) EXPECT(s0 == (uint64_t)start % F);
    uint64_t prev = 0;
    for (uint64_t i = 0; i < F; ++i) {
        const uint64_t s = replay_window_slot(s0, i, F);
        EXPECT(s < F);
        if (s < F) ++seen[(size_t)s];
        if (i) EXPECT(s == (prev + 1) % F);
        prev = s;
    }
    for (uint64_t s = 0; s < F; ++s) EXPECT(seen[(size_t)s] == 1);
}

int main() {
    const int64_t MAX = QTTT_REPLAY_MAX_CAPACITY;
    for (uint64_t c : {1u, 2u, 7u, 37u, 64u, 65u, 300u}) check_holder(c);
    // the limits: a full ring of 2^30 slots after 2^63 samples, and `written` one past a multiple of the capacity
    EXPECT(replay_holder(0, 1, (uint64_t)MAX) == 0);
    EXPECT(replay_holder((uint64_t)MAX - 1, (uint64_t)MAX, (uint64_t)MAX) == (uint64_t)MAX - 1);
    EXPECT(replay_holder(5, (1ull << 63) + 6, (uint64_t)MAX) == (1ull << 63) + 5);
    EXPECT(replay_holder(6, (1ull << 63) + 6, (uint64_t)MAX) == (1ull << 63) + 6 - (uint64_t)MAX);
    EXPECT(replay_holder(0, ~0ull, 7) == (~0ull - 1) - (~0ull - 1) % 7);
    for (uint64_t F : {1u, 2u, 7u, 37u, 64u, 300u})
        for (int64_t start : {(int64_t)-1, (int64_t)0, (int64_t)1, (int64_t)36, (int64_t)299, (int64_t)300, INT64_MAX})
            for (uint64_t hash : {0ull, 1ull, 0x8000000000000000ull, ~0ull}) check_window(F, start, hash);
    EXPECT(replay_window_start(-1, ~0ull, (uint64_t)MAX) == (uint64_t)MAX - 1);      // mulhi stays below F
    EXPECT(replay_window_start(-1, 0x8000000000000000ull, 10) == 5);
    EXPECT(replay_window_slot((uint64_t)MAX - 1, (uint64_t)MAX - 1, (uint64_t)MAX) == (uint64_t)MAX - 2);

    // the checks, with addresses that are never dereferenced
    alignas(64) static char ring[256], a[256], b[256], c[256], d[256];
    int32_t *slot = reinterpret_cast<int32_t *>(b);
    int64_t *number = reinterpret_cast<int64_t *>(c);
    float *v = reinterpret_cast<float *>(d);
    bool work = true;
    EXPECT(replay_gather_check(nullptr, 0, 1, 0, nullptr, nullptr, nullptr, nullptr, work) == QTTT_ERR_SIZE && !work);
    EXPECT(replay_gather_check(ring, 8, -1, 0, a, slot, number, v, work) == QTTT_ERR_SIZE);
    EXPECT(replay_gather_check(ring, 8, MAX + 1, 0, a, slot, number, v, work) == QTTT_ERR_SIZE);
    EXPECT(replay_gather_check(ring, 8, 1, 0x80000000u, a, slot, number, v, work) == QTTT_ERR_SIZE);
    EXPECT(replay_gather_check(nullptr, 8, 0, 0, nullptr, nullptr, nullptr, nullptr, work) == 0 && !work);
    EXPECT(replay_gather_check(nullptr, 8, 1, 0, a, slot, number, v, work) == QTTT_ERR_NULL);
    EXPECT(replay_gather_check(ring + 1, 8, 1, 0, nullptr, slot, number, v, work) == QTTT_ERR_NULL);
    EXPECT(replay_gather_check(ring, 8, 1, 0, a, nullptr, number, v, work) == QTTT_ERR_NULL);
    EXPECT(replay_gather_check(ring, 8, 1, 0, a, slot, nullptr, v, work) == QTTT_ERR_NULL);
    EXPECT(replay_gather_check(ring + 32, 8, 1, 0, a, slot, number, v, work) == QTTT_ERR_ACTION);
    EXPECT(replay_gather_check(ring, 8, 1, 0, a + 8, slot, number, v, work) == QTTT_ERR_ACTION);
    EXPECT(replay_gather_check(ring, 8, 1, 0, a, reinterpret_cast<int32_t *>(b + 2), number, v, work) == QTTT_ERR_ACTION);
    EXPECT(replay_gather_check(ring, 8, 1, 0, a, slot, reinterpret_cast<int64_t *>(c + 4), v, work) == QTTT_ERR_ACTION);
    EXPECT(replay_gather_check(ring, 8, 1, 0, a, slot, number, reinterpret_cast<float *>(d + 2), work) == QTTT_ERR_ACTION && !work);
    EXPECT(replay_gather_check(ring, 8, 1, 0x7FFFFFFFu, a, slot, number, nullptr, work) == 0 && work);
    EXPECT(replay_gather_check(ring, MAX, MAX, 0, a + 16, slot + 1, number + 1, v + 1, work) == 0 && work);

    const double *pi = reinterpret_cast<const double *>(a);
    EXPECT(replay_update_check(nullptr, 0, 1, nullptr, nullptr, nullptr, nullptr, work) == QTTT_ERR_SIZE && !work);
    EXPECT(replay_update_check(ring, 8, -1, slot, number, pi, v, work) == QTTT_ERR_SIZE);
    EXPECT(replay_update_check(ring, 8, MAX + 1, slot, number, pi, v, work) == QTTT_ERR_SIZE);
    EXPECT(replay_update_check(nullptr, 8, 0, nullptr, nullptr, nullptr, nullptr, work) == 0 && !work);
    EXPECT(replay_update_check(nullptr, 8, 1, slot, number, pi, v, work) == QTTT_ERR_NULL);
    EXPECT(replay_update_check(ring + 1, 8, 1, nullptr, number, pi, v, work) == QTTT_ERR_NULL);
    EXPECT(replay_update_check(ring, 8, 1, slot, nullptr, pi, v, work) == QTTT_ERR_NULL);
    EXPECT(replay_update_check(ring, 8, 1, slot, number, nullptr, nullptr, work) == QTTT_ERR_NULL);
    EXPECT(replay_update_check(ring + 32, 8, 1, slot, number, pi, v, work) == QTTT_ERR_ACTION);
    EXPECT(replay_update_check(ring, 8, 1, reinterpret_cast<int32_t *>(b + 1), number, pi, v, work) == QTTT_ERR_ACTION);
    EXPECT(replay_update_check(ring, 8, 1, slot, reinterpret_cast<int64_t *>(c + 4), pi, v, work) == QTTT_ERR_ACTION);
    EXPECT(replay_update_check(ring, 8, 1, slot, number, reinterpret_cast<const double *>(a + 4), v, work) == QTTT_ERR_ACTION);
    EXPECT(replay_update_check(ring, 8, 1, slot, number, pi, reinterpret_cast<float *>(d + 2), work) == QTTT_ERR_ACTION && !work);
    EXPECT(replay_update_check(ring, 8, 1, slot, number, pi, nullptr, work) == 0 && work);
    EXPECT(replay_update_check(ring, 8, 1, slot, number, nullptr, v, work) == 0 && work);
    std::printf(failures ? "replay_reanalyse_host_check: %d FAILED\n" : "replay_reanalyse_host_check: ok\n", failures);
    return failures ? 1 : 0;
}
