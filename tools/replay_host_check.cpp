// replay_host_check.cpp — a stand-alone host program over qtttgym_amd/csrc/qttt_replay_host.h (the replay ring's layout,
// the append's scan plan and the argument checks of include/qttt_replay.h), meant to be built with the host sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Iqtttgym_amd/csrc
//       tools/replay_host_check.cpp -o replay_host_check && ./replay_host_check
// No GPU and no HIP: it walks capacities and game counts up to the limits (where a 32-bit intermediate would overflow),
// replays the scan levels on the host with the plan's own offsets inside an exactly-sized allocation (an offset past the
// plan's size is a heap overflow the sanitizer reports), and calls the checks with every class of bad argument.
#include <cstdio>
#include <cstdlib>
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

static void check_layout(int64_t capacity) {
    const ReplayLayout l = replay_layout(capacity);
    const int64_t elem[6] = {8, 8, 288, 8, 4, 1};
    int64_t end = QTTT_REPLAY_HEADER_BYTES;
    for (int k = 0; k < 6; ++k) {
        EXPECT(l.off[k] % 64 == 0 && l.off[k] >= end && l.off[k] - end < 64);
        end = l.off[k] + elem[k] * capacity;
    }
    EXPECT(l.bytes >= end && l.bytes - end < 64 && l.bytes % 64 == 0);
}

// the scan of `games` lengths, level by level as the launches do it, in a buffer of exactly plan.words words
static void check_scan(int64_t games, unsigned seed) {
    const ReplayScanPlan p = replay_scan_plan(games);
    EXPECT(p.levels >= 1 && p.levels <= REPLAY_MAX_LEVELS && p.n[0] == games && p.n[p.levels] <= 1);
    EXPECT(p.off[0] == REPLAY_SCRATCH_HEAD_WORDS && p.words == p.off[p.levels] + p.n[p.levels]);
    std::vector<uint64_t> w((size_t)p.words, 0xDEADBEEFu);
    std::vector<uint8_t> length((size_t)games);
    uint64_t expect_total = 0;
    std::srand(seed);
    for (auto &x : length) {
        x = (uint8_t)(std::rand() % 14);
        expect_total += x < 10 ? x : 10;
    }
    for (int k = 0; k < p.levels; ++k) {
        EXPECT(p.n[k + 1] == (p.n[k] + QTTT_REPLAY_SCAN_BLOCK - 1) / QTTT_REPLAY_SCAN_BLOCK);
        for (int64_t b = 0; b < p.n[k + 1]; ++b) {               // one workgroup per total
            uint64_t run = 0;
            for (int64_t i = b * QTTT_REPLAY_SCAN_BLOCK; i < p.n[k] && i < (b + 1) * QTTT_REPLAY_SCAN_BLOCK; ++i) {
                const uint64_t x = k == 0 ? (length[(size_t)i] < 10 ? length[(size_t)i] : 10) : w[(size_t)(p.off[k] + i)];
                w[(size_t)(p.off[k] + i)] = run;
                run += x;
            }
            w[(size_t)(p.off[k + 1] + b)] = run;
        }
    }
    if (games > 0) EXPECT(w[(size_t)p.off[p.levels]] == expect_total);
    uint64_t run = 0;                                            // a game's rank = its prefixes added up over the levels
    for (int64_t g = 0; g < games; ++g) {
        uint64_t rank = 0;
        for (int k = 0; k < p.levels; ++k) rank += w[(size_t)(p.off[k] + (g >> (8 * k)))];
        EXPECT(rank == run);
        run += length[(size_t)g] < 10 ? length[(size_t)g] : 10;
    }
}

int main() {
    const int64_t MAX = QTTT_REPLAY_MAX_CAPACITY;
    for (int64_t c : {(int64_t)1, (int64_t)7, (int64_t)8, (int64_t)9, (int64_t)37, (int64_t)63, (int64_t)64, (int64_t)65, (int64_t)4096,
                      (int64_t)1000003, MAX - 1, MAX})
        check_layout(c);
    EXPECT(replay_capacity_bad(0) && replay_capacity_bad(-1) && replay_capacity_bad(MAX + 1) && !replay_capacity_bad(MAX));
    EXPECT(replay_games_bad(-1) && replay_games_bad((int64_t)QTTT_REPLAY_MAX_GAMES + 1) && !replay_games_bad(0));
    unsigned seed = 1;
    for (int64_t g : {0, 1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 65535, 65536, 65537, 200000}) check_scan(g, seed++);
    const ReplayScanPlan big = replay_scan_plan(QTTT_REPLAY_MAX_GAMES);
    EXPECT(big.levels == 4 && big.n[1] == 1 << 22 && big.n[2] == 1 << 14 && big.n[3] == 64 && big.n[4] == 1);
    EXPECT(big.words == 8 + (int64_t)(1 << 30) + (1 << 22) + (1 << 14) + 64 + 1);

    // the checks, with addresses that are never dereferenced
    alignas(64) static char ring[256], a[256], b[256], c[256];
    const double *pi = reinterpret_cast<const double *>(a);
    const float *v = reinterpret_cast<const float *>(b);
    const uint8_t *bytes = reinterpret_cast<const uint8_t *>(c);
    bool work = true;
    EXPECT(replay_append_check(nullptr, 0, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, work) == QTTT_ERR_SIZE && !work);
    EXPECT(replay_append_check(ring, 8, -1, a, pi, bytes, bytes, v, bytes, b, work) == QTTT_ERR_SIZE);
    EXPECT(replay_append_check(nullptr, 8, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, work) == 0 && !work);
    EXPECT(replay_append_check(ring, 8, 1, a, pi, bytes, bytes, v, bytes, nullptr, work) == QTTT_ERR_NULL);
    EXPECT(replay_append_check(ring + 1, 8, 1, a, pi, bytes, bytes, v, nullptr, b, work) == QTTT_ERR_NULL);
    EXPECT(replay_append_check(ring + 32, 8, 1, a, pi, bytes, bytes, v, bytes, b, work) == QTTT_ERR_ACTION);
    EXPECT(replay_append_check(ring, 8, 1, a + 8, pi, bytes, bytes, v, bytes, b, work) == QTTT_ERR_ACTION);
    EXPECT(replay_append_check(ring, 8, 1, a, pi, bytes, bytes, reinterpret_cast<const float *>(b + 2), bytes, b, work) == QTTT_ERR_ACTION && !work);
    EXPECT(replay_append_check(ring, 8, 1, a, pi, bytes + 1, bytes + 3, v, bytes + 5, b, work) == 0 && work);
    float *s = reinterpret_cast<float *>(a);
    double *po = reinterpret_cast<double *>(b);
    uint8_t *mo = reinterpret_cast<uint8_t *>(c);
    EXPECT(replay_sample_check(ring, 8, 1, 0x80000000u, s, po, mo, s, mo, nullptr, work) == QTTT_ERR_SIZE && !work);
    EXPECT(replay_sample_check(ring, 8, MAX + 1, 0, s, po, mo, s, mo, nullptr, work) == QTTT_ERR_SIZE);
    EXPECT(replay_sample_check(nullptr, 8, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, work) == 0 && !work);
    EXPECT(replay_sample_check(ring, 8, 1, 0, s, nullptr, mo, s, mo, nullptr, work) == QTTT_ERR_NULL);
    EXPECT(replay_sample_check(ring, 8, 1, 0, s, reinterpret_cast<double *>(b + 8), mo, s, mo, nullptr, work) == QTTT_ERR_ACTION);
    EXPECT(replay_sample_check(ring, 8, 1, 0, s, po, mo, s, mo, reinterpret_cast<int32_t *>(c + 2), work) == QTTT_ERR_ACTION);
    EXPECT(replay_sample_check(ring, 8, 1, 0x7FFFFFFFu, s, po, mo, s, mo + 1, nullptr, work) == 0 && work);
    std::printf(failures ? "replay_host_check: %d FAILED\n" : "replay_host_check: ok\n", failures);
    return failures ? 1 : 0;
}
