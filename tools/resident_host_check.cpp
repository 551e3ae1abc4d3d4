// resident_host_check.cpp — a stand-alone host program over qtttgym_amd/csrc/qttt_tree_resident_host.h (the resident search's
// tile, round plan and argument check), meant to be built with the host sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Iqtttgym_amd/csrc
//       tools/resident_host_check.cpp -o resident_host_check && ./resident_host_check
// No GPU and no HIP: it checks the tile for every K in both precisions, the plan at hand-computed points and — written into
// exactly-sized allocations, so that a round written past `cap` is an error the sanitizer sees — for every K <= 64 and every
// budget <= 200 against the schedule stated in words, and calls the check with every class of bad argument, in order.
#include <cstdio>
#include <limits>
#include <vector>
#include "qttt_tree_resident_host.h"

static int failures = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);             \
            ++failures;                                                       \
        }                                                                     \
    } while (0)

static void check_tile() {
    for (int K = 1; K <= QTTT_TREE_MAX_LEAVES; ++K) {
        EXPECT(resident_games_per_group(K, QTTT_NN_F32) == 64 / K && resident_games_per_group(K, QTTT_NN_BF16) == 128 / K);
        EXPECT(resident_games_per_group(K, QTTT_NN_F32) >= 1);
        EXPECT(resident_games_per_group(K, QTTT_NN_F32) * K <= 64 && resident_games_per_group(K, QTTT_NN_BF16) * K <= 128);
    }
    EXPECT(resident_games_per_group(3, QTTT_NN_F32) == 21 && resident_games_per_group(64, QTTT_NN_BF16) == 2);
    EXPECT(resident_games_per_group(0, QTTT_NN_F32) == QTTT_ERR_SIZE && resident_games_per_group(65, QTTT_NN_BF16) == QTTT_ERR_SIZE);
    EXPECT(resident_games_per_group(8, 2) == QTTT_ERR_SIZE && resident_games_per_group(8, -1) == QTTT_ERR_SIZE);
    EXPECT(resident_games_per_group(std::numeric_limits<int>::min(), 0) == QTTT_ERR_SIZE);
    EXPECT(resident_games_per_group(std::numeric_limits<int>::max(), 1) == QTTT_ERR_SIZE);
}

static void check_plan() {
    {
        std::vector<int32_t> r(4, -7);
        EXPECT(resident_plan(8, 31u, r.data(), 4) == 4 && r[0] == 8 && r[1] == 8 && r[2] == 8 && r[3] == 7);
    }
    {
        std::vector<int32_t> r(1, -7);
        EXPECT(resident_plan(8, 5u, r.data(), 1) == 1 && r[0] == 5);                  // rollouts < K: one short round
        EXPECT(resident_plan(8, 31u, r.data(), 1) == 4 && r[0] == 8);                 // the count is the launch's, one size written
    }
    EXPECT(resident_plan(8, 31u, nullptr, 0) == 4 && resident_plan(3, 0u, nullptr, 0) == 0);
    EXPECT(resident_plan(8, 5u, nullptr, 1) == QTTT_ERR_NULL && resident_plan(0, 5u, nullptr, 1) == QTTT_ERR_SIZE);
    EXPECT(resident_plan(65, 5u, nullptr, 0) == QTTT_ERR_SIZE && resident_plan(8, 5u, nullptr, -1) == QTTT_ERR_SIZE);
    EXPECT(resident_plan(8, (uint32_t)QTTT_TREE_MAX_ROLLOUTS + 1u, nullptr, 0) == QTTT_ERR_SIZE);
    EXPECT(resident_plan(1, (uint32_t)QTTT_TREE_MAX_ROLLOUTS, nullptr, 0) == QTTT_TREE_MAX_ROLLOUTS);
    EXPECT(resident_plan(8, std::numeric_limits<uint32_t>::max(), nullptr, 0) == QTTT_ERR_SIZE);
    for (int K = 1; K <= QTTT_TREE_MAX_LEAVES; ++K)
        for (uint32_t R = 0; R <= 200u; ++R) {
            const int want = (int)((R + (uint32_t)K - 1u) / (uint32_t)K);
            std::vector<int32_t> r((size_t)want, -7);                                 // exactly sized
            EXPECT(resident_plan(K, R, want ? r.data() : nullptr, want) == want);
            uint32_t sum = 0u, done = 0u;
            for (int i = 0; i < want; ++i) {
                EXPECT(r[i] == (i + 1 < want ? K : (int)(R - (uint32_t)K * (uint32_t)(want - 1))));      // rounds of K, then the rest
                EXPECT((uint32_t)r[i] == resident_round((uint32_t)K, R, done));                         // the kernel's own schedule
                sum += (uint32_t)r[i];
                done += (uint32_t)r[i];
            }
            EXPECT(sum == R);
            if (want > 1) {                                                           // a smaller cap writes the first cap sizes only
                std::vector<int32_t> first((size_t)(want - 1), -7);
                EXPECT(resident_plan(K, R, first.data(), want - 1) == want && first.back() == K);
            }
        }
}

static int check(const void *tree, int64_t games, int64_t capacity, uint32_t idx0, int leaves, uint32_t rollouts, int64_t offset,
                 double vloss, double k, const void *weights, int precision, bool *work_out = nullptr) {
    bool work = true;
    const int rc = resident_search_check(tree, games, capacity, idx0, leaves, rollouts, offset, vloss, k, weights, precision, work);
    if (work_out) *work_out = work;
    else EXPECT(!work || rc == 0);
    return rc;
}

static void check_arguments() {
    alignas(16) static unsigned char tree[32], weights[32];
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    bool work = false;
    EXPECT(check(tree, 2, 4, 0u, 2, 3u, 0, 1.0, -1.0, weights, QTTT_NN_F32, &work) == 0 && work);
    EXPECT(check(tree, 2, 4, 0u, 2, 3u, 0, 0.0, 2.0, weights, QTTT_NN_BF16, &work) == 0 && work);
    // sizes, each before any pointer is looked at
    const void *none = nullptr;
    EXPECT(check(none, -1, 4, 0u, 2, 3u, 0, 1.0, -1.0, none, 0) == QTTT_ERR_SIZE);
    EXPECT(check(none, 2, 0, 0u, 2, 3u, 0, 1.0, -1.0, none, 0) == QTTT_ERR_SIZE);
    EXPECT(check(none, 2, (int64_t)QTTT_TREE_MAX_CAPACITY + 1, 0u, 2, 3u, 0, 1.0, -1.0, none, 0) == QTTT_ERR_SIZE);
    EXPECT(check(none, 2, 4, 0u, 2, 3u, -1, 1.0, -1.0, none, 0) == QTTT_ERR_SIZE);
    EXPECT(check(none, 2, 4, 0u, 0, 3u, 0, 1.0, -1.0, none, 0) == QTTT_ERR_SIZE);
    EXPECT(check(none, 2, 4, 0u, 65, 3u, 0, 1.0, -1.0, none, 0) == QTTT_ERR_SIZE);
    EXPECT(check(none, std::numeric_limits<int64_t>::max(), 4, 0u, 2, 3u, 0, 1.0, -1.0, none, 0) == QTTT_ERR_SIZE);
    EXPECT(check(none, 2, 4, (uint32_t)QTTT_TREE_MAX_ROLLOUTS - 2u, 2, 3u, 0, 1.0, -1.0, none, 0) == QTTT_ERR_SIZE);
    EXPECT(check(none, 2, 4, std::numeric_limits<uint32_t>::max(), 2, std::numeric_limits<uint32_t>::max(), 0, 1.0, -1.0, none, 0) ==
           QTTT_ERR_SIZE);                                                             // the sum does not wrap
    EXPECT(check(none, 2, 4, 0u, 2, 3u, 0, -1.0, -1.0, none, 0) == QTTT_ERR_SIZE);
    EXPECT(check(none, 2, 4, 0u, 2, 3u, 0, nan, -1.0, none, 0) == QTTT_ERR_SIZE);
    EXPECT(check(none, 2, 4, 0u, 2, 3u, 0, inf, -1.0, none, 0) == QTTT_ERR_SIZE);
    EXPECT(check(none, 2, 4, 0u, 2, 3u, 0, 1.0, nan, none, 0) == QTTT_ERR_SIZE);
    EXPECT(check(none, 2, 4, 0u, 2, 3u, 0, 1.0, inf, none, 0) == QTTT_ERR_SIZE);
    EXPECT(check(none, 2, 4, 0u, 2, 3u, 0, 1.0, -inf, none, 0) == QTTT_ERR_SIZE);
    EXPECT(check(none, 2, 4, 0u, 2, 3u, 0, 1.0, -1.0, none, 2) == QTTT_ERR_SIZE);
    EXPECT(check(none, 2, 4, 0u, 2, 3u, 0, 1.0, -1.0, none, -1) == QTTT_ERR_SIZE);
    // the draw-index bound itself is allowed
    EXPECT(check(tree, 2, 4, (uint32_t)QTTT_TREE_MAX_ROLLOUTS - 3u, 2, 3u, 0, 1.0, -1.0, weights, 0, &work) == 0 && work);
    // nothing to do
    EXPECT(check(none, 0, 4, 0u, 2, 3u, 0, 1.0, -1.0, none, 0, &work) == 0 && !work);
    EXPECT(check(none, 2, 4, 0u, 2, 0u, 0, 1.0, -1.0, none, 0, &work) == 0 && !work);
    EXPECT(check(tree + 8, 2, 4, 0u, 2, 0u, 0, 1.0, -1.0, weights + 4, 1, &work) == 0 && !work);
    // nulls before alignment
    EXPECT(check(none, 2, 4, 0u, 2, 3u, 0, 1.0, -1.0, weights, 0) == QTTT_ERR_NULL);
    EXPECT(check(tree, 2, 4, 0u, 2, 3u, 0, 1.0, -1.0, none, 0) == QTTT_ERR_NULL);
    EXPECT(check(tree + 8, 2, 4, 0u, 2, 3u, 0, 1.0, -1.0, none, 0) == QTTT_ERR_NULL);
    EXPECT(check(none, 2, 4, 0u, 2, 3u, 0, 1.0, -1.0, weights + 4, 0) == QTTT_ERR_NULL);
    EXPECT(check(tree + 8, 2, 4, 0u, 2, 3u, 0, 1.0, -1.0, weights, 0) == QTTT_ERR_ACTION);
    EXPECT(check(tree, 2, 4, 0u, 2, 3u, 0, 1.0, -1.0, weights + 8, 0) == QTTT_ERR_ACTION);
    EXPECT(check(tree, 2, 4, 0u, 2, 3u, 0, 1.0, -1.0, weights + 4, 1) == QTTT_ERR_ACTION);
}

int main() {
    check_tile();
    check_plan();
    check_arguments();
    if (failures) {
        std::printf("resident_host_check: %d FAILED\n", failures);
        return 1;
    }
    std::printf("resident_host_check: ok\n");
    return 0;
}
