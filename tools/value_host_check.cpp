// value_host_check.cpp — a stand-alone host program over qtttgym_amd/csrc/qttt_selfplay_value_host.h (the argument checks
// of include/qttt_selfplay_value.h and one game's row arithmetic of qttt_selfplay_value_targets), meant to be built with
// the host sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Iqtttgym_amd/csrc
//       tools/value_host_check.cpp -o value_host_check && ./value_host_check
// No GPU and no HIP: it runs value_targets_game over every game of random batches held in exactly-sized allocations (an
// index past a row field is a heap overflow the sanitizer reports), checks the properties the header promises (rows at or
// past L, lambda = 1 and lambda = 0, exact rows, no -0.0), and calls the checks with every class of bad argument.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>
#include "qttt_selfplay_value_host.h"

static int failures = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);             \
            ++failures;                                                       \
        }                                                                     \
    } while (0)

static float sixteenth() { return (float)(std::rand() % 33 - 16) / 16.0f + 0.0f; }

struct Batch {
    int64_t games;
    std::vector<uint8_t> length, done, exact;
    std::vector<float> q, v;
};

// finished games of every length, the record's alternating outcome, exact rows late in the game holding other values
static Batch make(int64_t games, bool with_exact) {
    const size_t n = (size_t)(QTTT_SELFPLAY_ROWS * games);
    Batch b = {games, std::vector<uint8_t>((size_t)games), std::vector<uint8_t>(n, 0), std::vector<uint8_t>(n, 0),
               std::vector<float>(n), std::vector<float>(n, 0.0f)};
    for (auto &x : b.q) x = sixteenth();
    for (int64_t g = 0; g < games; ++g) {
        const int L = 1 + (int)(g % QTTT_SELFPLAY_ROWS);
        const float v0 = (float)(std::rand() % 3 - 1);
        b.length[(size_t)g] = (uint8_t)L;
        for (int t = 0; t < L; ++t) {
            const size_t i = (size_t)(t * games + g);
            const float x = (t & 1) ? -v0 : v0;
            b.v[i] = x == 0.0f ? 0.0f : x;
            if (with_exact && t >= 5 && t < L - 1 && std::rand() % 2) {
                b.exact[i] = 1;
                b.v[i] = sixteenth();
            }
        }
        b.done[(size_t)((L - 1) * games + g)] = 1;
    }
    return b;
}

static void run(Batch &b, int mode, double lambda, const std::vector<uint8_t> *rows, bool use_exact) {
    for (int64_t g = 0; g < b.games; ++g) {
        const int L = rows ? (*rows)[(size_t)g] : b.length[(size_t)g];
        value_targets_game(mode, lambda, L < QTTT_SELFPLAY_ROWS ? L : QTTT_SELFPLAY_ROWS, b.games, g, b.done.data(),
                           use_exact ? b.exact.data() : nullptr, b.q.data(), b.v.data());
    }
}

static bool same_bits(const std::vector<float> &a, const std::vector<float> &b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0;
}

static void check_arithmetic(int64_t games) {
    for (int with_exact = 0; with_exact < 2; ++with_exact) {
        const Batch b0 = make(games, with_exact != 0);
        for (int mode = QTTT_VALUE_MIX; mode <= QTTT_VALUE_TD; ++mode)
            for (double lambda : {0.0, 0.5, 0.8, 1.0}) {
                Batch b = b0;
                std::vector<uint8_t> rows((size_t)games);
                for (int64_t g = 0; g < games; ++g) {                // none, half, all of the game's rows (200: clamped to 10)
                    const int L = b.length[(size_t)g];
                    rows[(size_t)g] = (uint8_t)(g % 3 == 0 ? 0 : (g % 3 == 1 ? L / 2 : (L == QTTT_SELFPLAY_ROWS ? 200 : L)));
                }
                run(b, mode, lambda, (mode + (int)(lambda * 10)) % 2 ? &rows : nullptr, with_exact != 0);
                for (size_t i = 0; i < b.v.size(); ++i) {
                    EXPECT(!std::isnan(b.v[i]) && !(b.v[i] == 0.0f && std::signbit(b.v[i])));
                    const int64_t t = (int64_t)i / games, g = (int64_t)i % games;
                    if (t >= b.length[(size_t)g] || b.exact[i] == 1) EXPECT(std::memcmp(&b.v[i], &b0.v[i], 4) == 0);
                }
                EXPECT(same_bits(b.q, b0.q));
            }
        if (!with_exact) {                                           // the two identities, bit for bit
            Batch b = b0;
            run(b, QTTT_VALUE_TD, 1.0, nullptr, false);
            EXPECT(same_bits(b.v, b0.v));
            run(b, QTTT_VALUE_MIX, 0.0, nullptr, false);
            EXPECT(same_bits(b.v, b0.v));
            run(b, QTTT_VALUE_TD, 0.0, nullptr, false);              // the one-step target: -q of the next row, -v of a terminal one
            for (int64_t g = 0; g < games; ++g)
                for (int t = 0; t + 1 < b.length[(size_t)g]; ++t) {
                    const size_t i = (size_t)(t * games + g), j = i + (size_t)games;
                    EXPECT(b.v[i] == -(b.done[j] ? b0.v[j] : b.q[j]));
                }
        }
    }
    EXPECT(value_round(-1e-60) == 0.0f && !std::signbit(value_round(-1e-60)) && value_round(-0.0) == 0.0f &&
           !std::signbit(value_round(-0.0)) && value_round(0.3) == 0.3f);
}

static void check_arguments() {
    bool work = true;
    uint8_t *const B = reinterpret_cast<uint8_t *>(0x1000);
    float *const F = reinterpret_cast<float *>(0x2000), *const F2 = reinterpret_cast<float *>(0x2002);
    void *const T = reinterpret_cast<void *>(0x4000), *const T8 = reinterpret_cast<void *>(0x4008);
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    EXPECT(value_record_check(nullptr, -1, 4, 0, nullptr, nullptr, nullptr, work) == QTTT_ERR_SIZE && !work);
    EXPECT(value_record_check(T, 1, 0, 0, B, F, F, work) == QTTT_ERR_SIZE);
    EXPECT(value_record_check(T, 1, (int64_t)QTTT_TREE_MAX_CAPACITY + 1, 0, B, F, F, work) == QTTT_ERR_SIZE);
    EXPECT(value_record_check(T, 0, 4, QTTT_SELFPLAY_ROWS, B, F, F, work) == QTTT_ERR_SIZE);
    EXPECT(value_record_check(nullptr, 0, 4, -1, nullptr, nullptr, nullptr, work) == 0 && !work);
    EXPECT(value_record_check(nullptr, 1, 4, 0, B, F, F, work) == QTTT_ERR_NULL);
    EXPECT(value_record_check(T8, 1, 4, 0, nullptr, F, F, work) == QTTT_ERR_NULL);
    EXPECT(value_record_check(T, 1, 4, 0, B, nullptr, F2, work) == QTTT_ERR_NULL);
    EXPECT(value_record_check(T, 1, 4, 0, B, F, nullptr, work) == QTTT_ERR_NULL);
    EXPECT(value_record_check(T8, 1, 4, 0, B, F, F, work) == QTTT_ERR_ACTION);
    EXPECT(value_record_check(T, 1, 4, 0, B, F2, F, work) == QTTT_ERR_ACTION);
    EXPECT(value_record_check(T, 1, 4, 0, B, F, F2, work) == QTTT_ERR_ACTION && !work);
    for (int ply : {-5, -1, 0, 9}) EXPECT(value_record_check(T, 1, 4, ply, B, F, F, work) == 0 && work);
    for (double bad : {-0.001, 1.001, nan, inf, -inf}) EXPECT(value_targets_check(0, 0, bad, nullptr, nullptr, nullptr, nullptr, work) == QTTT_ERR_SIZE);
    EXPECT(value_targets_check(-1, 0, 0.5, B, B, F, F, work) == QTTT_ERR_SIZE);
    EXPECT(value_targets_check(1, 2, 0.5, B, B, F, F, work) == QTTT_ERR_SIZE && value_targets_check(1, -1, 0.5, B, B, F, F, work) == QTTT_ERR_SIZE);
    EXPECT(value_targets_check(0, 1, 1.0, nullptr, nullptr, nullptr, F2, work) == 0 && !work);
    EXPECT(value_targets_check(1, 1, 1.0, nullptr, B, F, F, work) == QTTT_ERR_NULL);
    EXPECT(value_targets_check(1, 1, 1.0, B, nullptr, F2, F, work) == QTTT_ERR_NULL);
    EXPECT(value_targets_check(1, 1, 1.0, B, B, nullptr, F, work) == QTTT_ERR_NULL);
    EXPECT(value_targets_check(1, 1, 1.0, B, B, F, nullptr, work) == QTTT_ERR_NULL);
    EXPECT(value_targets_check(1, 0, 0.0, B, B, F2, F, work) == QTTT_ERR_ACTION);
    EXPECT(value_targets_check(1, 0, 0.0, B, B, F, F2, work) == QTTT_ERR_ACTION && !work);
    EXPECT(value_targets_check(1, 0, 0.0, B, B, F, F, work) == 0 && work);
}

int main() {
    std::srand(2026);
    for (int64_t games : {1, 3, 64, 65, 257}) check_arithmetic(games);
    check_arguments();
    if (failures) {
        std::printf("value_host_check: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("value_host_check: ok\n");
    return 0;
}
