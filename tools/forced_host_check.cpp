// forced_host_check.cpp — a stand-alone host program over qtttgym_amd/csrc/qttt_tree_forced_host.h (one action's arithmetic:
// the forced predicate, min(N, F), the pruned visit count; the factor's and the root entry's checks) and
// qttt_selfplay_record_host.h (the one check of the eight record entries and the one of the three leaf-parallel selects, which
// the forced select and the pruned records go through with every other), meant to be built with the host sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Iqtttgym_amd/csrc
//       tools/forced_host_check.cpp -o forced_host_check && ./forced_host_check
// No GPU and no HIP: it checks the predicate and F at hand-computed points, min(N, F) against the definition by a plain
// search, the bisection of the pruned visits against a look at every d on random roots held in exactly-sized allocations,
// the properties the header promises of N', and calls the checks with every class of bad argument: the forced select and the
// pruned records, and the plain, sampled and Gumbel records in both forms and the plain and Gumbel selects besides.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>
#include "qttt_selfplay_record_host.h"

static int failures = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);             \
            ++failures;                                                       \
        }                                                                     \
    } while (0)

static double unit() { return (double)(std::rand() % 10001) / 10000.0; }

// the smallest F with F * F >= t by the definition, capped
static uint32_t floor_by_search(double t, uint32_t cap) {
    for (uint32_t F = 0; F < cap; ++F)
        if ((double)F * (double)F >= t) return F;
    return cap;
}

// N' by a look at every d, as tests/forced_model.py finds it
static uint32_t pruned_by_scan(double W, uint32_t N, double P, double k, uint32_t S, double sq, double c_puct, double best) {
    if (N == 0u) return 0u;
    const uint32_t m = floor_by_search(forced_threshold(k, P, S), N);
    const double Q = W / (double)N;
    uint32_t d = 0u;
    for (uint32_t x = m; x >= 1u; --x)
        if (forced_lhs(Q, P, sq, N, x, c_puct) < best) { d = x; break; }
    const uint32_t left = N - d;
    return (d > 0u && left <= 1u) ? 0u : left;
}

static void check_points() {
    EXPECT(!forced_is(4u, 2.0, 0.5, 16u) && forced_is(3u, 2.0, 0.5, 16u) && !forced_is(0u, 2.0, 0.5, 16u));      // n * n == k P S
    EXPECT(forced_floor(forced_threshold(2.0, 0.5, 16u), 100u) == 4u);
    EXPECT(forced_is(2u, 2.0, 0.25, 10u) && !forced_is(3u, 2.0, 0.25, 10u) && forced_floor(forced_threshold(2.0, 0.25, 10u), 100u) == 3u);
    EXPECT(!forced_is(1u, 0.0, 1.0, 100u) && forced_floor(forced_threshold(0.0, 1.0, 100u), 100u) == 0u);
    EXPECT(!forced_is(4096u, 2.0, 1.0, 1u << 23) && forced_is(4095u, 2.0, 1.0, 1u << 23));
    EXPECT(forced_floor(forced_threshold(2.0, 1.0, 1u << 23), 1u << 24) == 4096u && forced_floor(16777216.0, 100u) == 100u);
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    EXPECT(forced_floor(nan, 7u) == 0u && forced_floor(inf, 7u) == 7u && forced_floor(-1.0, 7u) == 0u && forced_floor(1e300, 7u) == 7u);
    EXPECT(forced_floor(1e-300, 7u) == 1u && forced_floor(1.0, 0u) == 0u);
    for (int i = 0; i < 20000; ++i) {
        const uint32_t cap = (uint32_t)(std::rand() % 300);
        const double t = i % 3 == 0 ? (double)(std::rand() % 90000) : unit() * (double)(std::rand() % 90000);
        EXPECT(forced_floor(t, cap) == floor_by_search(t, cap));
    }
    for (uint32_t F = 16777000u; F < 16777216u; ++F) {           // the largest counts: the squares are still exact
        const double t = (double)F * (double)F;
        EXPECT(forced_floor(t, 1u << 24) == F && forced_floor(t + 1.0, 1u << 24) == F + 1u && forced_floor(t, F - 1u) == F - 1u);
    }
}

static void check_roots() {
    for (int root = 0; root < 4000; ++root) {
        const int legal = 1 + std::rand() % 36;
        std::vector<uint32_t> N((size_t)legal), Np((size_t)legal);
        std::vector<double> W((size_t)legal), P((size_t)legal);
        uint32_t S = 0u, star = 0u;
        double psum = 0.0;
        for (int a = 0; a < legal; ++a) {
            N[(size_t)a] = std::rand() % 4 == 0 ? 0u : (uint32_t)(std::rand() % (root % 7 == 0 ? 900 : 12));
            W[(size_t)a] = (unit() * 2.0 - 1.0) * (double)N[(size_t)a];
            P[(size_t)a] = unit() + 1e-4;
            psum += P[(size_t)a];
            S += N[(size_t)a];
        }
        for (int a = 0; a < legal; ++a) {
            P[(size_t)a] /= psum;
            if (N[(size_t)a] > N[star]) star = (uint32_t)a;                              // ties to the lowest action
        }
        const double k = (double)(root % 5), c_puct = root % 11 == 0 ? -1.0 : 0.5 + unit() * 2.0;
        const double sq = std::sqrt((double)(S + (uint32_t)(root % 3)));                 // Ntot is S, or a little more
        const double qs = N[star] ? W[star] / (double)N[star] : 0.0;
        const double best = qs + c_puct * (P[star] * sq / (double)(1u + N[star]));
        uint32_t total = 0u;
        for (int a = 0; a < legal; ++a) {
            const size_t i = (size_t)a;
            Np[i] = (uint32_t)a == star ? N[i] : forced_pruned_visits(W[i], N[i], P[i], k, S, sq, c_puct, best);
            if ((uint32_t)a != star) EXPECT(Np[i] == pruned_by_scan(W[i], N[i], P[i], k, S, sq, c_puct, best));
            EXPECT(Np[i] <= N[i] && (Np[i] == N[i] || Np[i] != 1u));                     // no single visit is left by a subtraction
            EXPECT(k > 0.0 || Np[i] == N[i]);                                            // k = 0 prunes nothing
            EXPECT(N[i] - Np[i] <= forced_floor(forced_threshold(k, P[i], S), N[i]) + 1u);
            total += Np[i];
        }
        EXPECT(total >= N[star]);
    }
}

// addresses that are only ever compared and masked: a tree and an array, and what is 8, 4 and 2 bytes past them
static void *const T = reinterpret_cast<void *>(0x4000), *const T8 = reinterpret_cast<void *>(0x4008);
static void *const A = reinterpret_cast<void *>(0x8000), *const A8 = reinterpret_cast<void *>(0x8008);
static void *const A4 = reinterpret_cast<void *>(0x8004), *const A2 = reinterpret_cast<void *>(0x8002);
static const RecordArgs RECORD_OK = {T, A, A, A, A, A, A, A, A, A};

static void check_arguments() {
    bool work = true;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    auto forced_select_check = [](const void *tree, int64_t games, int64_t capacity, uint32_t rollout_idx0, int leaves,
                                  int64_t board_offset, double virtual_loss, const void *paths, const void *leaf_state,
                                  double forced_k, bool &w) {
        return select_batch_check(SELECT_FORCED, tree, games, capacity, rollout_idx0, leaves, board_offset, virtual_loss, paths,
                                  leaf_state, {forced_k}, w);
    };
    for (double bad : {-0.001, nan, inf, -inf}) {
        EXPECT(forced_k_bad(bad));
        EXPECT(forced_select_check(T, 1, 4, 0u, 2, 0, 1.0, A, A, bad, work) == QTTT_ERR_SIZE && !work);
        EXPECT(forced_select_check(nullptr, 0, 4, 0u, 2, 0, 1.0, nullptr, nullptr, bad, work) == QTTT_ERR_SIZE);
        EXPECT(forced_root_check(T, 1, 4, bad, 1.0, nullptr, work) == QTTT_ERR_SIZE);
    }
    for (double good : {0.0, 2.0, 1e300}) EXPECT(!forced_k_bad(good));
    // the select: the sizes of qttt_tree_select_batch, then nulls, then alignment
    EXPECT(forced_select_check(T, -1, 4, 0u, 2, 0, 1.0, A, A, 2.0, work) == QTTT_ERR_SIZE);
    EXPECT(forced_select_check(T, 1, 0, 0u, 2, 0, 1.0, A, A, 2.0, work) == QTTT_ERR_SIZE);
    EXPECT(forced_select_check(T, 1, (int64_t)QTTT_TREE_MAX_CAPACITY + 1, 0u, 2, 0, 1.0, A, A, 2.0, work) == QTTT_ERR_SIZE);
    EXPECT(forced_select_check(T, 1, 4, 0u, 0, 0, 1.0, A, A, 2.0, work) == QTTT_ERR_SIZE);
    EXPECT(forced_select_check(T, 1, 4, 0u, QTTT_TREE_MAX_LEAVES + 1, 0, 1.0, A, A, 2.0, work) == QTTT_ERR_SIZE);
    EXPECT(forced_select_check(T, 1, 4, (uint32_t)QTTT_TREE_MAX_ROLLOUTS - 1u, 2, 0, 1.0, A, A, 2.0, work) == QTTT_ERR_SIZE);
    EXPECT(forced_select_check(T, 1, 4, 0u, 2, -1, 1.0, A, A, 2.0, work) == QTTT_ERR_SIZE);
    EXPECT(forced_select_check(T, 1, 4, 0u, 2, 0, -1.0, A, A, 2.0, work) == QTTT_ERR_SIZE);
    EXPECT(forced_select_check(T, 1, 4, 0u, 2, 0, nan, A, A, 2.0, work) == QTTT_ERR_SIZE);
    EXPECT(forced_select_check(nullptr, 0, 4, 0u, 2, 0, 1.0, nullptr, nullptr, 2.0, work) == 0 && !work);
    EXPECT(forced_select_check(nullptr, 1, 4, 0u, 2, 0, 1.0, A8, A, 2.0, work) == QTTT_ERR_NULL);
    EXPECT(forced_select_check(T8, 1, 4, 0u, 2, 0, 1.0, nullptr, A, 2.0, work) == QTTT_ERR_NULL);
    EXPECT(forced_select_check(T, 1, 4, 0u, 2, 0, 1.0, A, nullptr, 2.0, work) == QTTT_ERR_NULL);
    EXPECT(forced_select_check(T8, 1, 4, 0u, 2, 0, 1.0, A, A, 2.0, work) == QTTT_ERR_ACTION);
    EXPECT(forced_select_check(T, 1, 4, 0u, 2, 0, 1.0, A8, A, 2.0, work) == QTTT_ERR_ACTION && !work);
    EXPECT(forced_select_check(T, 1, 4, 0u, 2, 0, 1.0, A, A8, 0.0, work) == 0 && work);
    // the root
    EXPECT(forced_root_check(T, -1, 4, 2.0, 1.0, nullptr, work) == QTTT_ERR_SIZE && !work);
    EXPECT(forced_root_check(T, 1, 4, 2.0, nan, nullptr, work) == QTTT_ERR_SIZE && forced_root_check(T, 1, 4, 2.0, inf, nullptr, work) == QTTT_ERR_SIZE);
    EXPECT(forced_root_check(nullptr, 0, 4, 2.0, 1.0, nullptr, work) == 0 && !work);
    EXPECT(forced_root_check(nullptr, 1, 4, 2.0, 1.0, nullptr, work) == QTTT_ERR_NULL);
    EXPECT(forced_root_check(T8, 1, 4, 2.0, 1.0, nullptr, work) == QTTT_ERR_ACTION);
    EXPECT(forced_root_check(T, 1, 4, 2.0, 1.0, static_cast<const int32_t *>(A2), work) == QTTT_ERR_ACTION);
    EXPECT(forced_root_check(T, 1, 4, 2.0, -1.0, static_cast<const int32_t *>(A4), work) == 0 && work);
    // the records
    const RecordArgs &ok = RECORD_OK;
    auto rec = [&](const RecordArgs &p, int64_t games = 1, bool stream = false, int ply = 0, uint32_t draw = 0u,
                   uint32_t n_rollouts = 8u, double alpha = 1.0, double v1 = 1.0, double v2 = -1.0, int64_t off = 0,
                   double temp = 1.0, int plies = 2, double k = 2.0, double c = 1.0) {
        return record_check(RECORD_PRUNED, stream, p, games, 4, ply, draw, n_rollouts, alpha, v1, v2, {off, temp, plies, k, c}, work);
    };
    EXPECT(rec(ok) == 0 && work);
    EXPECT(rec(ok, -1) == QTTT_ERR_SIZE && !work);
    EXPECT(rec(ok, 1, false, -1) == QTTT_ERR_SIZE && rec(ok, 1, false, QTTT_SELFPLAY_ROWS) == QTTT_ERR_SIZE);
    EXPECT(rec(ok, 1, true, -1) == 0 && rec(ok, 1, true, 99) == 0);                      // the stream record has no ply
    EXPECT(rec(ok, 1, true, 0, QTTT_SELFPLAY_MAX_MOVE_DRAWS) == QTTT_ERR_SIZE && rec(ok, 1, false, 0, QTTT_SELFPLAY_MAX_MOVE_DRAWS) == 0);
    EXPECT(rec(ok, 1, false, 0, 0u, 0u) == QTTT_ERR_SIZE);
    EXPECT(rec(ok, 1, false, 0, 0u, 8u, 0.0) == QTTT_ERR_SIZE && rec(ok, 1, false, 0, 0u, 8u, nan) == QTTT_ERR_SIZE);
    EXPECT(rec(ok, 1, false, 0, 0u, 8u, 1.0, inf) == QTTT_ERR_SIZE && rec(ok, 1, false, 0, 0u, 8u, 1.0, 1.0, nan) == QTTT_ERR_SIZE);
    EXPECT(rec(ok, 1, false, 0, 0u, 8u, 1.0, 1.0, -1.0, -1) == QTTT_ERR_SIZE);
    EXPECT(rec(ok, 1, false, 0, 0u, 8u, 1.0, 1.0, -1.0, 0, 0.0) == QTTT_ERR_SIZE && rec(ok, 1, false, 0, 0u, 8u, 1.0, 1.0, -1.0, 0, inf) == QTTT_ERR_SIZE);
    EXPECT(rec(ok, 1, false, 0, 0u, 8u, 1.0, 1.0, -1.0, 0, 1.0, -1) == QTTT_ERR_SIZE);
    EXPECT(rec(ok, 1, false, 0, 0u, 8u, 1.0, 1.0, -1.0, 0, 1.0, QTTT_SELFPLAY_ROWS + 1) == QTTT_ERR_SIZE);
    EXPECT(rec(ok, 1, false, 0, 0u, 8u, 1.0, 1.0, -1.0, 0, 1.0, 0) == 0);                // sample_plies = 0: the plain move
    for (double bad : {-1.0, nan, inf}) EXPECT(rec(ok, 1, false, 0, 0u, 8u, 1.0, 1.0, -1.0, 0, 1.0, 2, bad) == QTTT_ERR_SIZE);
    for (double bad : {nan, inf, -inf}) EXPECT(rec(ok, 1, false, 0, 0u, 8u, 1.0, 1.0, -1.0, 0, 1.0, 2, 2.0, bad) == QTTT_ERR_SIZE);
    const RecordArgs none = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    EXPECT(rec(none, 0) == 0 && !work && rec(none, -1) == QTTT_ERR_SIZE && rec(none, 1, false, 10) == QTTT_ERR_SIZE);
    for (int i = 0; i < 10; ++i) {                               // every pointer is required; nulls come before alignment
        const void *f[10] = {T8, A8, A4, A, A, A2, A, A, A, A};
        f[i] = nullptr;
        const RecordArgs q = {f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7], f[8], f[9]};
        EXPECT(rec(q) == QTTT_ERR_NULL);
    }
    RecordArgs p = ok;
    p.tree = T8;
    EXPECT(rec(p) == QTTT_ERR_ACTION);
    p = ok; p.states = A8;
    EXPECT(rec(p) == QTTT_ERR_ACTION);
    p = ok; p.pi = A4;
    EXPECT(rec(p) == QTTT_ERR_ACTION);
    p = ok; p.v = A2;
    EXPECT(rec(p) == QTTT_ERR_ACTION && !work);
    p = ok; p.mask = A2; p.done = A2; p.actions = A2;
    EXPECT(rec(p) == 0 && work);
}

// the other modes of the one record check, lockstep and stream: every class of bad argument, and what a mode must NOT test
static void check_record_modes() {
    bool work = true;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const uint32_t DRAWS = QTTT_SELFPLAY_MAX_MOVE_DRAWS;
    const RecordArgs &ok = RECORD_OK;
    const RecordExtra sampled = {0, 1.0, 2}, gumbel = {0, 0.0, 0, 0.0, 0.0, A, 50.0, 1.0};
    // every field of another mode at a value that mode would refuse: a mode looks at its own fields only
    const RecordExtra foreign_plain = {-1, nan, -1, nan, nan, A8, nan, nan}, foreign_sampled = {0, 1.0, 2, nan, nan, A8, nan, nan};
    const RecordExtra foreign_gumbel = {-1, nan, -1, nan, nan, A, 50.0, 1.0};
    for (int form = 0; form < 2; ++form) {
        const bool st = form == 1;
        auto chk = [&](int mode, const RecordExtra &x, const RecordArgs &p = RECORD_OK, int64_t games = 1, int64_t capacity = 4, int ply = 0, uint32_t draw = 0u, uint32_t n_rollouts = 8u,
                       double alpha = 1.0, double v1 = 1.0, double v2 = -1.0) {
            return record_check(mode, st, p, games, capacity, ply, draw, n_rollouts, alpha, v1, v2, x, work);
        };
        const struct { int mode; RecordExtra good, foreign; } modes[3] = {
            {RECORD_PLAIN, {}, foreign_plain}, {RECORD_SAMPLED, sampled, foreign_sampled}, {RECORD_GUMBEL, gumbel, foreign_gumbel}};
        for (const auto &m : modes) {
            const bool gm = m.mode == RECORD_GUMBEL, draws = m.mode == RECORD_SAMPLED;
            EXPECT(chk(m.mode, m.good) == 0 && work);
            EXPECT(chk(m.mode, m.foreign) == 0 && work);
            // sizes
            EXPECT(chk(m.mode, m.good, ok, -1) == QTTT_ERR_SIZE && !work);
            EXPECT(chk(m.mode, m.good, ok, 1, 0) == QTTT_ERR_SIZE && chk(m.mode, m.good, ok, 1, (int64_t)QTTT_TREE_MAX_CAPACITY + 1) == QTTT_ERR_SIZE);
            EXPECT(chk(m.mode, m.good, ok, 1, 4, -1) == (st ? 0 : QTTT_ERR_SIZE));                   // the ply: lockstep only
            EXPECT(chk(m.mode, m.good, ok, 1, 4, QTTT_SELFPLAY_ROWS) == (st ? 0 : QTTT_ERR_SIZE));
            EXPECT(chk(m.mode, m.good, ok, 1, 4, QTTT_SELFPLAY_ROWS - 1) == 0);
            EXPECT(chk(m.mode, m.good, ok, 1, 4, 0, DRAWS) == (st && draws ? QTTT_ERR_SIZE : 0));   // the draw: the drawing stream records only
            EXPECT(chk(m.mode, m.good, ok, 1, 4, 0, DRAWS - 1u) == 0);
            EXPECT(chk(m.mode, m.good, ok, 1, 4, 0, 0u, 0u) == (gm ? 0 : QTTT_ERR_SIZE));            // the Gumbel record has no budget and no alpha
            for (double bad : {0.0, -1.0, nan, inf}) EXPECT(chk(m.mode, m.good, ok, 1, 4, 0, 0u, 8u, bad) == (gm ? 0 : QTTT_ERR_SIZE));
            for (double bad : {nan, inf, -inf}) {
                EXPECT(chk(m.mode, m.good, ok, 1, 4, 0, 0u, 8u, 1.0, bad) == QTTT_ERR_SIZE);
                EXPECT(chk(m.mode, m.good, ok, 1, 4, 0, 0u, 8u, 1.0, 1.0, bad) == QTTT_ERR_SIZE);
            }
            // sizes come first, then the empty batch, then nulls, then alignment
            const RecordArgs none = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
            RecordExtra norec = m.good;
            norec.rec = nullptr;
            EXPECT(chk(m.mode, norec, none, 0) == 0 && !work && chk(m.mode, norec, none, -1) == QTTT_ERR_SIZE);
            for (int i = 0; i < 10; ++i) {
                const void *f[10] = {T8, A8, A4, A, A, A2, A, A, A, A};
                f[i] = nullptr;
                const RecordArgs q = {f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7], f[8], f[9]};
                EXPECT(chk(m.mode, m.good, q) == QTTT_ERR_NULL);
            }
            RecordArgs p = ok;
            p.tree = T8;
            EXPECT(chk(m.mode, m.good, p) == QTTT_ERR_ACTION);
            p = ok; p.states = A8;
            EXPECT(chk(m.mode, m.good, p) == QTTT_ERR_ACTION);
            p = ok; p.pi = A4;
            EXPECT(chk(m.mode, m.good, p) == QTTT_ERR_ACTION);
            p = ok; p.v = A2;
            EXPECT(chk(m.mode, m.good, p) == QTTT_ERR_ACTION && !work);
            p = ok; p.mask = A2; p.done = A2; p.action36 = A2; p.length = A2; p.winner = A2; p.actions = A2;
            EXPECT(chk(m.mode, m.good, p) == 0 && work);
        }
        // the sampled record's own
        RecordExtra x = sampled;
        x.board_offset = -1;
        EXPECT(chk(RECORD_SAMPLED, x) == QTTT_ERR_SIZE);
        for (double bad : {0.0, -1.0, nan, inf}) { x = sampled; x.temperature = bad; EXPECT(chk(RECORD_SAMPLED, x) == QTTT_ERR_SIZE); }
        for (int bad : {-1, QTTT_SELFPLAY_ROWS + 1}) { x = sampled; x.sample_plies = bad; EXPECT(chk(RECORD_SAMPLED, x) == QTTT_ERR_SIZE); }
        x = sampled; x.sample_plies = 0;
        EXPECT(chk(RECORD_SAMPLED, x) == 0);
        x.sample_plies = QTTT_SELFPLAY_ROWS;
        EXPECT(chk(RECORD_SAMPLED, x) == 0);
        // the Gumbel record's own: the scales, and rec required and 16-byte aligned
        for (double bad : {-0.5, nan, inf}) { x = gumbel; x.c_visit = bad; EXPECT(chk(RECORD_GUMBEL, x) == QTTT_ERR_SIZE); }
        for (double bad : {nan, inf, -inf}) { x = gumbel; x.c_scale = bad; EXPECT(chk(RECORD_GUMBEL, x) == QTTT_ERR_SIZE); }
        x = gumbel; x.c_visit = 0.0; x.c_scale = -3.0;
        EXPECT(chk(RECORD_GUMBEL, x) == 0);
        x = gumbel; x.rec = nullptr;
        EXPECT(chk(RECORD_GUMBEL, x) == QTTT_ERR_NULL);
        RecordArgs p = ok;
        p.tree = T8;
        EXPECT(chk(RECORD_GUMBEL, x, p) == QTTT_ERR_NULL);                                           // nulls come before alignment
        x.rec = A8;
        EXPECT(chk(RECORD_GUMBEL, x) == QTTT_ERR_ACTION && !work);
    }
}

// the plain and the Gumbel select through the one select check
static void check_select_rules() {
    bool work = true;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const SelectExtra gumbel = {0.0, A, A4, 16, 0, 50.0, 1.0};
    const SelectExtra foreign_plain = {nan, A8, A2, 0, -1, nan, nan}, foreign_gumbel = {nan, A, A4, 16, 0, 50.0, 1.0};
    const struct { int rule; SelectExtra good, foreign; } rules[2] = {{SELECT_PUCT, {}, foreign_plain}, {SELECT_GUMBEL, gumbel, foreign_gumbel}};
    for (const auto &r : rules) {
        auto sel = [&](const SelectExtra &x, const void *tree, int64_t games = 1, int64_t capacity = 4, uint32_t idx0 = 0u, int leaves = 2,
                       int64_t off = 0, double vl = 1.0, const void *paths = A, const void *leaf = A8) {
            return select_batch_check(r.rule, tree, games, capacity, idx0, leaves, off, vl, paths, leaf, x, work);
        };
        EXPECT(sel(r.good, T) == 0 && work);
        EXPECT(sel(r.foreign, T) == 0 && work);
        EXPECT(sel(r.good, T, -1) == QTTT_ERR_SIZE && !work);
        EXPECT(sel(r.good, T, INT64_MAX / (256 * (int64_t)QTTT_TREE_MAX_LEAVES) + 1) == QTTT_ERR_SIZE);
        EXPECT(sel(r.good, T, 1, 0) == QTTT_ERR_SIZE && sel(r.good, T, 1, (int64_t)QTTT_TREE_MAX_CAPACITY + 1) == QTTT_ERR_SIZE);
        EXPECT(sel(r.good, T, 1, 4, (uint32_t)QTTT_TREE_MAX_ROLLOUTS - 1u) == QTTT_ERR_SIZE);
        EXPECT(sel(r.good, T, 1, 4, (uint32_t)QTTT_TREE_MAX_ROLLOUTS - 2u) == 0);
        EXPECT(sel(r.good, T, 1, 4, 0u, 0) == QTTT_ERR_SIZE && sel(r.good, T, 1, 4, 0u, QTTT_TREE_MAX_LEAVES + 1) == QTTT_ERR_SIZE);
        EXPECT(sel(r.good, T, 1, 4, 0u, 2, -1) == QTTT_ERR_SIZE);
        for (double bad : {-1.0, nan, inf}) EXPECT(sel(r.good, T, 1, 4, 0u, 2, 0, bad) == QTTT_ERR_SIZE);
        EXPECT(sel(r.good, T, 1, 4, 0u, 2, 0, 0.0) == 0);
        SelectExtra norec = r.good;
        norec.rec = norec.visit_table = nullptr;
        EXPECT(sel(norec, nullptr, 0, 4, 0u, 2, 0, 1.0, nullptr, nullptr) == 0 && !work);
        EXPECT(sel(norec, nullptr, -1, 4, 0u, 2, 0, 1.0, nullptr, nullptr) == QTTT_ERR_SIZE);
        EXPECT(sel(r.good, nullptr, 1, 4, 0u, 2, 0, 1.0, A8) == QTTT_ERR_NULL);                      // nulls come before alignment
        EXPECT(sel(r.good, T8, 1, 4, 0u, 2, 0, 1.0, nullptr) == QTTT_ERR_NULL);
        EXPECT(sel(r.good, T, 1, 4, 0u, 2, 0, 1.0, A, nullptr) == QTTT_ERR_NULL);
        EXPECT(sel(r.good, T8) == QTTT_ERR_ACTION);
        EXPECT(sel(r.good, T, 1, 4, 0u, 2, 0, 1.0, A8) == QTTT_ERR_ACTION && !work);
        EXPECT(sel(r.good, T, 1, 4, 0u, 2, 0, 1.0, A, A2) == 0 && work);                             // the leaves' planes: any address
    }
    // the Gumbel select's own: the budget, the position in it, the scales, rec and visit_table
    auto gsel = [&](const SelectExtra &x, int leaves = 2, const void *tree = T) {
        return select_batch_check(SELECT_GUMBEL, tree, 1, 4, 0u, leaves, 0, 1.0, A, A, x, work);
    };
    SelectExtra x = gumbel;
    for (int bad : {0, -1, (int)QTTT_TREE_MAX_ROLLOUTS + 1}) { x = gumbel; x.n_sims = bad; EXPECT(gsel(x) == QTTT_ERR_SIZE); }
    x = gumbel; x.sim_idx0 = -1;
    EXPECT(gsel(x) == QTTT_ERR_SIZE);
    x.sim_idx0 = 15;
    EXPECT(gsel(x) == QTTT_ERR_SIZE && gsel(x, 1) == 0);                                             // sim_idx0 + leaves <= n_sims
    x.sim_idx0 = 14;
    EXPECT(gsel(x) == 0);
    for (double bad : {-0.5, nan, inf}) { x = gumbel; x.c_visit = bad; EXPECT(gsel(x) == QTTT_ERR_SIZE); }
    for (double bad : {nan, inf, -inf}) { x = gumbel; x.c_scale = bad; EXPECT(gsel(x) == QTTT_ERR_SIZE); }
    x = gumbel; x.rec = nullptr;
    EXPECT(gsel(x) == QTTT_ERR_NULL);
    x = gumbel; x.visit_table = nullptr;
    EXPECT(gsel(x) == QTTT_ERR_NULL && gsel(x, 2, T8) == QTTT_ERR_NULL);
    x = gumbel; x.rec = A8;
    EXPECT(gsel(x) == QTTT_ERR_ACTION);
    x = gumbel; x.visit_table = A2;
    EXPECT(gsel(x) == QTTT_ERR_ACTION && !work);
    EXPECT(gsel(gumbel) == 0 && work);
}

int main() {
    std::srand(2030);
    check_points();
    check_roots();
    check_arguments();
    check_record_modes();
    check_select_rules();
    if (failures) {
        std::printf("forced_host_check: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("forced_host_check: ok\n");
    return 0;
}
