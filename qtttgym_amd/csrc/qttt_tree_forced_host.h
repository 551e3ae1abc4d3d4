// qttt_tree_forced_host.h — plain C++ without HIP: the factor's and the root entry's argument checks (the forced select's and
// the pruned records' are qttt_selfplay_record_host.h's), and the arithmetic of include/qttt_tree_forced.h's rules for ONE
// action (the forced predicate, min(N, F), the pruned visit count),
// which the kernels (qttt_tree_forced_kernels.h) run in a lane and a stand-alone program runs under the host sanitizers
// (tools/forced_host_check.cpp).  Kept apart from the kernels for that program's sake.
#ifndef QTTT_TREE_FORCED_HOST_H
#define QTTT_TREE_FORCED_HOST_H
#include "qttt_checks.h"

#ifdef __HIPCC__
#define QTTT_FORCED_HD __host__ __device__
#else
#define QTTT_FORCED_HD
#endif

namespace {

inline bool forced_k_bad(double k) { return !(is_finite(k) && k >= 0.0); }

// `work`: the call has something to launch (games > 0)
inline int forced_root_check(const void *tree, int64_t games, int64_t capacity, double forced_k, double c_puct,
                             const int32_t *n_pruned, bool &work) {
    work = false;
    if (tree_size_bad(games, capacity) || forced_k_bad(forced_k) || !is_finite(c_puct)) return QTTT_ERR_SIZE;
    if (games == 0) return 0;
    if (!tree) return QTTT_ERR_NULL;
    if (misaligned(tree, 16) || misaligned(n_pruned, 4)) return QTTT_ERR_ACTION;
    work = true;
    return 0;
}

// (k * P) * S: two rounded products
QTTT_FORCED_HD inline double forced_threshold(double k, double P, uint32_t S) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double kp = k * P;
    return kp * (double)S;
}

// the predicate: n > 0 and n * n < (k P) S
QTTT_FORCED_HD inline bool forced_is(uint32_t n, double k, double P, uint32_t S) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double nn = (double)n * (double)n;
    return n > 0u && nn < forced_threshold(k, P, S);
}

// min(cap, F), F = the smallest integer with F * F >= t; 0 for a t that is not a number.  The square root only proposes:
// the two short loops settle F by the definition's own comparison.
QTTT_FORCED_HD inline uint32_t forced_floor(double t, uint32_t cap) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    if ((double)cap * (double)cap < t) return cap;               // F > cap
    if (!(t > 0.0)) return 0u;
    uint32_t F = (uint32_t)__builtin_sqrt(t);                    // t <= cap * cap: it fits
    for (int i = 0; i < 2; ++i)
        if ((double)F * (double)F < t) ++F;
    for (int i = 0; i < 2; ++i)
        if (F > 0u && (double)(F - 1u) * (double)(F - 1u) >= t) --F;
    return F < cap ? F : cap;
}

// the left side of the prune's inequality: tree_score (qttt_tree_kernels.h) with N - d visits and Q held fixed
QTTT_FORCED_HD inline double forced_lhs(double Q, double P, double sq, uint32_t N, uint32_t d, double c_puct) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double u = P * sq / (double)(1u + (N - d));
    return Q + c_puct * u;
}

// N' of an action that is not c*: sq = sqrt(Ntot), best = score(c*)
QTTT_FORCED_HD inline uint32_t forced_pruned_visits(double W, uint32_t N, double P, double k, uint32_t S, double sq,
                                                    double c_puct, double best) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    if (N == 0u) return 0u;
    const uint32_t m = forced_floor(forced_threshold(k, P, S), N);
    if (m == 0u) return N;
    const double Q = W / (double)N;
    uint32_t d = 0u;
    if (forced_lhs(Q, P, sq, N, m, c_puct) < best) {
        d = m;
    } else if (c_puct >= 0.0 && m > 1u && forced_lhs(Q, P, sq, N, 1u, c_puct) < best) {
        uint32_t lo = 1u, hi = m;                                // the inequality holds at lo and not at hi
        for (int it = 0; it < 32 && hi - lo > 1u; ++it) {
            const uint32_t mid = lo + (hi - lo) / 2u;
            if (forced_lhs(Q, P, sq, N, mid, c_puct) < best) lo = mid;
            else hi = mid;
        }
        d = lo;
    }
    const uint32_t left = N - d;
    return (d > 0u && left <= 1u) ? 0u : left;
}

}  // namespace

#endif  // QTTT_TREE_FORCED_HOST_H
