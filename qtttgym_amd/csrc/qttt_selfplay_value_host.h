// qttt_selfplay_value_host.h — plain C++ without HIP: the argument checks of include/qttt_selfplay_value.h in the order
// that header promises (on qttt_checks.h), and the row arithmetic of qttt_selfplay_value_targets for ONE game, which the kernel
// (qttt_selfplay_value_kernels.h) runs in a lane and a stand-alone program runs under the host sanitizers
// (tools/value_host_check.cpp).  Kept apart from the kernels for that program's sake.
#ifndef QTTT_SELFPLAY_VALUE_HOST_H
#define QTTT_SELFPLAY_VALUE_HOST_H
#include "qttt_checks.h"

#ifdef __HIPCC__
#define QTTT_VALUE_HD __host__ __device__
#else
#define QTTT_VALUE_HD
#endif

namespace {

inline bool value_lambda_bad(double lambda) { return !(lambda >= 0.0 && lambda <= 1.0); }      // NaN fails both

// `work`: the call has something to launch (games > 0)
inline int value_record_check(const void *tree, int64_t games, int64_t capacity, int ply, const uint8_t *length, const float *q,
                              const float *v, bool &work) {
    work = false;
    if (tree_size_bad(games, capacity) || ply > QTTT_SELFPLAY_ROWS - 1) return QTTT_ERR_SIZE;
    if (games == 0) return 0;
    if (!tree || !length || !q || !v) return QTTT_ERR_NULL;
    if (misaligned(tree, 16) || misaligned(q, 4) || misaligned(v, 4)) return QTTT_ERR_ACTION;
    work = true;
    return 0;
}

inline int value_targets_check(int64_t games, int mode, double lambda, const uint8_t *length, const uint8_t *done, const float *q,
                               const float *v, bool &work) {
    work = false;
    if (games < 0 || (mode != QTTT_VALUE_MIX && mode != QTTT_VALUE_TD) || value_lambda_bad(lambda)) return QTTT_ERR_SIZE;
    if (games == 0) return 0;
    if (!length || !done || !q || !v) return QTTT_ERR_NULL;
    if (misaligned(q, 4) || misaligned(v, 4)) return QTTT_ERR_ACTION;
    work = true;
    return 0;
}

// the one rounding of a row: f64 -> f32, a zero (a tiny negative that underflows included) stored as +0.0
QTTT_VALUE_HD inline float value_round(double x) {
    const float y = (float)x;
    return y == 0.0f ? 0.0f : y;
}

// (1 - lambda) * a + lambda * b: two rounded products, then their rounded sum — never an FMA
QTTT_VALUE_HD inline double value_blend(double lambda, double a, double b) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double x = (1.0 - lambda) * a, y = lambda * b;
    return x + y;
}

// Game g of a batch of `games`: rows t < L of v rewritten in place (include/qttt_selfplay_value.h, word for word).
// exact may be null.  L <= QTTT_SELFPLAY_ROWS is the caller's clamp; element (t, g) of a row field is at t * games + g.
QTTT_VALUE_HD inline void value_targets_game(int mode, double lambda, int L, int64_t games, int64_t g, const uint8_t *done,
                                             const uint8_t *exact, const float *q, float *v) {
    if (mode == QTTT_VALUE_MIX) {
        for (int t = 0; t < QTTT_SELFPLAY_ROWS; ++t) {
            if (t >= L) break;
            const int64_t i = (int64_t)t * games + g;
            if (done[i] != 0 || (exact && exact[i] == 1)) continue;
            v[i] = value_round(value_blend(lambda, (double)v[i], (double)q[i]));
        }
        return;
    }
    if (L < 2) return;                                           // row L - 1 is never written
    int64_t i = (int64_t)(L - 1) * games + g;                    // row t + 1 while the loop runs
    double ret = (double)v[i];
    bool keep = done[i] != 0 || (exact && exact[i] == 1);        // is b the row's v?
    for (int k = 0; k < QTTT_SELFPLAY_ROWS - 1; ++k) {
        const int t = L - 2 - k;
        if (t < 0) break;
        const double b = keep ? (double)v[i] : (double)q[i];
        ret = 0.0 - value_blend(lambda, b, ret);
        i -= games;                                              // row t
        const bool ex = exact && exact[i] == 1;
        if (ex) ret = (double)v[i];
        else v[i] = value_round(ret);
        keep = ex || done[i] != 0;
    }
}

}  // namespace

#endif  // QTTT_SELFPLAY_VALUE_HOST_H
