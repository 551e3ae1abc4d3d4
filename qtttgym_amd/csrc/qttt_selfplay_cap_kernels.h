// qttt_selfplay_cap_kernels.h — the record and the harvest of playout cap randomisation (include/qttt_selfplay_cap.h,
// DESIGN.md §31): batches in which only the fully searched plies become rows.
//
// Mapping: the record's (qttt_selfplay_kernels.h): ONE WAVEFRONT PER GAME, lane a = action a, TREE_BLOCK threads.  Both
// kernels are the existing bodies, selfplay_record_game<MODE, true, true> and selfplay_harvest_game<true>: a fast game's
// wave reads its root and full[g] (one byte at a wave-uniform address) and stores the two bytes of its move; a finished
// game's back-fill reads the P word of each of its rows (at most ten lanes, one row each) for the side to move.  A wave
// touches only its own game's columns: no atomics, no LDS, nothing handed from lane to lane through memory (the terminal
// row's own state comes from the root's header in registers, not from the store lane 0 just made).
#ifndef QTTT_SELFPLAY_CAP_KERNELS_H
#define QTTT_SELFPLAY_CAP_KERNELS_H
#include "qttt_selfplay_stream_kernels.h"
#include "qttt_selfplay_cap.h"

namespace {

// MODE: RECORD_PRUNED (forced_k >= 0) or RECORD_SAMPLED (the plain pi row; sample_plies = 0 draws nothing)
template <int MODE>
__global__ __launch_bounds__(TREE_BLOCK) void selfplay_record_capped_kernel(const void *tree, int64_t games, int64_t capacity,
                                                                            int draw, u32 n_rollouts, double alpha,
                                                                            float v_first, float v_second, SelfPlayOut o,
                                                                            SelfPlaySampling<MODE> sampling,
                                                                            const uint8_t *full) {
    const int64_t g = (int64_t)blockIdx.x * TREE_GAMES_PER_BLOCK + threadIdx.x / 64;
    const u32 lane = threadIdx.x & 63u;
    if (g >= games) return;
    selfplay_record_game<MODE, true, true>(tree, games, capacity, draw, n_rollouts, alpha, v_first, v_second, o, sampling, full,
                                           g, lane);
}

__global__ __launch_bounds__(TREE_BLOCK) void selfplay_harvest_capped_kernel(const void *tree, int64_t games, int64_t capacity,
                                                                             float v_first, float v_second, SelfPlayOut o,
                                                                             SelfPlayHarvest hv) {
    const int64_t g = (int64_t)blockIdx.x * TREE_GAMES_PER_BLOCK + threadIdx.x / 64;
    const u32 lane = threadIdx.x & 63u;
    if (g >= games) return;
    selfplay_harvest_game<true>(tree, games, capacity, v_first, v_second, o, hv, g, lane);
}

}  // namespace

#endif  // QTTT_SELFPLAY_CAP_KERNELS_H
