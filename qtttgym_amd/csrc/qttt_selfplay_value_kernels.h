// qttt_selfplay_value_kernels.h — search-value targets for self-play (include/qttt_selfplay_value.h):
// selfplay_record_value_kernel keeps the searched value of every root that the ply's record kernel is about to record,
// selfplay_value_targets_kernel rewrites a batch's value targets from those values.
//
// selfplay_record_value_kernel.  Mapping: the root kernels' (qttt_tree_kernels.h): ONE WAVEFRONT PER
// GAME, lane a = action a, the root's 36 slots one coalesced 576-byte read through tree_root_lane — the very load of
// tree_root_kernel, so W and N are what qttt_tree_root returns.  The two sums are taken in ASCENDING ACTION ORDER, which a
// butterfly is not: lane a's pair is broadcast (a wave-uniform lane index: two v_readlane per double) and added by every
// lane, 36 steps, so every lane holds the same SW and SN and lane 0 stores the one float.  The tree, length and v are read
// only; a wave writes q[r, g] and nothing else; no atomics, no LDS, no scratch.
//
// selfplay_value_targets_kernel.  Mapping: ONE LANE PER GAME: a wavefront reads 64 consecutive games of one row, so every
// load and store of v, q, done and exact is contiguous; the backward pass is at most nine dependent steps of f64
// arithmetic per lane (value_targets_game, qttt_selfplay_value_host.h: the code a host program runs under the sanitizers).
// A lane touches only its own game's column; no atomics, no LDS, no scratch.
#ifndef QTTT_SELFPLAY_VALUE_KERNELS_H
#define QTTT_SELFPLAY_VALUE_KERNELS_H
#include "qttt_tree_kernels.h"
#include "qttt_selfplay_value_host.h"

namespace {

constexpr int VALUE_TARGETS_BLOCK = 256;

// lane a's double in every lane: two v_readlane_b32 into SGPRs (a is a constant of the unrolled loop), no LDS crossbar and
// no VGPR per broadcast value
__device__ __forceinline__ double value_lane(double x, int a) {
    const u64 b = (u64)__double_as_longlong(x);
    const u32 lo = (u32)__builtin_amdgcn_readlane((int)(u32)b, a), hi = (u32)__builtin_amdgcn_readlane((int)(u32)(b >> 32), a);
    return __longlong_as_double((long long)(((u64)hi << 32) | lo));
}

// ply < 0: the stream form, the row is the game's own length[g]
__global__ __launch_bounds__(TREE_BLOCK) void selfplay_record_value_kernel(const void *tree, int64_t games, int64_t capacity,
                                                                           int ply, const uint8_t *length, float *q,
                                                                           const float *v) {
    const int64_t g = (int64_t)blockIdx.x * TREE_GAMES_PER_BLOCK + threadIdx.x / 64;
    const u32 lane = threadIdx.x & 63u;
    if (g >= games) return;
    const int len = (int)length[g];
    const int r = ply < 0 ? len : ply;
    if (r >= QTTT_SELFPLAY_ROWS || len != r) return;             // wave-uniform: not a row this ply's record looks at
    const TreeView tv = tree_view(const_cast<void *>(tree), games, capacity);
    const TreeRootLane root = tree_root_lane(tv, g, lane);       // W = 0, N = 0 where the action is not legal
    const double w = root.s.W, n = (double)root.s.N;             // 36 counts below 2^32: their f64 sum is exact
    double sw = 0.0, sn = 0.0;
#pragma unroll
    for (int a = 0; a < 36; ++a) {
        sw = sw + value_lane(w, a);
        sn = sn + value_lane(n, a);
    }
    if (lane == 0u) {
        const int64_t i = (int64_t)r * games + g;
        if (sn > 0.0) q[i] = value_round(sw / sn);
        else reinterpret_cast<u32 *>(q)[i] = reinterpret_cast<const u32 *>(v)[i];      // the row's v, bit for bit
    }
}

__global__ __launch_bounds__(VALUE_TARGETS_BLOCK) void selfplay_value_targets_kernel(int64_t games, int mode, double lambda,
                                                                                     const uint8_t *rows, const uint8_t *length,
                                                                                     const uint8_t *done, const uint8_t *exact,
                                                                                     const float *q, float *v) {
    const int64_t g = (int64_t)blockIdx.x * VALUE_TARGETS_BLOCK + threadIdx.x;
    if (g >= games) return;
    const int L = (int)(rows ? rows[g] : length[g]);
    value_targets_game(mode, lambda, L < QTTT_SELFPLAY_ROWS ? L : QTTT_SELFPLAY_ROWS, games, g, done, exact, q, v);
}

}  // namespace

#endif  // QTTT_SELFPLAY_VALUE_KERNELS_H
