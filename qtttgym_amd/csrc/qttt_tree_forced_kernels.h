// qttt_tree_forced_kernels.h — forced playouts at the root and policy target pruning (include/qttt_tree_forced.h, DESIGN.md
// §30): ForcedRootRule is the root rule of tree_select_batch_forced_kernel, forced_root gives the predicate and the pruned
// visit counts of a root as it stands, which tree_root_forced_kernel writes out and selfplay_record_kernel<RECORD_PRUNED>
// (qttt_selfplay_kernels.h) makes its pi row of.
//
// Mapping: the tree kernels' (qttt_tree_kernels.h).  ONE WAVEFRONT PER GAME, lane a = action a, four games per workgroup.
// The select is tree_select_batch_game, the body of qttt_tree_select_batch, with ForcedRootRule as the root rule of the one
// tree_descend: there is no second descent.  The rule reads the root's slots that tree_descend has loaded already and the
// root's 36 priors (one coalesced 144-byte read); it stores nothing.  Its reductions are two six-step butterflies (the u32
// sum of the visits, wave_argmax over the forced lanes).  forced_root adds one more argmax (c*) and one broadcast; the
// per-lane arithmetic is qttt_tree_forced_host.h's, whose only loop is a bisection of at most 32 steps.  No atomics, no LDS
// of their own, no scratch, nothing handed between lanes through memory.
#ifndef QTTT_TREE_FORCED_KERNELS_H
#define QTTT_TREE_FORCED_KERNELS_H
#include "qttt_tree_leaves_kernels.h"
#include "qttt_tree_forced_host.h"
#include "qttt_tree_forced.h"

namespace {

__device__ __forceinline__ u32 forced_wave_sum(u32 x) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) x += __shfl_xor(x, m);
    return x;
}

// P of lane a's action at a node with header h and prior row `row`: tree_prior where the node has priors and the action is
// legal, 0 elsewhere
__device__ __forceinline__ double forced_prior(const TreeNodeHdr &h, const float *row, bool legal, u32 lane) {
    if (!legal || !(h.flags & TN_PRIORS)) return 0.0;
    if (h.flags & TN_UNIFORM) return g_uniform_priors.p[__builtin_popcountll(h.legal)];
    return (double)row[lane];
}

// the root rule of a descent under forced playouts: the forced action of largest in-flight score, or -1
struct ForcedRootRule {
    static constexpr bool on = true;
    const float *row;                  // the root's priors
    double k, c_puct, vloss;
    __device__ __forceinline__ int operator()(const TreeNodeHdr &h, const TreeSlot &s, u32 lane) const {
        if (!(k > 0.0)) return -1;                               // wave-uniform: nothing is forced
        const bool legal = lane < 36u && ((h.legal >> lane) & 1ull);
        const u32 n = legal ? tree_effective(s.N) : 0u;
        const u32 S = forced_wave_sum(n);
        const double P = forced_prior(h, row, legal, lane);
        const bool forced = legal && forced_is(n, k, P, S);
        if (__ballot(forced) == 0ull) return -1;
        const double sc = tree_score_in_flight(s.W, s.N, P, tree_sqrt(tree_effective(h.Ntot)), c_puct, vloss);
        return __builtin_amdgcn_readfirstlane(wave_argmax(forced, sc, lane));
    }
};

__global__ __launch_bounds__(TREE_BLOCK) void tree_select_batch_forced_kernel(void *tree, int64_t games, int64_t capacity,
                                                                              u64 seed, u32 rollout_idx0, u32 leaves,
                                                                              u64 board_offset, double c_puct, double vloss,
                                                                              TreePathRec *paths, u64 *leafP, u64 *leafQ,
                                                                              double forced_k) {
    __shared__ __attribute__((aligned(16))) uint8_t lut[LINE_LUT_BYTES];
    fill_line_lut<TREE_BLOCK>(lut);                              // ends with the workgroup barrier
    const int64_t g = (int64_t)blockIdx.x * TREE_GAMES_PER_BLOCK + threadIdx.x / 64;
    const u32 lane = threadIdx.x & 63u;
    if (g >= games) return;
    const TreeView v = tree_view(tree, games, capacity);
    const float *row = v.prior(g, v.games[g].root);              // select never moves the root
    tree_select_batch_game(v, g, g * (int64_t)leaves, lane, lut, seed, rollout_idx0, leaves, board_offset, c_puct, vloss, paths, leafP, leafQ,
                           [&](u32) { return ForcedRootRule{row, forced_k, c_puct, vloss}; });
}

// the predicate and the pruned visits of lane a's action of a root r as it stands
struct ForcedRoot {
    bool forced;
    u32 n_pruned;                      // N', 0 where the action is not legal
};
__device__ __forceinline__ ForcedRoot forced_root(const TreeView &v, int64_t g, const TreeRootLane &r, u32 lane, double k,
                                                  double c_puct) {
    ForcedRoot o;
    const double P = forced_prior(r.h, v.prior(g, v.games[g].root), r.legal, lane);
    const u32 n = r.legal ? tree_effective(r.s.N) : 0u;
    const u32 S_now = forced_wave_sum(n);                        // every lane takes part in the butterfly
    o.forced = r.legal && !(r.h.flags & TN_TERMINAL) && forced_is(n, k, P, S_now);
    // the prune reads the record's own N: nothing is in flight at record time (tree_root_lane: 0 where not legal)
    const u32 N = r.s.N;
    const u32 S = forced_wave_sum(N);
    const double sq = tree_sqrt(r.h.Ntot);
    const int star = wave_argmax(r.legal, (double)N, lane);      // most visits, ties to the lowest action
    const double best = __shfl(tree_score(r.s.W, N, P, sq, c_puct), star < 0 ? 0 : star);
    o.n_pruned = (!r.legal || (int)lane == star) ? N : forced_pruned_visits(r.s.W, N, P, k, S, sq, c_puct, best);
    return o;
}

__global__ __launch_bounds__(TREE_BLOCK) void tree_root_forced_kernel(const void *tree, int64_t games, int64_t capacity,
                                                                      double forced_k, double c_puct, uint8_t *forced,
                                                                      int32_t *n_pruned) {
    const int64_t g = (int64_t)blockIdx.x * TREE_GAMES_PER_BLOCK + threadIdx.x / 64;
    const u32 lane = threadIdx.x & 63u;
    if (g >= games) return;
    const TreeView v = tree_view(const_cast<void *>(tree), games, capacity);
    const ForcedRoot f = forced_root(v, g, tree_root_lane(v, g, lane), lane, forced_k, c_puct);
    if (lane < 36u) {
        if (forced) forced[g * 36 + lane] = f.forced ? 1 : 0;
        if (n_pruned) n_pruned[g * 36 + lane] = (int32_t)f.n_pruned;
    }
}

}  // namespace

#endif  // QTTT_TREE_FORCED_KERNELS_H
