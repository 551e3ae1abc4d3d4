// qttt_tree_subset_kernels.h — search rounds and root noise for a listed subset of the games (include/qttt_tree_subset.h,
// DESIGN.md §31): what playout cap randomisation needs of the trees.  Wave w of a launch takes game g = ids[w]; its path
// records, leaves, values and priors rows are w * K + j, so the network launch between the select and the backup has
// n_ids * K rows and the games that are not listed cost nothing.
//
// Mapping: the tree kernels' (qttt_tree_kernels.h).  ONE WAVEFRONT PER LISTED GAME, lane a = action a, four listed games per
// 256-thread workgroup, the LDS line table for the expansions.  ids[w] is one load at a wave-uniform address, made uniform
// with readfirstlane; an id outside 0..games-1 ends the wave before it touches the tree (the caller's precondition is a
// list of distinct ids in range: two waves on one game would race).  The bodies are the full launches' own device
// functions, called with a row base that is not g * K: tree_select_batch_game (TreePuctRoot or ForcedRootRule at the
// root), tree_backup_batch_game<false>, tree_root_noise_game.  No atomics, plain vector stores, no LDS beyond the line
// table, every loop bounded as in those functions.
#ifndef QTTT_TREE_SUBSET_KERNELS_H
#define QTTT_TREE_SUBSET_KERNELS_H
#include "qttt_tree_leaves_kernels.h"
#include "qttt_tree_explore_kernels.h"
#include "qttt_tree_forced_kernels.h"
#include "qttt_tree_subset_host.h"
#include "qttt_tree_subset.h"

namespace {

// the wave's index in the list and its game: -1 where the wave has no game (past the list, or an id out of range)
struct SubsetWave {
    int64_t w, g;
};
__device__ __forceinline__ SubsetWave subset_wave(const int32_t *ids, int64_t n_ids, int64_t games) {
    SubsetWave s;
    const u32 wave = __builtin_amdgcn_readfirstlane(threadIdx.x / 64u);
    s.w = (int64_t)blockIdx.x * TREE_GAMES_PER_BLOCK + wave;
    s.g = -1;
    if (s.w < n_ids) {
        const int32_t id = __builtin_amdgcn_readfirstlane(ids[s.w]);
        if (id >= 0 && (int64_t)id < games) s.g = id;
    }
    return s;
}

// FORCED: the forced root rule of include/qttt_tree_forced.h with factor forced_k; else the plain PUCT root
template <bool FORCED>
__global__ __launch_bounds__(TREE_BLOCK) void tree_select_batch_subset_kernel(void *tree, int64_t games, int64_t capacity,
                                                                              u64 seed, u32 rollout_idx0, u32 leaves,
                                                                              u64 board_offset, double c_puct, double vloss,
                                                                              double forced_k, const int32_t *ids,
                                                                              int64_t n_ids, TreePathRec *paths, u64 *leafP,
                                                                              u64 *leafQ) {
    __shared__ __attribute__((aligned(16))) uint8_t lut[LINE_LUT_BYTES];
    fill_line_lut<TREE_BLOCK>(lut);                              // ends with the workgroup barrier
    const SubsetWave s = subset_wave(ids, n_ids, games);
    const u32 lane = threadIdx.x & 63u;
    if (s.g < 0) return;
    const TreeView v = tree_view(tree, games, capacity);
    const int64_t row0 = s.w * (int64_t)leaves;
    if constexpr (FORCED) {
        const float *row = v.prior(s.g, v.games[s.g].root);      // select never moves the root
        tree_select_batch_game(v, s.g, row0, lane, lut, seed, rollout_idx0, leaves, board_offset, c_puct, vloss, paths, leafP,
                               leafQ, [&](u32) { return ForcedRootRule{row, forced_k, c_puct, vloss}; });
    } else {
        tree_select_batch_game(v, s.g, row0, lane, lut, seed, rollout_idx0, leaves, board_offset, c_puct, vloss, paths, leafP,
                               leafQ, [](u32) { return TreePuctRoot(); });
    }
}

__global__ __launch_bounds__(TREE_BLOCK) void tree_backup_batch_subset_kernel(void *tree, int64_t games, int64_t capacity,
                                                                              u32 leaves, const int32_t *ids, int64_t n_ids,
                                                                              const TreePathRec *paths, const float *leaf_value,
                                                                              const float *leaf_probs) {
    const SubsetWave s = subset_wave(ids, n_ids, games);
    const u32 lane = threadIdx.x & 63u;
    if (s.g < 0) return;
    const TreeLeafRows rows = {leaf_value, leaf_probs};
    tree_backup_batch_game<false>(tree_view(tree, games, capacity), s.g, s.w * (int64_t)leaves, lane, capacity, leaves, paths,
                                  rows, rows);
}

__global__ __launch_bounds__(TREE_BLOCK) void tree_root_noise_subset_kernel(void *tree, int64_t games, int64_t capacity,
                                                                            u64 seed, u32 noise_idx, u64 board_offset,
                                                                            double epsilon, double alpha, const int32_t *ids,
                                                                            int64_t n_ids, double *noise, uint8_t *applied) {
    const SubsetWave s = subset_wave(ids, n_ids, games);
    const u32 lane = threadIdx.x & 63u;
    if (s.g < 0) return;
    tree_root_noise_game(tree_view(tree, games, capacity), s.g, lane, seed, noise_idx, board_offset, epsilon, alpha, noise,
                         applied);
}

}  // namespace

#endif  // QTTT_TREE_SUBSET_KERNELS_H
