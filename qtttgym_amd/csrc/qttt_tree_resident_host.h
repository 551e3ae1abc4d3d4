// qttt_tree_resident_host.h — plain C++ without HIP: what the host decides of the resident search
// (include/qttt_tree_resident.h): the tile (games per workgroup), the round plan of a launch, and the entry's argument check
// in the order include/qttt.h promises: the sizes of the subset select (games, capacity, board_offset, leaves, the draw-index
// bound, virtual_loss, forced_k) and of the value rollout (precision); an empty batch or no rollouts; the required pointers;
// the alignments.  tools/resident_host_check.cpp is the stand-alone program over this header.
#ifndef QTTT_TREE_RESIDENT_HOST_H
#define QTTT_TREE_RESIDENT_HOST_H
#include "qttt_checks.h"

namespace {

// rows of the network tile of a precision (NNCfg<PREC>::M of qttt_nn_kernels.h, which asserts the two agree), 0 = bad
inline int resident_tile_rows(int precision) { return precision == QTTT_NN_F32 ? 64 : precision == QTTT_NN_BF16 ? 128 : 0; }
inline bool resident_leaves_bad(int leaves) { return leaves < 1 || leaves > QTTT_TREE_MAX_LEAVES; }

// T: the games of one workgroup
inline int resident_games_per_group(int leaves, int precision) {
    const int rows = resident_tile_rows(precision);
    if (resident_leaves_bad(leaves) || rows == 0) return QTTT_ERR_SIZE;
    return rows / leaves;
}

// the size of the round that starts with `done` of `rollouts` rollouts made: the kernel's schedule and the plan's
#ifdef __HIPCC__
__host__ __device__
#endif
inline uint32_t resident_round(uint32_t leaves, uint32_t rollouts, uint32_t done) {
    const uint32_t left = rollouts - done;
    return left < leaves ? left : leaves;
}

inline int resident_plan(int leaves, uint32_t rollouts, int32_t *rounds_out, int cap) {
    if (resident_leaves_bad(leaves) || rollouts > QTTT_TREE_MAX_ROLLOUTS || cap < 0) return QTTT_ERR_SIZE;
    if (cap > 0 && !rounds_out) return QTTT_ERR_NULL;
    int n = 0;
    for (uint32_t done = 0; done < rollouts; ++n) {
        const uint32_t k = resident_round((uint32_t)leaves, rollouts, done);
        if (n < cap) rounds_out[n] = (int32_t)k;
        done += k;
    }
    return n;
}

// `work`: the call has something to launch (games > 0 and rollouts > 0)
inline int resident_search_check(const void *tree, int64_t games, int64_t capacity, uint32_t rollout_idx0, int leaves,
                                 uint32_t rollouts, int64_t board_offset, double virtual_loss, double forced_k,
                                 const void *weights, int precision, bool &work) {
    work = false;
    if (tree_size_bad(games, capacity) || board_offset < 0 || tree_leaves_bad(games, leaves) ||
        (uint64_t)rollout_idx0 + (uint64_t)rollouts > QTTT_TREE_MAX_ROLLOUTS || !is_finite(virtual_loss) || virtual_loss < 0.0 ||
        !is_finite(forced_k) || resident_tile_rows(precision) == 0)
        return QTTT_ERR_SIZE;
    if (games == 0 || rollouts == 0u) return 0;
    if (any_null(tree, weights)) return QTTT_ERR_NULL;
    if (misaligned(tree, 16) || misaligned(weights, 16)) return QTTT_ERR_ACTION;
    work = true;
    return 0;
}

}  // namespace

#endif  // QTTT_TREE_RESIDENT_HOST_H
