// qttt_tree_subset_host.h — plain C++ without HIP: the argument checks of the three subset entries
// (include/qttt_tree_subset.h), in the order include/qttt.h promises: the sizes of the entry that is extended, then forced_k
// and n_ids; an empty batch or an empty list; the required pointers, ids among them; the alignments.
#ifndef QTTT_TREE_SUBSET_HOST_H
#define QTTT_TREE_SUBSET_HOST_H
#include "qttt_checks.h"

namespace {

inline bool subset_list_bad(int64_t games, int64_t n_ids) { return n_ids < 0 || n_ids > games; }

// `work`: the call has something to launch (games > 0 and n_ids > 0)
inline int subset_select_check(const void *tree, int64_t games, int64_t capacity, uint32_t rollout_idx0, int leaves,
                               int64_t board_offset, double virtual_loss, double forced_k, const void *ids, int64_t n_ids,
                               const void *paths, const void *leaf_state, bool &work) {
    work = false;
    if (tree_size_bad(games, capacity) || board_offset < 0 || tree_leaves_bad(games, leaves) ||
        (uint64_t)rollout_idx0 + (uint64_t)leaves > QTTT_TREE_MAX_ROLLOUTS || !is_finite(virtual_loss) || virtual_loss < 0.0 ||
        !is_finite(forced_k) || subset_list_bad(games, n_ids))
        return QTTT_ERR_SIZE;
    if (games == 0 || n_ids == 0) return 0;
    if (any_null(tree, paths, leaf_state, ids)) return QTTT_ERR_NULL;
    if (misaligned(tree, 16) || misaligned(paths, 16) || misaligned(ids, 4)) return QTTT_ERR_ACTION;
    work = true;
    return 0;
}

inline int subset_backup_check(const void *tree, int64_t games, int64_t capacity, int leaves, const void *ids, int64_t n_ids,
                               const void *paths, const float *leaf_value, const float *leaf_probs, bool &work) {
    work = false;
    if (tree_size_bad(games, capacity) || tree_leaves_bad(games, leaves) || subset_list_bad(games, n_ids)) return QTTT_ERR_SIZE;
    if (games == 0 || n_ids == 0) return 0;
    if (any_null(tree, paths, leaf_value, leaf_probs, ids)) return QTTT_ERR_NULL;
    if (misaligned(tree, 16) || misaligned(paths, 16) || misaligned(leaf_value, 4) || misaligned(leaf_probs, 4) ||
        misaligned(ids, 4))
        return QTTT_ERR_ACTION;
    work = true;
    return 0;
}

inline int subset_noise_check(const void *tree, int64_t games, int64_t capacity, uint32_t noise_idx, int64_t board_offset,
                              double epsilon, double alpha, const void *ids, int64_t n_ids, const double *noise, bool &work) {
    work = false;
    if (tree_size_bad(games, capacity) || board_offset < 0 || noise_idx >= QTTT_TREE_MAX_NOISE ||
        !(epsilon >= 0.0 && epsilon <= 1.0) || !is_finite(alpha) || alpha <= 0.0 || subset_list_bad(games, n_ids))
        return QTTT_ERR_SIZE;
    if (games == 0 || n_ids == 0) return 0;
    if (any_null(tree, ids)) return QTTT_ERR_NULL;
    if (misaligned(tree, 16) || misaligned(noise, 8) || misaligned(ids, 4)) return QTTT_ERR_ACTION;
    work = true;
    return 0;
}

}  // namespace

#endif  // QTTT_TREE_SUBSET_HOST_H
