/* qttt_tree_subset.h — leaf-parallel rounds and root noise for a LISTED SUBSET of the games of the device search trees
 * (DESIGN.md §31): what playout cap randomisation (Wu, "Accelerating Self-Play Learning in Go", 2019, section 3.1) needs of
 * the trees, so that the games that stop searching early cost no network rows.  Part of the C ABI of libqttt_hip.so
 * (additive entries of QTTT_ABI_VERSION 6; included by qttt.h after qttt_tree_forced.h; the buffer layout, conventions
 * and error order of qttt_tree.h, the round, the path records and the in-flight invariant of qttt_tree_leaves.h, the
 * noise of qttt_tree_explore.h and the forced root rule of qttt_tree_forced.h hold here).
 *
 * ---- The list.  ids is i32[n_ids] on the device: ASCENDING, DISTINCT, every entry in 0..games-1.  That is the caller's
 * precondition; the host cannot test it without reading the device.  (An entry outside 0..games-1 is skipped by the
 * kernels; a game listed twice is searched by two waves at once and its bytes are then undefined.)  Wave w of a launch
 * takes game g = ids[w].  GAMES THAT ARE NOT LISTED ARE NOT TOUCHED, not one byte of their tree slots.
 *
 * ---- A subset round of K = `leaves` rollouts is
 *   qttt_tree_select_batch_subset -> qttt_evaluate(leaf_state, n = n_ids * K, value + probs) -> qttt_tree_backup_batch_subset
 * with the rows packed densely: the path record, the leaf, its value and its priors row of descent j of game ids[w] are
 * row w * K + j, NOT g * K + j.  leaf_state holds n_ids * K boards (qttt_state_bytes(n_ids * K) bytes) and paths has
 * qttt_tree_paths_bytes(n_ids, K) bytes.
 *
 * qttt_tree_select_batch_subset searches game g = ids[w] by the select rule of qttt_tree_select_batch: the same collapse
 * bits, qttt_hash(seed, board_offset + g, QTTT_TREE_SELECT_BASE + rollout_idx0 + j) — addressed by the GAME, not by w —
 * the same in-flight marks, the same overflow rule, the same update of the game header.  forced_k < 0 is the plain PUCT
 * root; forced_k >= 0 is the forced root rule of qttt_tree_forced.h with that k (so forced_k = 0 forces nothing).  With
 * n_ids == games and ids = 0, 1, ..., games-1 the launch leaves the bytes of the tree, of paths and of leaf_state that
 * qttt_tree_select_batch (qttt_tree_select_batch_forced) leaves.
 *
 * qttt_tree_backup_batch_subset applies the backup rule of qttt_tree_backup_batch to game ids[w] with rows w * K + j.
 * The in-flight invariant holds per game: a listed game must be backed up by the subset backup of the same list before
 * any other tree entry reads it.
 *
 * ---- qttt_tree_root_noise_subset is qttt_tree_root_noise for the listed games only.  The draws are addressed by
 * (seed, board_offset + g, noise_idx) as there, so a listed game gets exactly the noise that the full launch would give
 * it.  noise f64[games, 36] and applied u8[games] (both nullable) are indexed by the GAME: row g is written for a listed
 * game, the other rows keep what they held.
 *
 * Errors, in qttt_tree.h's order, before any device work.  QTTT_ERR_SIZE: the sizes of the entry that is extended (games,
 * capacity, board_offset, leaves, rollout_idx0 + leaves, virtual_loss for the select; games, capacity, leaves for the
 * backup; games, capacity, board_offset, noise_idx, epsilon, alpha for the noise), then forced_k not finite (negative is
 * allowed), then n_ids < 0 or n_ids > games.  0 with no device work for games == 0 or n_ids == 0.  QTTT_ERR_NULL for a null
 * pointer that the extended entry requires, or a null ids.  QTTT_ERR_ACTION for the extended entry's alignments, or ids
 * not 4-byte aligned. */
#ifndef QTTT_TREE_SUBSET_H
#define QTTT_TREE_SUBSET_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int qttt_tree_select_batch_subset(void *tree, int64_t games, int64_t capacity, uint64_t seed, uint32_t rollout_idx0,
                                  int leaves, int64_t board_offset, double c_puct, double virtual_loss, double forced_k,
                                  const int32_t *ids, int64_t n_ids, void *paths, void *leaf_state, void *stream);

int qttt_tree_backup_batch_subset(void *tree, int64_t games, int64_t capacity, int leaves, const int32_t *ids,
                                  int64_t n_ids, const void *paths, const float *leaf_value, const float *leaf_probs,
                                  void *stream);

int qttt_tree_root_noise_subset(void *tree, int64_t games, int64_t capacity, uint64_t seed, uint32_t noise_idx,
                                int64_t board_offset, double epsilon, double alpha, const int32_t *ids, int64_t n_ids,
                                double *noise, uint8_t *applied, void *stream);

#ifdef __cplusplus
}
#endif
#endif
