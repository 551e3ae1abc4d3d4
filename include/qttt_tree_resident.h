/* qttt_tree_resident.h — the RESIDENT search of the device search trees: every round of a move's
 * leaf-parallel search in ONE launch.  Part of the C ABI of libqttt_hip.so (additive entries of QTTT_ABI_VERSION 6;
 * included by qttt.h after qttt_selfplay_cap.h; the buffer layout, conventions and error order of qttt_tree.h, the round
 * and the in-flight invariant of qttt_tree_leaves.h, the value rule of qttt_tree_value.h and the forced root rule of
 * qttt_tree_forced.h hold here).
 *
 * ---- What a launch computes.  qttt_tree_search_resident(..., leaves = K, rollouts = R, ...) leaves in `tree` the bytes
 * that the rounds of qttt_tree_resident_plan(K, R) leave when each is run as
 *   qttt_tree_select_batch[_forced] -> qttt_evaluate(value + probs) -> qttt_tree_backup_batch
 * with rollout_idx0 advanced by the round's size after each: ROUNDS OF K WHILE K ROLLOUTS REMAIN, THEN ONE ROUND OF THE
 * REMAINDER.  Every byte: game headers, node headers, slots, priors.  The collapse bits of descent j of a round that
 * starts at index i are qttt_hash(seed, board_offset + g, QTTT_TREE_SELECT_BASE + i + j), as there.  forced_k < 0 is the
 * plain PUCT root; forced_k >= 0 is the forced root rule with that k.  The network is `weights` (a packed blob of
 * qttt_nn.h) in `precision`; a row's value and priors are the bits qttt_evaluate gives for that leaf.  The path records,
 * the leaves and the network's rows of a round never leave the compute unit: there is no workspace argument.
 *
 * Two launches of R1 and R2 rollouts, R1 a multiple of K, the second at rollout_idx0 + R1, leave the bytes of one launch
 * of R1 + R2: a caller bounds a launch's duration by splitting at round boundaries.
 *
 * The root needs priors before a round of K > 1 descends from it (qttt_tree_leaves.h): the first rollout after a
 * qttt_tree_reset or qttt_tree_sync is the caller's, through qttt_tree_select -> qttt_tree_value_rollout.
 *
 * ---- Tiles.  A workgroup owns T = qttt_tree_resident_games_per_group(K, precision) consecutive games, the games
 * [T * b, T * b + T) for workgroup b: T = 64 / K (integer division) in QTTT_NN_F32 and 128 / K in QTTT_NN_BF16.  Nothing
 * is handed between workgroups and nothing waits on another workgroup.
 *
 * ---- qttt_tree_resident_plan(leaves, rollouts, rounds_out, cap) returns the number of rounds n of a launch,
 * ceil(rollouts / leaves), and writes the sizes of the first min(n, cap) of them to rounds_out (nullable when cap == 0).
 * Host only.  Their sum over all n rounds is `rollouts`.
 *
 * Errors, in qttt_tree.h's order, before any device work.  QTTT_ERR_SIZE: games, capacity, board_offset, leaves,
 * rollout_idx0 + rollouts > QTTT_TREE_MAX_ROLLOUTS (the select's draw-index bound), virtual_loss not finite or negative,
 * forced_k not finite (negative is allowed), precision neither QTTT_NN_F32 nor QTTT_NN_BF16.  0 with no device work for
 * games == 0 or rollouts == 0.  QTTT_ERR_NULL for a null tree or weights.  QTTT_ERR_ACTION for a tree or weights not
 * 16-byte aligned.  qttt_tree_resident_games_per_group: QTTT_ERR_SIZE for leaves outside 1..QTTT_TREE_MAX_LEAVES or a bad
 * precision.  qttt_tree_resident_plan: QTTT_ERR_SIZE for such leaves, rollouts > QTTT_TREE_MAX_ROLLOUTS or cap < 0, then
 * QTTT_ERR_NULL for a null rounds_out with cap > 0. */
#ifndef QTTT_TREE_RESIDENT_H
#define QTTT_TREE_RESIDENT_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int qttt_tree_search_resident(void *tree, int64_t games, int64_t capacity, uint64_t seed, uint32_t rollout_idx0,
                              int leaves, uint32_t rollouts, int64_t board_offset, double c_puct, double virtual_loss,
                              double forced_k, const void *weights, int precision, void *stream);

int qttt_tree_resident_games_per_group(int leaves, int precision);

int qttt_tree_resident_plan(int leaves, uint32_t rollouts, int32_t *rounds_out, int cap);

#ifdef __cplusplus
}
#endif
#endif
