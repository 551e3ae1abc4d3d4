/* qttt_tree_forced.h — forced playouts at a noised PUCT root and policy target pruning in the self-play record (Wu,
 * "Accelerating Self-Play Learning in Go", 2019, section 3.2).  Part of the C ABI of libqttt_hip.so (additive
 * entries of QTTT_ABI_VERSION 6; included by qttt.h after qttt_selfplay_value.h; the buffer layout, conventions and error
 * order of qttt_tree.h, the in-flight invariant of qttt_tree_leaves.h and the record's buffers of qttt_selfplay.h and
 * qttt_selfplay_stream.h hold here).
 *
 * At small budgets Dirichlet noise at a PUCT root (qttt_tree_explore.h) has two defects: an action that the noise lifts
 * gets one visit, looks bad once and is never looked at again; and the visits that the noise did cause stay in the policy
 * target.  Forced playouts give every visited root action about sqrt(k P S) visits; pruning takes out of the recorded
 * target the visits that PUCT alone would not have made.  Both rules are +, *, /, comparisons and the correctly rounded
 * f64 sqrt of qttt_tree.h's score: no exp, no log.  All arithmetic below is IEEE double without contraction, in the
 * order written.
 *
 * A searched move is what it was under qttt_tree_leaves.h with qttt_tree_select_batch_forced in the place of
 * qttt_tree_select_batch: [one plain rollout where the root has no priors yet] [-> qttt_tree_root_noise] -> rounds of
 * { qttt_tree_select_batch_forced -> qttt_evaluate on the games * K leaves -> qttt_tree_backup_batch }.  The backups are
 * the existing ones, unchanged: qttt_tree_backup_batch, qttt_tree_backup_batch_exact, qttt_tree_solve_leaves,
 * qttt_tree_prove.
 *
 * ---- Forced.  For a root with priors P (what qttt_tree_root gives as P: the network's or the uniform priors, after any
 * noise), slots (W, N) and a factor k >= 0, a legal action a is FORCED iff
 *     n(a) > 0  and  (double)n(a) * (double)n(a) < (k * P(a)) * (double)S
 * where n(a) = the slot's visit count with the visits in flight added (bits 24-31 of the N word, qttt_tree_leaves.h) and
 * S = the sum of n over the 36 slots.  There is no square root in it.  n * n == (k P) S exactly is NOT forced.
 *
 * ---- Select.  qttt_tree_select_batch_forced is qttt_tree_select_batch with one difference.  At depth 0 of every descent,
 * if any legal action of the root is forced, the descent takes the forced action of largest ordinary in-flight score (the
 * score of qttt_tree_leaves.h, ties to the lowest action); if none is forced the ordinary score decides among all legal
 * actions.  A root without priors ends the descent before any rule is asked, so does a terminal root, and with k = 0
 * nothing is ever forced: the launch then leaves the bytes that qttt_tree_select_batch leaves.  Below the root nothing
 * changes.  The rule stores nothing.
 *
 * ---- Prune (the record only).  All statistics are those at record time, so nothing is in flight: N is the slot's N word,
 * S the sum of N over the legal actions, Ntot the root's word, P = 0 at a root without priors.
 *   c* = the legal action with the most visits, ties to the lowest action.
 *   score(c*) = qttt_tree.h's score of c*: q + c_puct * ((P(c*) * sqrt(Ntot)) / (1 + N(c*))), q = W / N or 0 where N = 0.
 *   For every other legal action c with N(c) > 0:
 *     F(c) = the smallest integer F >= 0 with (double)F * (double)F >= (k * P(c)) * (double)S;
 *     d(c) = the largest d in [0, min(N(c), F(c))] such that d = 0 or
 *            Q(c) + c_puct * ((P(c) * sqrt(Ntot)) / (double)(1 + (N(c) - d))) < score(c*),   Q(c) = W(c) / N(c) held fixed;
 *     N'(c) = N(c) - d(c), and N'(c) = 0 if d(c) > 0 and N(c) - d(c) <= 1.
 *   N'(c*) = N(c*); N'(c) = N(c) = 0 for an unvisited action.  A product (k P) S that is not a number prunes nothing.
 *   The left side does not fall as d grows when c_puct >= 0 (every operation in it is monotone under IEEE rounding), so the
 *   d that satisfy the inequality are 1 .. d(c) and the device finds d(c) by bisection, at most 24 steps; for c_puct < 0 the
 *   left side does not rise, and d(c) is min(N, F) or 0.  tests/forced_model.py scans every d.
 *   The recorded row is pi = (N' / n_rollouts) ** alpha over the legal actions, normalised as qttt_selfplay.h normalises
 *   the plain row.  The move played, v, the mask, done and every other field are qttt_selfplay_record_sampled's: MCTS.choose
 *   and the sampled move read the unpruned N.  sample_plies = 0 plays the plain move.
 *
 * ---- qttt_selfplay_record_pruned / qttt_selfplay_record_stream_pruned: qttt_selfplay_record_sampled and
 * qttt_selfplay_record_stream_sampled (qttt_tree_explore.h, qttt_selfplay_stream.h) with that pi row; they take the same
 * arguments, then forced_k and c_puct.
 *
 * ---- qttt_tree_root_forced (both outputs nullable): forced u8[games, 36] = the predicate of every root as it stands (0 at
 * illegal actions, at a root without priors and at a terminal root), n_pruned i32[games, 36] = N' (N at a root where
 * nothing is pruned, 0 at illegal actions).  One wave per game, reads only.
 *
 * Errors, in qttt_tree.h's order, before any device work.  QTTT_ERR_SIZE: the sizes of the entry this one extends (games,
 * capacity, board_offset, leaves, rollout_idx0, virtual_loss for the select; ply or draw_index, n_rollouts, alpha, the
 * value targets, temperature, sample_plies for the records), then forced_k negative or not finite, and for the records and
 * the root c_puct not finite.  0 with no device work for games == 0.  QTTT_ERR_NULL for a null pointer that the extended
 * entry requires (the tree alone for qttt_tree_root_forced).  QTTT_ERR_ACTION for a tree, paths or states not 16-byte
 * aligned, pi not 8-byte, v or n_pruned not 4-byte aligned. */
#ifndef QTTT_TREE_FORCED_H
#define QTTT_TREE_FORCED_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int qttt_tree_select_batch_forced(void *tree, int64_t games, int64_t capacity, uint64_t seed, uint32_t rollout_idx0,
                                  int leaves, int64_t board_offset, double c_puct, double virtual_loss, void *paths,
                                  void *leaf_state, double forced_k, void *stream);

int qttt_tree_root_forced(const void *tree, int64_t games, int64_t capacity, double forced_k, double c_puct,
                          uint8_t *forced, int32_t *n_pruned, void *stream);

int qttt_selfplay_record_pruned(const void *tree, int64_t games, int64_t capacity, int ply, uint32_t n_rollouts,
                                double alpha, double v_first, double v_second, void *states, double *pi, uint8_t *mask,
                                uint8_t *done, float *v, uint8_t *action36, uint8_t *length, int8_t *winner,
                                uint8_t *actions, uint64_t seed, int64_t board_offset, double temperature,
                                int sample_plies, double forced_k, double c_puct, void *stream);

int qttt_selfplay_record_stream_pruned(const void *tree, int64_t games, int64_t capacity, uint32_t n_rollouts, double alpha,
                                       double v_first, double v_second, void *states, double *pi, uint8_t *mask,
                                       uint8_t *done, float *v, uint8_t *action36, uint8_t *length, int8_t *winner,
                                       uint8_t *actions, uint64_t seed, int64_t board_offset, double temperature,
                                       int sample_plies, uint32_t draw_index, double forced_k, double c_puct, void *stream);

#ifdef __cplusplus
}
#endif
#endif
