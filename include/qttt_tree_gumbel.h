/* qttt_tree_gumbel.h — the Gumbel root of the device search trees of qttt_tree.h: the actions to consider are sampled
 * without replacement with Gumbel noise, the budget is spent on them by sequential halving, and the move and the policy
 * target come from the completed Q values ("Policy improvement by planning with Gumbel", Danihelka et al., ICLR 2022;
 * DESIGN.md §19).  Part of the C ABI of libqttt_hip.so (additive entries of QTTT_ABI_VERSION 6; included by qttt.h after
 * qttt_tree_leaves.h; the buffer layout, conventions and error order of qttt_tree.h, the in-flight invariant of
 * qttt_tree_leaves.h and the record's buffers of qttt_selfplay.h hold here).
 *
 * A searched move of n simulations with K = `leaves` per round is
 *   [one plain rollout where the root has no priors yet] -> qttt_tree_root_states -> qttt_evaluate(value, logits)
 *   -> qttt_tree_gumbel_begin -> rounds of { qttt_tree_select_batch_gumbel -> qttt_evaluate on the games * K leaves
 *   -> qttt_tree_backup_batch } with sim_idx0 = 0, K, 2 K, ... -> qttt_tree_gumbel_root or qttt_selfplay_record_gumbel
 * with no host synchronisation in between.  Only the rule at the ROOT differs from the leaf-parallel search: below the
 * root the in-flight PUCT score of qttt_tree_leaves.h holds unchanged, and so do the expansion, the overflow rule, the
 * depth bound, the path records and the backup.  The paper's non-root rule is not built.  Q is not rescaled: values here
 * lie in [-1, 1] already.
 *
 * ---- The record.  `rec` is the caller's buffer of qttt_tree_gumbel_bytes(games) bytes, 16-byte aligned: one record of
 * QTTT_TREE_GUMBEL_BYTES per game, little-endian, byte offsets:
 *   f64 gumbel[36] at 0 | f64 prior[36] at 288 | f32 logits[36] at 576 | u32 n0[36] at 720 | u64 considered at 864
 *   | f32 root_value at 872 | u32 m_eff at 876.
 * qttt_tree_gumbel_begin writes every byte of it.  gumbel, prior and n0 are 0 at illegal actions; logits holds the
 * caller's row as it is (-inf at illegal actions from qttt_evaluate).
 *
 * ---- The visit sequence (host only).  qttt_gumbel_visit_sequence(m, n_sims, out) writes n = n_sims entries: for m >= 2,
 * with L = ceil(log2 m), visits[0..m) = 0 and c = m:  while fewer than n entries have been emitted { e = max(1,
 * floor(n / (L * c))); e times { append visits[0..c); visits[i] += 1 for i < c }; c = max(2, c / 2) }, truncated to n
 * entries.  For m <= 1 the sequence is 0, 1, .., n - 1.  Entry i is the number of visits the action of simulation i must
 * have had since begin.  The caller builds the table i32[37, n_sims], row m = the sequence of m considered actions, once
 * per budget and keeps it on the device.  QTTT_ERR_SIZE for m outside 0..36 or n_sims outside 1..QTTT_TREE_MAX_ROLLOUTS,
 * QTTT_ERR_NULL for a null out.
 *
 * ---- qttt_tree_root_states: the roots' packed states (qttt_state_bytes(games) bytes), so that qttt_evaluate gives the
 * roots' value and masked logits.
 *
 * ---- qttt_tree_gumbel_begin.  One wave per game, a lane per action.  A root is LIVE when it is not terminal and has a
 * legal action.  Per live root and legal action a, in IEEE doubles without contraction:
 *   u = U53(qttt_hash(seed, board_offset + g, QTTT_TREE_GUMBEL_BASE + move_idx * 36 + a)), the uniform of
 *     qttt_tree_explore.h, strictly inside (0, 1); move_idx < QTTT_TREE_MAX_GUMBEL (the caller counts its calls since
 *     qttt_tree_reset), and the indices collide with no other draw: they lie above QTTT_SELFPLAY_MOVE_BASE + 10.
 *   gumbel[a] = -log(-log(u))   (the device library's log, an ulp or so from the exact one),
 *   s0(a) = gumbel[a] + (double)logits[a],
 *   prior[a] = exp((double)logits[a] - mx) / Z, mx = the largest (double)logits over the legal actions, Z = the sum of
 *     the 36 exp terms (0 at illegal actions) as qttt_selfplay.h takes sums (64 terms, s[i] += s[i ^ m], m = 1 .. 32).
 *     It is stored so that every later rule is +, *, / on stored numbers: no later kernel calls exp for it.
 *   m_eff = min(max_considered, popcount(legal)); considered = the m_eff legal actions of largest s0, ties to the lowest
 *     action: a is considered when fewer than m_eff legal b have s0(b) > s0(a) or (s0(b) == s0(a) and b < a).
 *   n0[a] = the low 24 bits of the root's N word: a subtree reused after qttt_tree_sync has visits already.
 *   root_value = root_value[g], the network's value of the root seen by the player to move there (the view of the
 *     root's W, qttt_tree_value.h).
 * A root that is not live gets m_eff = 0, considered = 0 and zero gumbel and prior rows.
 *
 * ---- Completed Q and sigma, of a root with the record, in IEEE doubles without contraction, in exactly this order.
 * n(a) = the low 24 bits of the root's N word, f(a) = its bits 24-31 (in flight, qttt_tree_leaves.h), over legal a:
 *   q(a) = W(a) / n(a) where n(a) > 0;  S = sum_b n(b) and N_max = max_b n(b) as integers;
 *   A = sum over {b: n(b) > 0} of prior[b] * q(b),  B = sum over the same b of prior[b], both as qttt_selfplay.h sums;
 *   v_mix = S == 0 ? root_value : (root_value + (S * A) / B) / (1 + S);
 *   q^(a) = n(a) ? q(a) : v_mix;     sigma(q) = ((c_visit + N_max) * c_scale) * q.
 * In-flight visits do not enter q^; W is never perturbed.
 *
 * ---- qttt_tree_select_batch_gumbel: qttt_tree_select_batch with one difference.  At the root, for descent j of a game
 * with m_eff > 0: c = visit_table[m_eff * n_sims + sim_idx0 + j]; the action is the argmax of s0(a) + sigma(q^(a)) over
 * the considered a with (n(a) - n0[a]) + f(a) == c, ties to the lowest action; if no considered action matches, the same
 * argmax over all considered actions.  m_eff == 0 (or a record whose m_eff is not in 0..36): the ordinary rule.
 * visit_table: i32[37, n_sims] on the device.
 *
 * ---- qttt_tree_gumbel_root (every output nullable): choose u8[games] = the argmax of s0 + sigma(q^) over the considered
 * actions whose n - n0 is the largest among the considered, ties to the lowest; 255 where nothing is considered (no legal
 * action, a terminal root).  q_completed f64[games, 36] = q^ on the legal actions, 0 elsewhere.  pi f64[games, 36] = the
 * improved policy: x(a) = (double)logits[a] + sigma(q^(a)), pi(a) = exp(x(a) - max x) / (the sum of those 36 terms as
 * qttt_selfplay.h sums) on the legal actions, 0 elsewhere.
 *
 * ---- qttt_selfplay_record_gumbel: qttt_selfplay_record (every buffer, field and rule, qttt_selfplay.h) except that at a
 * live root the move is `choose` above and the pi row the improved policy above.  n_rollouts and alpha are ignored.
 *
 * Errors, in qttt_tree.h's order, before any device work.  QTTT_ERR_SIZE: the sizes of the entry this one extends
 * (games, capacity, board_offset, leaves, rollout_idx0, virtual_loss; ply and the value targets for the record), then
 * max_considered outside 1..36, move_idx >= QTTT_TREE_MAX_GUMBEL, n_sims < 1 or sim_idx0 + leaves > n_sims, c_visit
 * negative or not finite, c_scale not finite.  0 with no device work for games == 0.  QTTT_ERR_NULL for a null tree,
 * rec, visit_table, state, root_value, root_logits or any pointer the extended entry requires.  QTTT_ERR_ACTION for a
 * tree, rec or paths not 16-byte aligned, pi / q_completed not 8-byte, visit_table / root_value / root_logits not 4-byte
 * aligned. */
#ifndef QTTT_TREE_GUMBEL_H
#define QTTT_TREE_GUMBEL_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QTTT_TREE_GUMBEL_BYTES 880
#define QTTT_TREE_GUMBEL_BASE 0xF0000000u
#define QTTT_TREE_MAX_GUMBEL (0x10000000u / 36u)      /* move_idx values whose draw indices stay below 2^32 */

/* Bytes of the per-game Gumbel records (host-only); QTTT_ERR_SIZE for games < 0. */
int64_t qttt_tree_gumbel_bytes(int64_t games);

/* The visit sequence above for m considered actions and a budget of n_sims (host-only). */
int qttt_gumbel_visit_sequence(int m, int n_sims, int32_t *out);

int qttt_tree_root_states(const void *tree, int64_t games, int64_t capacity, void *state_out, void *stream);

int qttt_tree_gumbel_begin(const void *tree, int64_t games, int64_t capacity, uint64_t seed, uint32_t move_idx,
                           int64_t board_offset, int max_considered, const float *root_value, const float *root_logits,
                           void *rec, void *stream);

int qttt_tree_select_batch_gumbel(void *tree, int64_t games, int64_t capacity, uint64_t seed, uint32_t rollout_idx0,
                                  int leaves, int64_t board_offset, double c_puct, double virtual_loss, void *paths,
                                  void *leaf_state, const void *rec, const int32_t *visit_table, int n_sims, int sim_idx0,
                                  double c_visit, double c_scale, void *stream);

int qttt_tree_gumbel_root(const void *tree, const void *rec, int64_t games, int64_t capacity, double c_visit,
                          double c_scale, uint8_t *choose, double *pi, double *q_completed, void *stream);

int qttt_selfplay_record_gumbel(const void *tree, int64_t games, int64_t capacity, int ply, uint32_t n_rollouts,
                                double alpha, double v_first, double v_second, void *states, double *pi, uint8_t *mask,
                                uint8_t *done, float *v, uint8_t *action36, uint8_t *length, int8_t *winner,
                                uint8_t *actions, const void *rec, double c_visit, double c_scale, void *stream);

#ifdef __cplusplus
}
#endif
#endif
