/* qttt_tree_leaves.h — leaf-parallel rounds of the device search trees of qttt_tree.h: K leaves per game per round, kept
 * apart by virtual loss, so that ONE network launch evaluates games * K leaves.  Part of the C ABI of
 * libqttt_hip.so (additive entries of QTTT_ABI_VERSION 6; included by qttt.h after qttt_tree_value.h; the buffer layout,
 * conventions and error order of qttt_tree.h and the value and priors rules of qttt_tree_value.h hold here).
 *
 * A round of K = `leaves` rollouts is
 *   qttt_tree_select_batch -> qttt_evaluate(leaf_state, n = games * K, value + probs) -> qttt_tree_backup_batch
 * three launches with no host synchronisation in between; it stands where K value rollouts (qttt_tree_select ->
 * qttt_tree_value_rollout) stand.  leaf_state is an ordinary state buffer of games * K boards (qttt_state_bytes(games * K)
 * bytes): board g * K + j is the leaf of descent j of game g.  `paths` is the caller's scratch of
 * qttt_tree_paths_bytes(games, K) bytes (16-byte aligned): one record of QTTT_TREE_PATH_BYTES per (g, j), at
 * QTTT_TREE_PATH_BYTES * (g * K + j), little-endian, byte offsets:
 *   i32 leaf (the node the descent ended on) | u8 depth at 4 (its number of edges, 0..10) | u8 flags at 5 (bit 0 this
 *   descent overflowed, bit 1 leaf turn, bit 2 leaf terminal: the bits of the game header's flags) | 2 B padding
 *   | u8 action[10] at 8 | 6 B padding | i32 node[10] at 24: edge d of the path leaves node[d] by action[d].
 *   A select writes leaf, depth, flags and the first `depth` path entries; the padding and the other entries keep what
 *   the caller's buffer held.
 *
 * The in-flight invariant.  N and Ntot stay below 2^24 (QTTT_TREE_MAX_ROLLOUTS).  Between a qttt_tree_select_batch and
 * its qttt_tree_backup_batch, bits 24-31 of a slot's N word hold the number of this round's descents that passed through
 * that edge, and bits 24-31 of a node's Ntot word the same count for the node; after qttt_tree_backup_batch all those bits
 * are zero again.  W is never perturbed.  NO OTHER TREE ENTRY MAY BE CALLED BETWEEN THE TWO: every other entry reads N
 * and Ntot as plain counts.
 *
 * The select rule, per game, for j = 0 .. K-1 in order.  Descent j is qttt_tree_select's descent (the same loop
 * condition, the expansion of both collapse children, the overflow rule, the depth bound of 10) with the collapse bits
 * of rollout index rollout_idx0 + j and the score taken on effective statistics, in IEEE doubles without contraction:
 *   f = N >> 24, n = N & 0xFFFFFF, Ne = n + f, We = W - virtual_loss * (double)f, q = Ne ? We / Ne : 0,
 *   u = P * sqrt((double)Ntot_e) / (1 + Ne) with Ntot_e formed from the Ntot word as Ne from N, score = q + c_puct * u.
 * With f = 0 this is qttt_tree_score bit for bit.  After the descent every edge on its path gets one in-flight visit
 * (N += 1 << 24, and Ntot += 1 << 24 in the edge's node); then record j and leaf row g * K + j are written.  Two
 * descents may end on the same leaf (a fresh child, or a forced line): both are recorded and both are backed up.  The
 * game header's `used` and overflow flag are updated; depth, leaf and the leaf flags are left as qttt_tree_compact leaves
 * them: depth 0, leaf = the root, the root's flags.  The header's path entries are not written.
 *
 * The backup rule, per game, for j ascending.  v_j by the value rule of qttt_tree_value.h: a terminal leaf gives +-1 or 0
 * from the node's winner flag and turn and the network's row is ignored; any other leaf gives (double)leaf_value[g K + j],
 * non-finite values as they are.  The edges of record j, deepest first, get -v, +v, ...: W += that, and the N word and
 * the node's Ntot word get + 1 - (1 << 24).  The priors rule: a leaf that is neither terminal nor has priors gets row
 * g K + j of leaf_probs and the has-priors flag; a leaf that already has priors keeps them, also when an earlier j of
 * this round just gave them to it.  A record whose depth, leaf, nodes or actions do not lie in the pool is skipped.
 *
 * Errors, in qttt_tree.h's order, before any device work: QTTT_ERR_SIZE for games < 0, capacity outside
 * 1..QTTT_TREE_MAX_CAPACITY, board_offset < 0, leaves outside 1..QTTT_TREE_MAX_LEAVES, rollout_idx0 + leaves >
 * QTTT_TREE_MAX_ROLLOUTS, a virtual_loss that is negative or not finite (qttt_tree_paths_bytes returns it for bad games
 * or leaves); 0 with no device work for games == 0; QTTT_ERR_NULL for a null tree, paths, leaf_state, leaf_value or
 * leaf_probs; QTTT_ERR_ACTION for a tree or paths not 16-byte aligned, leaf_value / leaf_probs not 4-byte aligned. */
#ifndef QTTT_TREE_LEAVES_H
#define QTTT_TREE_LEAVES_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QTTT_TREE_MAX_LEAVES 64
#define QTTT_TREE_PATH_BYTES 64

/* Bytes of the path scratch of a round (host-only); QTTT_ERR_SIZE for bad sizes. */
int64_t qttt_tree_paths_bytes(int64_t games, int leaves);

/* `leaves` descents per game by the select rule above: marks their edges in flight, writes the path records and the
 * leaves' packed states to leaf_state (qttt_state_bytes(games * leaves) bytes). */
int qttt_tree_select_batch(void *tree, int64_t games, int64_t capacity, uint64_t seed, uint32_t rollout_idx0,
                           int leaves, int64_t board_offset, double c_puct, double virtual_loss,
                           void *paths, void *leaf_state, void *stream);

/* Backs the round of the last qttt_tree_select_batch up by the backup rule above.  leaf_value f32[games * leaves] and
 * leaf_probs f32[games * leaves, 36]: qttt_evaluate's value and probs rows of that call's leaf_state. */
int qttt_tree_backup_batch(void *tree, int64_t games, int64_t capacity, int leaves, const void *paths,
                           const float *leaf_value, const float *leaf_probs, void *stream);

#ifdef __cplusplus
}
#endif
#endif
