/* qttt_tree_exact.h — exact leaves in the device search trees of qttt_tree.h: a leaf with enough moves played is solved on
 * the device, once, and backed up with its exact expectimax value instead of the network's.  Part of the
 * C ABI of libqttt_hip.so (additive entries of QTTT_ABI_VERSION 6; included by qttt.h after qttt_solve.h; the buffer
 * layout and conventions of qttt_tree.h, the round, the path records and the error order of qttt_tree_leaves.h and the
 * definitions of qttt_solve.h hold here).
 *
 * ---- Node state.  Two additions to the u32 flags of a node's header (qttt_tree.h uses bits 0-3 and 8-9):
 *   bit 4        solved: the node's position was enumerated in full and bits 16-21 hold its value;
 *   bits 16-21   16 V + 16, an integer in 0..32: V = the position's exact value for the player to move there, as
 *                qttt_solve defines it (a multiple of 1 / QTTT_SOLVE_DENOMINATOR in [-1, 1]).  0 while bit 4 is clear.
 * qttt_tree_sync and qttt_tree_compact move the flags unchanged; a fresh node has neither.  A solved node is a
 * generalised terminal node: it carries a value in sixteenths where a terminal node carries a winner.  It never receives
 * priors while it is below the root, so every later descent ends on it (the descent of qttt_tree_select stops at a node
 * without priors) and no child of it is ever expanded.  No entry of qttt_tree.h ... qttt_tree_gumbel.h sets or reads the
 * two fields; without the entries below the trees are, byte for byte, what they were.
 *
 * ---- A round with exact leaves is
 *   qttt_tree_select_batch (or _gumbel) -> qttt_evaluate -> qttt_tree_solve_leaves -> qttt_tree_backup_batch_exact
 * four launches with no host synchronisation in between; the in-flight invariant of qttt_tree_leaves.h spans them.
 *
 * ---- qttt_tree_solve_leaves(tree, games, capacity, leaves, paths, leaf_state, min_ply, leaf_value, leaf_exact, stream).
 * One launch; no counter is read back.  paths and leaf_state are what the round's select wrote.  Record (g, j), row
 * r = g * leaves + j, is ELIGIBLE iff all of these hold:
 *   its depth is >= 1;  its depth, leaf, and the nodes and actions of its first `depth` edges lie in the pool (the check
 *   of qttt_tree_backup_batch);  it is not marked overflowed (record flag bit 0);  the leaf node is not terminal and has
 *   no priors (the node's flags);  board r of leaf_state has at least min_ply moves played (qttt_solve.h's n).
 * An eligible leaf whose node is solved costs no enumeration: its stored value is read.  An eligible leaf that is not is
 * enumerated in full by qttt_solve's definition (board r of leaf_state, which is the node's position), and its node
 * receives the solved bit and the value bits; a non-terminal position with an empty legal mask is a leaf of the solver
 * and receives the solver's leaf value in the same way.  For every eligible record leaf_value[r] (f32, nullable) is
 * overwritten with V and leaf_exact[r] (u8, nullable) is set to 1; for every other record leaf_exact[r] is set to 0 and
 * leaf_value[r] is not written.  leaf_state and paths are read only.
 *   Two records of one round may name the same node (qttt_tree_leaves.h: two descents may end on the same leaf), in one
 * workgroup or in two.  Each of them that finds the node unsolved enumerates it, and each writes the flags word it read
 * with the solved bit and the value bits added.  That is benign: V is a function of the node's position alone, no other
 * bit of the word changes during the launch, so every writer stores the same 32 bits, with one aligned 32-bit vector
 * store; a record that reads the word after such a store sees a solved node with that same value.  The cost is one
 * redundant enumeration, in the one round that first meets the node.
 *   min_ply lies in QTTT_TREE_EXACT_MIN_PLY..QTTT_SOLVE_MAX_PLY.  At six moves played a position's tree holds under
 * 5 * 10^4 positions, at seven and more at most 2 000; at five one board costs milliseconds, which is no leaf evaluation.
 *
 * ---- qttt_tree_backup_batch_exact: the arguments and the rule of qttt_tree_backup_batch with two changes, applied to a
 * record of depth >= 1 whose leaf node has the solved bit, is not terminal and has no priors:
 *   v_j = (double)(stored - 16) / 16, not leaf_value[r];   the leaf gets NO priors and no has-priors flag.
 * Every other record is backed up by qttt_tree_backup_batch's rule, bit for bit; a record of depth 0 among them: a root
 * that was solved while it was a leaf gets its priors and is searched like any root (its value bits stay, unused).
 * Sums of sixteenths are exact in f64 far beyond QTTT_TREE_MAX_ROLLOUTS terms, so W of an edge that only solved leaves
 * were backed up through is exact.
 *
 * Errors, in qttt_tree_leaves.h's order, before any device work: QTTT_ERR_SIZE for games < 0, capacity outside
 * 1..QTTT_TREE_MAX_CAPACITY, leaves outside 1..QTTT_TREE_MAX_LEAVES, min_ply outside
 * QTTT_TREE_EXACT_MIN_PLY..QTTT_SOLVE_MAX_PLY; 0 with no device work for games == 0; QTTT_ERR_NULL for a null tree, paths
 * or leaf_state (solve_leaves), a null tree, paths, leaf_value or leaf_probs (backup_batch_exact); QTTT_ERR_ACTION for a
 * tree, paths or leaf_state not 16-byte aligned, leaf_value / leaf_probs not 4-byte aligned. */
#ifndef QTTT_TREE_EXACT_H
#define QTTT_TREE_EXACT_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QTTT_TREE_EXACT_MIN_PLY 6
#define QTTT_TREE_NODE_SOLVED (1u << 4)
#define QTTT_TREE_NODE_VALUE_SHIFT 16
#define QTTT_TREE_NODE_VALUE_MASK (63u << QTTT_TREE_NODE_VALUE_SHIFT)

int qttt_tree_solve_leaves(void *tree, int64_t games, int64_t capacity, int leaves, const void *paths,
                           const void *leaf_state, int min_ply, float *leaf_value, uint8_t *leaf_exact, void *stream);

int qttt_tree_backup_batch_exact(void *tree, int64_t games, int64_t capacity, int leaves, const void *paths,
                                 const float *leaf_value, const float *leaf_probs, void *stream);

#ifdef __cplusplus
}
#endif
#endif
