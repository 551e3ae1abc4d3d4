/* qttt_tree_prove.h — proven interior nodes in the device search trees of qttt_tree.h (MCTS-Solver): a node every one of
 * whose legal actions leads to terminal or solved children is itself solved, with the solver's own formula, and from then
 * on behaves like an exact leaf of qttt_tree_exact.h.  Part of the C ABI of libqttt_hip.so (additive
 * entries of QTTT_ABI_VERSION 6; included by qttt.h after qttt_tree_exact.h; the buffer layout and conventions of
 * qttt_tree.h, the round, the path records and the error order of qttt_tree_leaves.h, the node state of qttt_tree_exact.h
 * and the definitions of qttt_solve.h hold here).
 *
 * ---- A round that proves is
 *   qttt_tree_select_batch (or _gumbel) -> qttt_evaluate -> qttt_tree_solve_leaves -> qttt_tree_backup_batch_exact
 *   -> qttt_tree_prove
 * five launches with no host synchronisation in between.  qttt_tree_prove runs after the backup, when no visit is in
 * flight, on the path records that the round's select wrote.
 *
 * ---- qttt_tree_prove(tree, games, capacity, leaves, paths, proved, stream).  One launch; no counter is read back.
 * For game g the round's records j = 0 .. leaves - 1 are taken in order.  A record that fails the pool check of
 * qttt_tree_backup_batch (its depth, leaf, and the nodes and actions of its first `depth` edges lie in the pool) is
 * SKIPPED, and so is a record of depth 0.  Any other record of depth D is WALKED upwards: d = D - 1 down to 0 over
 * x = node[d], the nodes its descent passed through, the game's root last.
 *   x is PROVABLE iff all of these hold:
 *     x is not terminal;  its legal mask is not empty;  the child word of every legal action a is expanded (>= 0);
 *     every child of that action (one, or two where bit 30 of the child word says collapse) is terminal or has the solved
 *     bit (bit 4 of qttt_tree_exact.h).
 *   If x is not provable the walk of this record ENDS there.  If it is, in integer sixteenths
 *     16 Q(a) = -16 V(c0)  for one child,  -(16 V(c0) + 16 V(c1)) / 2  for a collapse
 *               (the sum is even: qttt_solve.h's exactness paragraph — below a collapse at most three more can follow, so
 *               both children's values are multiples of 1/8);
 *     16 V(c) = the stored field (bits 16-21) minus 16 for a solved child,  16 * the terminal value of qttt_tree_value.h
 *               for a terminal child (the value for the player to move at c: -16, 0 or 16; a terminal child is read as
 *               terminal whatever else its flags say);
 *     16 V(x) = the maximum over the legal a of 16 Q(a),
 *   which is qttt_solve's definition of V(x) given its children's, and x's flags receive
 *     QTTT_TREE_NODE_SOLVED | (16 V + 16) << QTTT_TREE_NODE_VALUE_SHIFT;
 *   if d >= 1, bits 0 and 1 (has priors, uniform priors) are CLEARED as well.  The game's root (d = 0) keeps its priors
 *   and is searched on as before.  The walk continues at d - 1.  A node that is solved already is re-derived and stored
 *   again, with the same bits (V is a function of the position alone), and the walk continues: a sibling may have been
 *   solved since, so its ancestors still have to be looked at.
 * Every position's value is a multiple of 1 / QTTT_SOLVE_DENOMINATOR at any number of moves played (a game holds at most
 * four collapses; that argument of qttt_solve.h does not depend on min_ply), so the six value bits always suffice.
 * UNTOUCHED: every child word, every W, N and Ntot, every priors row; the path records are read only.
 * proved (i32[games], nullable) receives the number of nodes of game g whose solved bit this launch set for the first
 * time.  A second launch on the same records stores the same bytes and reports 0 everywhere.
 *
 * ---- Consequence.  A proven node below the root is solved, not terminal, and has no priors.  Every later
 * qttt_tree_select* therefore stops on it (the descent ends at a node without priors), its subtree is never visited
 * again, and qttt_tree_backup_batch_exact backs the record up with the node's stored value and gives it no priors — at
 * any number of moves played; those two kernels are not changed.  qttt_tree_solve_leaves does NOT treat such a record as
 * eligible when its board has fewer than min_ply moves played: it leaves leaf_value[r] alone and sets leaf_exact[r] = 0
 * (the backup does not read that row: it reads the node).  A proven node that qttt_tree_sync makes the root gets priors
 * from its first record of depth 0, as qttt_tree_exact.h says of a solved leaf, and goes on with its old slots and
 * children.  qttt_tree_sync and qttt_tree_compact move the flags unchanged; the children of a proven node stay reachable
 * and are kept by a compaction.  Without exact leaves (qttt_tree_backup_batch) a proven node would be handed its priors
 * back: the entry belongs to rounds of qttt_tree_exact.h alone.
 *
 * ---- qttt_tree_root_exact(tree, games, capacity, q, proven, value, solved, stream): what the proofs say of the roots.
 * Read only; one launch; every output is nullable.
 *   proven[g, a] (u8[games, 36]) = 1 iff a is legal at the root, its child word is expanded, and all its children are
 *                 terminal or solved; else 0.
 *   q[g, a]      (f32[games, 36]) = Q(a) as above, exact in f32, written as 0 - x so that it is never -0.0; NaN where
 *                 proven[g, a] is 0.
 *   solved[g]    (u8[games]) = the root's solved bit.
 *   value[g]     (f32[games]) = the root's stored value (stored - 16) / 16, NaN where solved[g] is 0.
 * A root with every legal action proven was proven by the round that completed it, so its value is the maximum of its q
 * and the lowest action attaining it is the solver's best move.
 *
 * Errors, in qttt_tree_leaves.h's order, before any device work: QTTT_ERR_SIZE for games < 0, capacity outside
 * 1..QTTT_TREE_MAX_CAPACITY, leaves outside 1..QTTT_TREE_MAX_LEAVES (qttt_tree_prove); 0 with no device work for
 * games == 0; QTTT_ERR_NULL for a null tree, or null paths (qttt_tree_prove); QTTT_ERR_ACTION for a tree or paths not
 * 16-byte aligned, proved, q or value not 4-byte aligned. */
#ifndef QTTT_TREE_PROVE_H
#define QTTT_TREE_PROVE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int qttt_tree_prove(void *tree, int64_t games, int64_t capacity, int leaves, const void *paths, int32_t *proved,
                    void *stream);

int qttt_tree_root_exact(const void *tree, int64_t games, int64_t capacity, float *q, uint8_t *proven, float *value,
                         uint8_t *solved, void *stream);

#ifdef __cplusplus
}
#endif
#endif
