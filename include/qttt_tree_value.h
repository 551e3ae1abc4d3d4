/* qttt_tree_value.h — the value rollout of the device search trees of qttt_tree.h: the leaf is scored by the network's
 * value head instead of by playouts.  Part of the C ABI of libqttt_hip.so (an additive entry of
 * QTTT_ABI_VERSION 6; included by qttt.h after qttt_symmetry.h; the buffer layout, conventions and error order of
 * qttt_tree.h and the weight blob and precisions of qttt_nn.h hold here).
 *
 * A value rollout is
 *   qttt_tree_select -> qttt_tree_value_rollout on the leaf buffer
 * two launches with no host synchronisation in between; it stands where qttt_tree_select -> qttt_rollout_policy ->
 * qttt_tree_backup stands in a playout rollout, and every other entry of qttt_tree.h (reset, root, sync, compact) is
 * used as before.  No draw is taken: the only draws of such a search are select's collapse choices, addressed by the
 * rollout index k alone, so k < QTTT_TREE_MAX_ROLLOUTS is the only bound on it.
 *
 * The value rule.  Per game, v is the leaf's value seen by THE PLAYER TO MOVE AT THE LEAF (the meaning of the
 * reference's r_tot / num_simulations, alphazero.py:178).  The recorded path's edges, deepest first, get -v, +v, ...:
 * W += that, N += 1, Ntot += 1, in IEEE doubles without contraction, exactly as qttt_tree_backup does with its v.
 *   leaf not terminal:  v = (double)value, value = the f32 the network's value head gives for the leaf, bit for bit what
 *                       qttt_evaluate gives for leaf_state in the same precision.
 *   leaf terminal:      the network is not consulted.  v is the game's reward from the node's winner flag: True -> +1 if
 *                       the leaf's turn is True and -1 otherwise, False -> the opposite, None -> 0.  This is what playouts
 *                       from a terminal leaf back up.
 * The priors rule.  A leaf that is neither terminal nor has priors gets the network's 36 f32 probs (qttt_evaluate's
 * probs row of the leaf) and the has-priors flag, never the uniform flag.  A leaf that already has priors keeps them; a
 * select that overflowed ends on such a node, which is backed up with its own value like any other leaf.
 * The non-finite rule.  A NaN or infinite value goes into W as it is.  The comparisons of later selects with it then
 * fail the way torch's would (a NaN score is never the maximum); no loop or branch of any kernel depends on it, and
 * the call returns.
 *
 * leaf_value f32[games] and leaf_probs f32[games, 36], both nullable: what the network gave for every game's leaf,
 * terminal leaves included (qttt_evaluate's value and probs rows of leaf_state).
 *
 * Errors, in this order, before any device work: QTTT_ERR_SIZE for games < 0, capacity outside
 * 1..QTTT_TREE_MAX_CAPACITY or a precision that is neither QTTT_NN_F32 nor QTTT_NN_BF16; 0 with no device work for
 * games == 0; QTTT_ERR_NULL for a null tree, leaf_state or weights; QTTT_ERR_ACTION for a tree or weights not 16-byte
 * aligned or leaf_value / leaf_probs not 4-byte aligned. */
#ifndef QTTT_TREE_VALUE_H
#define QTTT_TREE_VALUE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* One launch: evaluates the network `weights` (qttt_nn.h's packed blob of `precision`) on leaf_state, the
 * qttt_state_bytes(games) bytes the last qttt_tree_select wrote, backs the value up along the path that select
 * recorded and gives the leaf its priors, by the rules above. */
int qttt_tree_value_rollout(void *tree, int64_t games, int64_t capacity, const void *leaf_state, const void *weights,
                            int precision, float *leaf_value, float *leaf_probs, void *stream);

#ifdef __cplusplus
}
#endif
#endif
