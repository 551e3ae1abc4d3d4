/* qttt_tree.h — batched MCTS / AlphaZero search trees that live on the device, part of the C ABI of libqttt_hip.so (an
 * additive entry of QTTT_ABI_VERSION 6; included by qttt.h, whose conventions hold here: device pointers owned by the
 * caller, work enqueued on `stream`, 0 / hipError_t / negative argument error).
 *
 * One tree per game for `games` independent games, in one caller-owned buffer of qttt_tree_bytes(games, capacity)
 * bytes (16-byte aligned).  A rollout of the reference (MCTS._rollout, mcts.py:166-176; AlphaZero shares the tree code) is
 *   qttt_tree_select -> qttt_rollout_many or qttt_rollout_policy on the leaf buffer -> qttt_tree_backup
 * with no host synchronisation in between.  A move is qttt_tree_root (choose) -> the caller steps its games ->
 * qttt_tree_sync -> (optionally) qttt_tree_compact.
 *
 * Compaction (qttt_tree_compact, declared in qttt_tree_compact.h; the reference's _prune, mcts.py:222-231, 330-337).
 * A sync leaves the nodes outside the new root's subtree allocated; qttt_tree_compact gives them back.  Per game it
 * keeps the nodes reachable from the root in their old relative order, the root at index 0, and sets used to their
 * number.  Nodes come from a bump counter and a node has one parent, so a child's index is larger than its parent's,
 * before and after: one ascending sweep finds the reachable nodes and numbers them in a forwarding table (i32 per
 * node, the caller's scratch buffer of qttt_tree_compact_bytes(games, capacity) bytes), a second moves each record
 * down to its new index (never above its old one) with its child words rewritten; a collapse pair stays adjacent
 * with bit 30 set.  W, N, Ntot, flags and priors move unchanged and no draw is addressed by a node index, so a search
 * that goes on after the call computes bit for bit what it would have computed without it.  The recorded path is
 * cleared as by qttt_tree_reset (depth 0, leaf 0, the leaf flags of the root); the overflow flag keeps its value; the
 * header's padding and path entries are not written.  A game that is compact already (root 0, every node reachable)
 * is left byte for byte as it is.  Records and priors at or beyond the new `used` are unspecified after the call.
 *
 * Buffer layout (all little-endian, byte offsets):
 *   game header g at 128 g, 128 B:  i32 used (nodes allocated) | i32 root | i32 depth (path length of the last select)
 *                                   | i32 leaf | u32 flags (bit 0 overflow, 1 leaf turn, 2 leaf terminal) | 12 B padding
 *                                   | i32 path_node[10] at 32 | u8 path_action[10] at 72 | padding to 128
 *                                   (no entry writes the padding, and a select writes only the first `depth` path
 *                                   entries: those bytes keep what the caller's buffer held)
 *   node i of game g at 128 games + QTTT_TREE_NODE_BYTES (g capacity + i), 608 B:
 *     header 32 B:  u64 P, u64 Q (the packed state, planes P / Q of the state layout) | u64 legal (bit a = action a)
 *                   | u32 Ntot | u32 flags (bit 0 has priors, 1 uniform priors, 2 terminal, 3 turn (True = the first
 *                   player to move), bits 8-9 winner + 1: 0 None, 1 False, 2 True)
 *                   (bit 4 and bits 16-21, the exact leaves' solved flag and value: qttt_tree_exact.h; set for proven
 *                   interior nodes too: qttt_tree_prove.h)
 *     36 action slots of 16 B at 32 + 16 a:  f64 W | u32 N | i32 child (-1 = not expanded; else bits [0,30) = the
 *                   index of child 0 and bit 30 = a collapse, whose child 1 sits at index + 1)
 *   priors of node i of game g at 128 games + QTTT_TREE_NODE_BYTES games capacity + 144 (g capacity + i): f32[36], the
 *     network's probs; read only when the node's flags say it has non-uniform priors.  Uniform priors (MCTS,
 *     mcts.py:287-289) are 1 / popcount(legal) as a double, a function of the node.
 *
 * Draws.  k = the rollout index since qttt_tree_reset (the caller counts it).  Rollout k's playouts use step_idx0 =
 * k * n_sims * QTTT_SIM_STRIDE; its collapse choice at path depth d (the d-th edge from the root) is bit d of
 * qttt_hash(seed, board_offset + g, QTTT_TREE_SELECT_BASE + k): the child index in qttt_expand's order (child 0 = the
 * closing move lands on the lower square).  Playout step indices stay below QTTT_TREE_SELECT_BASE, and Ntot below
 * QTTT_TREE_MAX_ROLLOUTS, so k < QTTT_TREE_MAX_ROLLOUTS and (k + 1) * n_sims * QTTT_SIM_STRIDE <= QTTT_TREE_SELECT_BASE.
 *
 * Exactness: W, Q and the selection score are IEEE doubles in the reference's order of operations, without
 * contraction: score = Q + c_puct * ((P * sqrt(Ntot)) / (1 + N)), Q = W / N (0 while N = 0), argmax over the legal
 * actions with ties to the lowest action.  qttt_tree_sqrt exports the select kernel's sqrt(Ntot) and
 * qttt_tree_score its score.
 *
 * Errors, in this order, before any device work: QTTT_ERR_SIZE for games < 0, capacity outside
 * 1..QTTT_TREE_MAX_CAPACITY (qttt_tree_bytes returns it too), board_offset < 0, rollout_idx >= QTTT_TREE_MAX_ROLLOUTS,
 * n_sims outside 1..QTTT_TREE_MAX_SIMS; 0 with no device work for games == 0; QTTT_ERR_NULL for a null tree, state,
 * leaf_state, result
 * or scratch; QTTT_ERR_ACTION for a tree not 16-byte aligned, leaf_probs / N / Ntot / nodes_used not 4-byte
 * aligned or W / Q / P not 8-byte aligned, the scratch of qttt_tree_compact not 4-byte aligned. */
#ifndef QTTT_TREE_H
#define QTTT_TREE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QTTT_TREE_GAME_BYTES 128
#define QTTT_TREE_NODE_BYTES 608
#define QTTT_TREE_PRIOR_BYTES 144
#define QTTT_TREE_MAX_DEPTH 10
#define QTTT_TREE_MAX_CAPACITY (1 << 30)
#define QTTT_TREE_MAX_SIMS 128
#define QTTT_TREE_MAX_ROLLOUTS (1u << 24)
#define QTTT_TREE_SELECT_BASE 0x80000000u

/* Bytes of a tree buffer (host-only); QTTT_ERR_SIZE for bad sizes. */
int64_t qttt_tree_bytes(int64_t games, int64_t capacity);

/* MCTS.reset (mcts.py:139-164) of every game: the root is node 0, holding the packed state of board g of `state`
 * (qttt_state_bytes(games) bytes) — its full state, open entanglements included; turn = the number of moves is even. */
int qttt_tree_reset(void *tree, int64_t games, int64_t capacity, const void *state, void *stream);

/* _select (mcts.py:269-285) with _expand_child (:210-221) for rollout `rollout_idx`: descends from the root while the
 * node has priors and is not terminal, expands the chosen action on first visit (1 node, 2 on a collapse), records the
 * path in the game header and writes the leaf's packed state to leaf_state (qttt_state_bytes(games) bytes).  An
 * expansion that does not fit `capacity` sets the game's overflow flag and ends the select at the current node. */
int qttt_tree_select(void *tree, int64_t games, int64_t capacity, uint64_t seed, uint32_t rollout_idx,
                     int64_t board_offset, double c_puct, void *leaf_state, void *stream);

/* _backpropogate (mcts.py:175-183) of the last select, and the leaf's priors (_simulate :188-191).  result
 * i8[games, n_sims] = the playouts' rewards (qttt_rollout_many / qttt_rollout_policy on leaf_state); the value is
 * v = (sum of result, negated when the leaf's turn is False) / n_sims, and the path's edges, deepest first, get
 * -v, +v, ...  leaf_probs f32[games, 36] nullable: null = uniform priors (MCTS), else the leaf's network probs. */
int qttt_tree_backup(void *tree, int64_t games, int64_t capacity, const int8_t *result, int n_sims,
                     const float *leaf_probs, void *stream);

/* MCTS.sync (mcts.py:317-337): re-roots game g onto the root child whose packed state equals board g of `state`,
 * keeping its subtree; a fresh root (1 node, turn = not the old root's) when no expanded child matches; nothing
 * when the position equals the root's. */
int qttt_tree_sync(void *tree, int64_t games, int64_t capacity, const void *state, void *stream);

/* The roots' statistics, every output nullable: N i32[games, 36], W, Q, P f64[games, 36] (0 at illegal actions; P 0
 * while the root has no priors), Ntot i32[games], choose u8[games] (MCTS.choose, mcts.py:308-315: the legal action
 * with the largest Q among those with N > 0, lowest on ties; the lowest legal action if none was visited; 255 if
 * none is legal), nodes_used i32[games], overflow u8[games]. */
int qttt_tree_root(const void *tree, int64_t games, int64_t capacity, int32_t *N, double *W, double *Q, double *P,
                   int32_t *Ntot, uint8_t *choose, int32_t *nodes_used, uint8_t *overflow, void *stream);

/* out[i] = the select kernel's sqrt((double)(first + i)), i < n (so that its rounding can be checked). */
int qttt_tree_sqrt(uint32_t first, int64_t n, double *out, void *stream);

/* out[i] = the select kernel's score of an action with statistics W[i], N[i], prior[i] in a node with Ntot[i] visits,
 * i < n (so that its order of operations can be checked bit for bit).  Errors as qttt_tree_sqrt: QTTT_ERR_SIZE for
 * n < 0; 0 for n == 0; QTTT_ERR_NULL for a null array; QTTT_ERR_ACTION for W / prior / out not 8-byte or N / Ntot not
 * 4-byte aligned. */
int qttt_tree_score(const double *W, const uint32_t *N, const double *prior, const uint32_t *Ntot, double c_puct,
                    int64_t n, double *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif
