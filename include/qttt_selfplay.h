/* qttt_selfplay.h — the self-play record: what turns the device search trees of qttt_tree.h into the trainer's batch
 * of the reference (self_play.py:43-76 play_game, :193-216 the samples), part of the C ABI of libqttt_hip.so (an
 * additive entry of QTTT_ABI_VERSION 6; included by qttt.h after qttt_tree_compact.h, whose conventions hold here:
 * device pointers owned by the caller, work enqueued on `stream`, 0 / hipError_t / negative argument error).
 *
 * A game of self-play is at most 9 moves, so at most QTTT_SELFPLAY_ROWS = 10 roots: the position before every move and
 * the terminal one.  One call records root number `ply` of every game and gives back the move to play:
 *   for ply in 0..9:  rollouts (qttt_tree_select ... qttt_tree_backup) -> qttt_selfplay_record(ply) ->
 *                     qttt_step(actions) -> qttt_tree_sync [-> qttt_tree_compact]
 * with no host synchronisation in between.  The tree is read only.
 *
 * Buffers, all caller-owned device memory, QTTT_SELFPLAY_ROWS rows each, zero-filled by the caller before ply 0 (a row a
 * game never reaches is not written):
 *   states    10 x qttt_state_bytes(games) bytes: row t is a state buffer in its own right (planes P / Q with the plane
 *             stride of `games` boards), holding the roots' packed states
 *   pi        f64[10, games, 36]   the policy target          mask      u8[10, games, 36]  the legal actions
 *   done      u8[10, games]        1 in a game's terminal row v         f32[10, games]     the value target
 *   action36  u8[10, games]        the move played from the row (255: none)
 *   length    u8[games]            rows recorded so far       winner    i8[games]          1 / 0 / -1 = True / False / None
 *   actions   u8[games, 2]         this ply's move as the pair of squares qttt_step takes
 *
 * Game g is LIVE at ply t when t == 0, or when length[g] == t and row t - 1 was not its terminal row (done[t - 1, g]
 * == 0): the call reads back what the call before it wrote, so the plies are recorded in order.  Per game:
 *   not live (its terminal row was recorded earlier): actions[g] = (255, 255), a noop of the step; nothing else is
 *     written.
 *   live, root not terminal: row t gets the root's packed state; mask[a] = the root's legal bit;
 *     pi[a] = x_a / sum_b x_b with x_a = pow((double)N[a] / (double)n_rollouts, alpha) on the legal actions and 0
 *     elsewhere (self_play.py:208-211; alpha == 1.0 takes x_a = N[a] / n_rollouts without the pow); done = 0;
 *     action36[t, g] = MCTS.choose of the root (mcts.py:308-315, as qttt_tree_root's `choose`); actions[g] = that
 *     action's squares, (255, 255) if choose gives 255; length[g] = t + 1.
 *   live, root terminal: row t gets the state; pi = 1 / 36 and mask = 1 at all 36 actions (self_play.py:204-205);
 *     done = 1; action36 = 255; actions[g] = (255, 255); length[g] = t + 1; winner[g] from the root's flags; and the
 *     value targets of the whole game are written: v[i, g] = v0 * (-1)^i for i = 0..t (self_play.py:195-216), v0 =
 *     (float)v_first if the winner is True, (float)v_second if it is False, 0 if there is none.  A zero is stored as
 *     +0.0.
 *
 * The sum.  sum_b x_b is taken over 64 terms, x_0 .. x_35 followed by 28 zeros, as a balanced binary tree of IEEE
 * double additions: s[i] = s[i] + s[i ^ m] for every i, for m = 1, 2, 4, 8, 16, 32 in this order; the sum is s[0]
 * (every s[i] holds the same value at the end: the addition is commutative).  x_a, the sum and the quotient are IEEE
 * doubles, each division correctly rounded; pow is the device library's, a few ulps from the exact power.
 *
 * Two things are the reference's and kept.  A root without a single visit gives NaN on its legal actions (0 / 0,
 * self_play.py:211) and 0 elsewhere.  The reference's own targets are (v_first, v_second) = (1, 0): its `elif winner:`
 * (self_play.py:198) can never fire, so a loss of the first player trains towards 0; (1, -1) is the evident intention.
 *
 * Errors, in this order, before any device work: QTTT_ERR_SIZE for games < 0, capacity outside
 * 1..QTTT_TREE_MAX_CAPACITY, ply outside 0..QTTT_SELFPLAY_ROWS - 1, n_rollouts == 0, alpha, v_first or v_second not
 * finite, alpha <= 0; 0 with no device work for games == 0; QTTT_ERR_NULL for any null buffer; QTTT_ERR_ACTION for
 * tree or states not 16-byte aligned, pi not 8-byte aligned, v not 4-byte aligned. */
#ifndef QTTT_SELFPLAY_H
#define QTTT_SELFPLAY_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QTTT_SELFPLAY_ROWS 10      /* at most 9 moves, so at most 10 roots per game, the terminal one included */

int qttt_selfplay_record(const void *tree, int64_t games, int64_t capacity, int ply, uint32_t n_rollouts, double alpha,
                         double v_first, double v_second, void *states, double *pi, uint8_t *mask, uint8_t *done,
                         float *v, uint8_t *action36, uint8_t *length, int8_t *winner, uint8_t *actions, void *stream);

#ifdef __cplusplus
}
#endif
#endif
