/* qttt_solve.h — the exact endgame solver: the expectimax value of late positions, of every legal action there, and the
 * size of the tree that proves them.  Part of the C ABI of libqttt_hip.so (an additive entry of
 * QTTT_ABI_VERSION 6; included by qttt.h after qttt_selfplay_stream.h; the packed state, the conventions and the error
 * order of qttt.h hold here).
 *
 * Quantum tic-tac-toe is an expectimax game: the mover maximises and a collapse is a fair coin (the reference's
 * random.choice in qeval.py; the two collapse children of qttt_expand).  A position with few moves left has a small full
 * tree, and qttt_solve enumerates it: no sampling, no pruning, no transposition table.
 *
 * ---- Definitions.  n = the number of moves played (the state's own count; the implicit autofill move is not one).
 *   Leaf.  A position is a leaf when its `terminal` flag is set or its legal mask is empty, both as qttt_node_info reports
 *     them.  Its value is +1 if `winner` is the player to move, -1 if it is the other player, 0 if it is None; the player
 *     to move is the first player iff n is even (`r if leaf.turn else -r`, mcts.py:174).
 *   Action value.  For a legal action a of a non-leaf take the one or two children of qttt_expand:
 *     one child:  Q(a) = 0 - V(child0);     a collapse:  Q(a) = 0 - (V(child0) + V(child1)) / 2.
 *     An action of the legal mask for which the expansion reports 0 children counts as illegal (none exists among the
 *     states this library writes).
 *   Position value.  V = max over the legal a of Q(a); `best` = the lowest action that attains it.
 *   nodes = the number of positions the plain recursion visits, the root included: 1 for a leaf, else 1 + the sum over
 *     the legal actions and their children of the child's nodes.  Transpositions are not merged and nothing is pruned,
 *     so the figure pins the full enumeration and is what a caller budgets with.
 *
 * ---- Exactness.  A collapse makes at least two more squares classical, so a game holds at most four of them, and every
 * value is k / QTTT_SOLVE_DENOMINATOR with an integer k in [-16, 16]: below a collapse node at most three more can
 * follow, the children's values are multiples of 1/8 and half their sum is a multiple of 1/16.  Negation, that halving
 * and max are exact on such numbers in f32 and f64 alike, so there is no tolerance anywhere: value and q are, bit for
 * bit, the f32 casts of a float64 evaluation of the definitions above, in any order of evaluation.  Written as `0 - x`
 * the negation never yields a negative zero, so no output is -0.0.  (The kernel holds 16 V as an integer.)
 *
 * ---- Which boards are solved.  Board i is solved iff it is a leaf or n >= min_ply; status[i] = 0 then.
 *   a solved leaf:      value by the leaf rule, q = -inf everywhere, best = 255, nodes = 1;
 *   a solved non-leaf:  value, q (-inf at illegal actions), best, nodes as defined;
 *   a skipped board:    status = 1, value = NaN, q = NaN everywhere, best = 255, nodes = 0; it costs no enumeration.
 * min_ply lies in QTTT_SOLVE_MIN_PLY..QTTT_SOLVE_MAX_PLY.  Below four moves played one board is 10^9 positions or more,
 * and nothing should start that by accident.  The largest trees seen in uniform play, none of them a bound
 * (tests/golden/make_golden_solve_deep.py): 29 695 353 positions in 96 boards with four moves played (29 796 849 in the
 * benchmark's 256), 1 244 383 in 1 280 boards with five (1 251 779 in the benchmark's 256), 51 268 in 2 000 boards with
 * six.  One launch solves all n boards, one 256-thread workgroup per board: a caller on a shared device bounds a launch's
 * run time by the number of boards it passes (VecEnv.solve's boards_per_launch).
 *
 * ---- qttt_solve(state, n, min_ply, value, q, best, nodes, status, stream).  state: the packed state of n boards
 * (qttt_state_bytes(n) bytes), read only.  Outputs, each nullable: value f32[n], q f32[n, 36], best u8[n], nodes
 * i64[n], status u8[n].
 *
 * Errors, in qttt.h's order, before any device work: QTTT_ERR_SIZE for n < 0 or min_ply outside
 * QTTT_SOLVE_MIN_PLY..QTTT_SOLVE_MAX_PLY; 0 with no device work for n == 0; QTTT_ERR_NULL for a null state;
 * QTTT_ERR_ACTION for a state not 16-byte aligned, value or q not 4-byte aligned, nodes not 8-byte aligned. */
#ifndef QTTT_SOLVE_H
#define QTTT_SOLVE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QTTT_SOLVE_MIN_PLY 4
#define QTTT_SOLVE_MAX_PLY 9
#define QTTT_SOLVE_DENOMINATOR 16

int qttt_solve(const void *state, int64_t n, int min_ply, float *value, float *q, uint8_t *best, int64_t *nodes,
               uint8_t *status, void *stream);

#ifdef __cplusplus
}
#endif
#endif
