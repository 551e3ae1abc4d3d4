/* qttt_selfplay_value.h — search-value targets for self-play: the searched value of every recorded root, and the value
 * targets made of it, MuZero's / KataGo's remedy for a high-variance game outcome.  Part of the C ABI of
 * libqttt_hip.so (additive entries of QTTT_ABI_VERSION 6; included by qttt.h after qttt_train_weighted.h; the staging
 * buffers of qttt_selfplay.h and the conventions of qttt.h hold here: device pointers owned by the caller, work enqueued on
 * `stream`, 0 / hipError_t / negative argument error, and no call waits for the device).
 *
 * The record kernels write one value target, the outcome of the one game (v[i, g] = v0 * (-1)^i).  The search that picked
 * every move held a better estimate of the root's value, and the sync that moves the root throws it away.  The first entry
 * keeps it, in a row field of its own, q f32[QTTT_SELFPLAY_ROWS, games]; the second rewrites v from it.
 *
 * ---- qttt_selfplay_record_value(tree, games, capacity, ply, length, q, v, stream).  One launch, a wavefront per game,
 * BEFORE the ply's record kernel (qttt_selfplay_record* / qttt_selfplay_record_stream*), in the lockstep loop and in the
 * stream alike: it reads length[g] as the record of the ply before left it.  The tree, length and v are read only.
 *   The row:  r = ply for ply >= 0 (lockstep);  r = length[g] for ply < 0 (stream: the row the next stream record writes).
 *   Row (r, g) is WRITTEN iff r < QTTT_SELFPLAY_ROWS and length[g] == r — the games the ply's record kernel looks at; a
 *   row past a game's end (a finished game riding along in lockstep, from its second ply after the end) is left alone.
 *   With W[a], N[a] the root's statistics as qttt_tree_root returns them (0 at an action that is not legal):
 *     SW = (((+0.0 + W[0]) + W[1]) + ... + W[35]),  SN = N[0] + ... + N[35]     in f64, ascending action order
 *     q[r, g] = (float)(SW / SN)   if SN > 0      — one division in f64, one rounding to f32, a zero stored as +0.0
 *     q[r, g] = v[r, g]            if SN == 0     — the row's own v, bit for bit
 *   The sign is that of qttt_tree_root's Q = W / N, the value for the player to move at the root, which is what
 *   Reanalyser(value_mix) mixes: sum_a N[a] Q[a] / sum_a N[a] = SW / SN.  There is no negation.
 *   SN == 0 is a terminal root (its node is never expanded) and a root that was not searched.  Because the entry runs
 *   before the record, v[r, g] is then what the caller's zero fill left, +0.0: the q of a terminal row carries nothing, and
 *   qttt_selfplay_value_targets never reads it.  The same holds for row length[g] of a finished game riding along.
 *   No output is NaN for finite W, and none is -0.0.
 *   Errors, in qttt.h's order, before any device work: QTTT_ERR_SIZE for games < 0, capacity outside
 *   1..QTTT_TREE_MAX_CAPACITY, ply > QTTT_SELFPLAY_ROWS - 1; 0 with no device work for games == 0; QTTT_ERR_NULL for a null
 *   tree, length, q or v; QTTT_ERR_ACTION for tree not 16-byte aligned, q or v not 4-byte aligned.
 *
 * ---- qttt_selfplay_value_targets(games, mode, lambda, rows, length, done, exact, q, v, stream).  One launch, a lane per
 * game.  Rewrites v f32[10, games] in place for rows t < L[g], L[g] = min(rows ? rows[g] : length[g], 10) (rows u8[games]
 * is nullable: qttt_selfplay_exact_targets' convention, SelfPlay.stream passes the harvested lengths).  exact u8[10, games]
 * is nullable; a row with exact == 1 keeps its v.  rows, length, done, exact and q are read only; rows at or past L[g] keep
 * every byte.  All arithmetic is in f64 without contraction into FMAs, a product is rounded before it is added, a row is
 * rounded to f32 once, negation is 0 - x, and a zero is stored as +0.0.  Every loop is bounded by 10.
 *   mode == QTTT_VALUE_MIX:  for every t < L[g] with done[t, g] == 0 and exact[t, g] != 1
 *       v[t] = (float)((1 - lambda) * v[t] + lambda * q[t])
 *     Reanalyser's rule and Reanalyser's lambda.  lambda == 0 leaves every bit (of a v that holds no -0.0, which no record
 *     and no relabel writes).
 *   mode == QTTT_VALUE_TD:  a backward pass down the game, g a f64 carried from row to row:
 *       g[L-1] = v[L-1]                                   (the terminal row's outcome, or v of the last row looked at)
 *       for t = L-2 .. 0:   b = v[t+1] if exact[t+1, g] == 1 or done[t+1, g] != 0, else q[t+1]
 *                           g[t] = 0 - ((1 - lambda) * b + lambda * g[t+1])
 *                           if exact[t, g] == 1:  g[t] = v[t], the row keeps its v and the recursion restarts from the truth
 *                           else:                 v[t] = (float)g[t]
 *     The mover alternates on every row, hence the negation, as in the record's own v0 * (-1)^i.  lambda == 1 is the game's
 *     outcome: 0 * b + g = g exactly, so every v keeps every bit of what the record wrote; lambda == 0 is the one-step
 *     target -b.  Row L-1 is never written.
 *   Errors, in qttt.h's order, before any device work: QTTT_ERR_SIZE for games < 0, a mode that is neither, lambda outside
 *   [0, 1] or not finite; 0 with no device work for games == 0; QTTT_ERR_NULL for a null length, done, q or v;
 *   QTTT_ERR_ACTION for q or v not 4-byte aligned. */
#ifndef QTTT_SELFPLAY_VALUE_H
#define QTTT_SELFPLAY_VALUE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QTTT_VALUE_MIX 0           /* v = (1 - lambda) v + lambda q, row by row */
#define QTTT_VALUE_TD  1           /* the TD(lambda) return of the rest of the game */

int qttt_selfplay_record_value(const void *tree, int64_t games, int64_t capacity, int ply, const uint8_t *length, float *q,
                               const float *v, void *stream);

int qttt_selfplay_value_targets(int64_t games, int mode, double lambda, const uint8_t *rows, const uint8_t *length,
                                const uint8_t *done, const uint8_t *exact, const float *q, float *v, void *stream);

#ifdef __cplusplus
}
#endif
#endif
