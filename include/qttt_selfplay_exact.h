/* qttt_selfplay_exact.h — exact value and policy targets for the late rows of a self-play batch: a recorded position with
 * enough moves played is enumerated in full on the device and its row of the trainer's batch is relabelled with the truth
 * (DESIGN.md §25).  Part of the C ABI of libqttt_hip.so (an additive entry of QTTT_ABI_VERSION 6; included by qttt.h after
 * qttt_tree_exact.h; the staging buffers of qttt_selfplay.h, the definitions of qttt_solve.h and the conventions of
 * qttt.h hold here: device pointers owned by the caller, work enqueued on `stream`, 0 / hipError_t / negative argument
 * error, and the call does not wait for the device).
 *
 * What the record leaves in row t of a game is the outcome of that one game (v) and the visit counts of a search guided by
 * the network being trained (pi).  Late in the game the truth is a few thousand positions away.  One launch replaces both
 * where the position is late enough; every other byte stays.
 *
 * ---- qttt_selfplay_exact_targets(states, games, min_ply, policy, rows, length, done, mask, pi, v, exact, stream).
 * The buffers are qttt_selfplay.h's, QTTT_SELFPLAY_ROWS = 10 rows each, every row of `states` a state buffer of its own:
 * states 10 x qttt_state_bytes(games) bytes, length u8[games], done u8[10, games], mask u8[10, games, 36],
 * pi f64[10, games, 36], v f32[10, games]; rows u8[games] (nullable) and exact u8[10, games] (nullable) are this entry's.
 * With L[g] = rows ? rows[g] : length[g], row (t, g) is RELABELLED iff all of these hold:
 *   t < L[g];   done[t, g] == 0;   the state's own count of moves played (qttt_solve.h's n) is >= min_ply;
 *   the position is no leaf of the solver (its `terminal` flag is clear and its legal mask is not empty) and at least one
 *   legal action has a child (qttt_solve.h's definitions, word for word).
 * A relabelled row gets
 *   v[t, g]      = (float)V, V the solver's value of the position for the player to move: a multiple of
 *                  1 / QTTT_SOLVE_DENOMINATOR in [-1, 1], never -0.0;
 *   pi[t, g, a]  = 1.0 / (double)k on the k legal actions with Q(a) == V and +0.0 on the other 36 - k, if policy != 0 (the
 *                  comparison is on the integers 16 Q: there is no tolerance); policy == 0 leaves pi alone;
 *   exact[t, g]  = 1.
 * Every other row keeps every byte of pi and v and gets exact[t, g] = 0, the rows at or past L[g] included: exact, when
 * given, is written at all 10 * games entries.  states, rows, length, done and mask are read only.  The legal actions are
 * those of the state's own legal mask, which is what the record wrote into mask[t, g]; mask is part of the staging set and
 * is checked like the others, the kernel does not load it.  Relabelling is idempotent: a second call stores the same bytes.
 *   `rows` is how a caller relabels some games only: SelfPlay.stream passes qttt_selfplay_harvest's harvest_len, which is
 * a finished game's length and 0 for every other slot, so only the games a ply hands to the ring are enumerated.
 *   The sign convention.  V is the mover's value, so the rows of one game alternate in sign as the record's
 * v[i] = v0 * (-1)^i does under value targets (v_first, v_second) = (1, -1).  The entry knows nothing of the targets the
 * other rows were written with: under the reference's (1, 0) a relabelled batch would mix two scales, and the caller must
 * not ask for it (SelfPlay raises).
 *   min_ply lies in QTTT_SELFPLAY_EXACT_MIN_PLY..QTTT_SELFPLAY_EXACT_MAX_PLY.  Six for the reason of
 * QTTT_TREE_EXACT_MIN_PLY: at six moves played a position's tree holds under 5 * 10^4 positions, at seven and more at most
 * 2 000; at five one board is milliseconds of work and needs qttt_solve's two levels (compose VecEnv.solve for that).  At
 * nine nothing is ever relabelled: a position with nine moves played is terminal.
 *
 * Errors, in qttt.h's order, before any device work: QTTT_ERR_SIZE for games < 0, min_ply outside
 * QTTT_SELFPLAY_EXACT_MIN_PLY..QTTT_SELFPLAY_EXACT_MAX_PLY, policy outside 0..1; 0 with no device work for games == 0;
 * QTTT_ERR_NULL for a null states, length, done, mask, pi or v; QTTT_ERR_ACTION for states not 16-byte aligned, pi not
 * 8-byte aligned, v not 4-byte aligned. */
#ifndef QTTT_SELFPLAY_EXACT_H
#define QTTT_SELFPLAY_EXACT_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QTTT_SELFPLAY_EXACT_MIN_PLY 6      /* as QTTT_TREE_EXACT_MIN_PLY, and for its reason */
#define QTTT_SELFPLAY_EXACT_MAX_PLY 9

int qttt_selfplay_exact_targets(const void *states, int64_t games, int min_ply, int policy, const uint8_t *rows,
                                const uint8_t *length, const uint8_t *done, const uint8_t *mask, double *pi, float *v,
                                uint8_t *exact, void *stream);

#ifdef __cplusplus
}
#endif
#endif
