/* qttt_symmetry.h — the eight symmetries of the board on the device: the image of packed states, and the self-play
 * batch of G games as the batch of K * G games it stands for.  Part of the C ABI of libqttt_hip.so (an
 * additive entry of QTTT_ABI_VERSION 6; included by qttt.h after qttt_selfplay.h, whose conventions hold here: device
 * pointers owned by the caller, work enqueued on `stream`, 0 / hipError_t / negative argument error).
 *
 * The group.  Square v = 3 r + c.  Symmetry k = 0..7: if k & 4, mirror first, (r, c) -> (r, 2 - c); then a quarter turn
 * clockwise, (r, c) -> (c, 2 - r), k & 3 times.  That is sigma_k, a permutation of the nine squares; k = 0 is the
 * identity.  On the 36 actions (the unordered pairs in lexicographic order, mcts.py:339-350) it acts as
 * tau_k[a] = move2ind(sigma_k(i), sigma_k(j)) for (i, j) = ind2move(a).
 *
 * The image of a state under k is THE STATE THAT STEPPING REACHES WHEN THE MIRRORED GAME IS PLAYED: every move (lo, hi)
 * replaced by (sigma(lo), sigma(hi)) and every collapse landing on sigma of the square it landed on.  All 16 bytes of
 * it: Board.board, Board.moves (each pair re-sorted) and the set of Board.qstructs are the permuted attributes; the
 * rooted forest is rebuilt by qttt_import's insertion rule; and the LIST ORDER of the qstructs, which is not the
 * permuted order (update_qstructs keeps a union at the place of the set that holds the move's LOWER square, and a
 * symmetry can swap lower and higher), is what replaying the still un-collapsed moves in round order through
 * update_qstructs' append / add / merge rules gives.  The implicit autofill stays implicit; the done bit is computed
 * as qttt_import computes it.  So node keys, encode, evaluate and every later step see exactly the position the
 * mirrored game would have produced.
 */
#ifndef QTTT_SYMMETRY_H
#define QTTT_SYMMETRY_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QTTT_SYMMETRIES 8

/* The tables, host-callable, no device work; each pointer is HOST memory and nullable (only what is asked for is
 * written): cells u8[8, 9] = sigma_k[v]; actions u8[8, 36] = tau_k[a]; inverse u8[8]; compose u8[8, 8] with
 * compose[a][b] = the k for which sigma_k = sigma_b o sigma_a (a first, then b).  Returns 0. */
int qttt_symmetry_tables(uint8_t *cells, uint8_t *actions, uint8_t *inverse, uint8_t *compose);

/* state_out[i] = the image of state_in[i], n boards each, one launch, one lane per board.  The two buffers may be the
 * same one (a lane reads its board before it writes it); they must not overlap otherwise.
 *   sym   u8[n] device memory: board i's symmetry, or NULL: every board's is `k`.  A sym[i] > 7 leaves board i's
 *         output equal to its input.
 *   k     0..7, checked in either case.
 * Errors, in this order, before any device work: QTTT_ERR_SIZE for n < 0 or k outside 0..7; 0 with no device work for
 * n == 0; QTTT_ERR_NULL for a null state buffer; QTTT_ERR_ACTION for a state buffer that is not 16-byte aligned. */
int qttt_transform(const void *state_in, void *state_out, const uint8_t *sym, int k, int64_t n, void *stream);

/* A self-play batch of `games` games (the nine buffers of qttt_selfplay_record, filled by a whole game) -> the batch of
 * n_sym * games games of its images, one launch.  symmetries u8[n_sym] is HOST memory, 1 <= n_sym <= 8, each entry
 * 0..7.  Output game j = s * games + g is game g under symmetries[s].  The output buffers are sized for n_sym * games
 * games (states: 10 x qttt_state_bytes(n_sym * games), each row addressed by its own plane stride) and zero-filled by
 * the caller; they must not overlap the inputs.
 *   rows t < length[g] (length is read as at most 10): states through qttt_transform's image; pi'[tau(a)] = pi[a], the
 *     eight bytes moved, never recomputed; mask'[tau(a)] = mask[a]; done and v copied; action36' = tau(action36), a
 *     value past 35 (255: none) stays.
 *   per game: length and winner copied; actions = sigma of each square, a value past 8 (255) stays.
 *   rows at or past length[g] are not written.
 * Errors, in this order, before any device work: QTTT_ERR_SIZE for games < 0, n_sym outside 1..8, or (symmetries given)
 * an entry past 7; 0 with no device work for games == 0; QTTT_ERR_NULL for symmetries or any of the eighteen buffers
 * null; QTTT_ERR_ACTION for a states buffer not 16-byte, a pi buffer not 8-byte or a v buffer not 4-byte aligned. */
int qttt_selfplay_augment(int64_t games, const uint8_t *symmetries, int n_sym, const void *states, const double *pi,
                          const uint8_t *mask, const uint8_t *done, const float *v, const uint8_t *action36,
                          const uint8_t *length, const int8_t *winner, const uint8_t *actions, void *states_out,
                          double *pi_out, uint8_t *mask_out, uint8_t *done_out, float *v_out, uint8_t *action36_out,
                          uint8_t *length_out, int8_t *winner_out, uint8_t *actions_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif
