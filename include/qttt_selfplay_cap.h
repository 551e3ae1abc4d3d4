/* qttt_selfplay_cap.h — the self-play record and harvest of playout cap randomisation (Wu, "Accelerating Self-Play Learning
 * in Go", 2019, section 3.1): most plies are searched cheaply and are NOT recorded, a random fraction gets the
 * full search and only those become rows of the batch.  Part of the C ABI of libqttt_hip.so (additive entries of
 * QTTT_ABI_VERSION 6; included by qttt.h after qttt_tree_subset.h; the staging buffers of qttt_selfplay.h, the per-game row
 * of qttt_selfplay_stream.h and the records of qttt_tree_explore.h and qttt_tree_forced.h hold here).
 *
 * ---- The draw (the caller's, on the host; stated here because it owns an index range).  Ply number i of game g is FULL iff
 *     (double)(qttt_hash(seed, board_offset + g, QTTT_SELFPLAY_CAP_BASE + i) >> 11) * 2^-53 < p
 * with i < QTTT_SELFPLAY_MAX_CAP_DRAWS, so the indices lie in 0xA0000000 .. 0xAFFFFFFF: above every select index
 * (QTTT_TREE_SELECT_BASE + k, k < 2^24), below QTTT_TREE_NOISE_BASE.  p = 1 makes every ply full.
 *
 * ---- qttt_selfplay_record_capped.  The per-game-row form only: the row is t = length[g] and a game is LIVE by
 * qttt_selfplay_stream.h's rule.  It takes qttt_selfplay_record_stream_pruned's arguments, then full u8[games].
 * forced_k < 0 asks for the unpruned pi row: the entry is then qttt_selfplay_record_stream_sampled's row (the plain row
 * with sample_plies = 0), and c_puct is not looked at.
 *   A game that is not live gets actions[g] = (255, 255) and nothing else, as there.
 *   A live game with full[g] != 0, and EVERY live game whose root is terminal, writes exactly what
 *     qttt_selfplay_record_stream_pruned (or _sampled) writes, but for the back-fill's signs (below).
 *   A live game with full[g] == 0 and a root that is not terminal writes actions[g] ONLY: the move that the record would
 *     have played (MCTS.choose, or the sampled move while t < sample_plies, drawn with draw_index as there).  No row, and
 *     length[g] does not advance: t counts the game's ROWS, no longer its plies.
 *
 * ---- qttt_selfplay_harvest_capped is qttt_selfplay_harvest for such batches: the same arguments, the same outputs, but
 * for the back-fill's signs.
 *
 * ---- The value back-fill, shared by the two.  A finished game's rows r = 0..t get v[r, g] = +v0 where the FIRST player is
 * to move in row r's recorded state (an even number of moves played, read from the staging `states`; the terminal row's
 * state is the root's), -v0 where the second is; v0 = v_first / v_second / 0 by the winner, a zero is +0.0.  When every ply
 * was recorded, row r has r moves played and these are the bits of qttt_selfplay_record_stream and qttt_selfplay_harvest.
 * A game whose plies were all fast yields its terminal row alone.
 *
 * Errors, in qttt_tree.h's order, before any device work.  The record: those of qttt_selfplay_record_stream_pruned in its
 * order, with forced_k only required to be finite and c_puct tested only where forced_k >= 0; QTTT_ERR_NULL also for a null
 * full.  The harvest: qttt_selfplay_harvest's. */
#ifndef QTTT_SELFPLAY_CAP_H
#define QTTT_SELFPLAY_CAP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QTTT_SELFPLAY_CAP_BASE 0xA0000000u
#define QTTT_SELFPLAY_MAX_CAP_DRAWS (1u << 28)

int qttt_selfplay_record_capped(const void *tree, int64_t games, int64_t capacity, uint32_t n_rollouts, double alpha,
                                double v_first, double v_second, void *states, double *pi, uint8_t *mask, uint8_t *done,
                                float *v, uint8_t *action36, uint8_t *length, int8_t *winner, uint8_t *actions,
                                uint64_t seed, int64_t board_offset, double temperature, int sample_plies,
                                uint32_t draw_index, double forced_k, double c_puct, const uint8_t *full, void *stream);

int qttt_selfplay_harvest_capped(const void *tree, int64_t games, int64_t capacity, double v_first, double v_second,
                                 void *states, double *pi, uint8_t *mask, uint8_t *done, float *v, uint8_t *action36,
                                 uint8_t *length, int8_t *winner, uint8_t *actions, uint8_t *harvest_len, uint8_t *finished,
                                 int64_t *games_done, int64_t *tally, void *stream);

#ifdef __cplusplus
}
#endif
#endif
