/* qttt_selfplay_stream.h — continuous self-play: finished games restart in place and feed the replay ring.
 * Part of the C ABI of libqttt_hip.so (additive entries of QTTT_ABI_VERSION 6; included by qttt.h after qttt_train.h; the
 * buffers of qttt_selfplay.h and the conventions of qttt_replay.h hold here: device pointers owned by the caller, work
 * enqueued on `stream`, 0 / hipError_t / negative argument error, and no call waits for the device).
 *
 * qttt_selfplay_record plays `games` games in lockstep: one scalar `ply` is every game's row.  Here every game slot keeps
 * its own ply in length[g], and one stream ply of all slots is
 *   the search of a move (qttt_tree.h ...) -> qttt_selfplay_record_stream -> qttt_step(actions) -> qttt_tree_sync
 *   [-> qttt_tree_compact] -> qttt_selfplay_harvest -> qttt_replay_append(length = harvest_len) -> qttt_selfplay_restart
 * with no host synchronisation in between.  A slot whose new root is terminal is harvested (its terminal row and value
 * targets are written, its rows go to the ring) and restarted from the empty board; the other slots are not touched.  The
 * staging buffers are those of qttt_selfplay.h (states, pi, mask, done, v, action36, length, winner, actions), zero-filled
 * by the caller before the first ply.
 *
 * ---- qttt_selfplay_record_stream (and _sampled, _gumbel): qttt_selfplay_record (qttt_selfplay_record_sampled of
 * qttt_tree_explore.h, qttt_selfplay_record_gumbel of qttt_tree_gumbel.h) with the row t = length[g] read per game instead
 * of the scalar ply.  Game g is LIVE when t < QTTT_SELFPLAY_ROWS and (t == 0 or done[t - 1, g] == 0); a game that is not
 * live gets actions[g] = (255, 255) and nothing else.  Every field and every rule of a live game's row is the lockstep
 * entry's at ply = t, bit for bit — the kernels are instantiations of one body — so a batch recorded in lockstep order
 * through these entries is the batch of the lockstep entries.  The sampled record draws its move when t < sample_plies,
 * from qttt_hash(seed, board_offset + g, QTTT_SELFPLAY_MOVE_BASE + draw_index): the index is the caller's counter,
 * draw_index < QTTT_SELFPLAY_MAX_MOVE_DRAWS, which keeps it below QTTT_TREE_GUMBEL_BASE.
 *   Errors: those of the lockstep entry, in its order, without the test of ply; the sampled record adds, last of its
 * QTTT_ERR_SIZE tests, draw_index >= QTTT_SELFPLAY_MAX_MOVE_DRAWS.
 *
 * ---- qttt_selfplay_harvest.  One launch after the sync, a wave per game.  With t = length[g]: a slot whose root is
 * terminal (and t < QTTT_SELFPLAY_ROWS: always, a game is nine moves at most) gets row t exactly as qttt_selfplay_record
 * writes a terminal root's row at ply t — the state, pi = 1 / 36 and mask = 1 at all 36 actions, done = 1, action36 = 255,
 * actions[g] = (255, 255), length[g] = t + 1, winner[g], and v[i, g] = v0 * (-1)^i for i = 0..t — by the same device
 * function; and harvest_len[g] = t + 1, finished[g] = 1, games_done[g] += 1, tally[g, k] += 1 for k = 0 / 1 / 2 = the first
 * player / the second player / nobody won, tally[g, 3] += t + 1.  Every other slot gets harvest_len[g] = 0 and finished[g]
 * = 0 and nothing else.  harvest_len u8[games] is the `length` to give qttt_replay_append with the staging buffers: the
 * harvested games' rows are appended in ascending slot order, each game's in row order.  games_done i64[games] and tally
 * i64[games, QTTT_SELFPLAY_TALLIES] are the caller's cumulative counters (zero-filled before the first ply): per-slot
 * integers that only the slot's wave writes; there are no atomics.  The tree is read only.
 *   Errors, in this order, before any device work: QTTT_ERR_SIZE for games < 0, capacity outside
 * 1..QTTT_TREE_MAX_CAPACITY, v_first or v_second not finite; 0 with no device work for games == 0; QTTT_ERR_NULL for any
 * null buffer; QTTT_ERR_ACTION for tree or states not 16-byte aligned, pi, games_done or tally not 8-byte aligned, v not
 * 4-byte aligned.
 *
 * ---- qttt_selfplay_restart.  One launch after the append has been enqueued.  For every slot with finished[g] != 0:
 *   board g of `state` (qttt_state_bytes(games) bytes, the environment's packed states) becomes the empty board, both words 0;
 *   tree slot g becomes what qttt_tree_reset makes of the empty board: node 0 is the root (no priors, 36 empty slots),
 *     used = 1, root = depth = leaf = 0, the header's flags those of that root — the same bytes written, the same bytes
 *     left alone (the header's padding and path entries, the records past node 0);
 *   length[g] = 0, and the slot's ten staging rows are zeroed: states, pi, mask, done, v and action36 at rows 0..9 (row 0
 *     too, which the next record overwrites: rows at or past a game's length are zero at all times).  winner[g] and
 *     actions[g] keep the finished game's values until the slot's next harvest and record.
 * A slot with finished[g] == 0 keeps every byte.
 *   Errors, in this order, before any device work: QTTT_ERR_SIZE for games < 0 or capacity outside
 * 1..QTTT_TREE_MAX_CAPACITY; 0 with no device work for games == 0; QTTT_ERR_NULL for any null buffer; QTTT_ERR_ACTION for
 * tree, state or states not 16-byte aligned, pi not 8-byte aligned, v not 4-byte aligned. */
#ifndef QTTT_SELFPLAY_STREAM_H
#define QTTT_SELFPLAY_STREAM_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QTTT_SELFPLAY_MAX_MOVE_DRAWS (1u << 28)    /* QTTT_TREE_GUMBEL_BASE - QTTT_SELFPLAY_MOVE_BASE */
#define QTTT_SELFPLAY_TALLIES 4                    /* first player won, second player won, nobody won, rows harvested */

int qttt_selfplay_record_stream(const void *tree, int64_t games, int64_t capacity, uint32_t n_rollouts, double alpha,
                                double v_first, double v_second, void *states, double *pi, uint8_t *mask, uint8_t *done,
                                float *v, uint8_t *action36, uint8_t *length, int8_t *winner, uint8_t *actions,
                                void *stream);

int qttt_selfplay_record_stream_sampled(const void *tree, int64_t games, int64_t capacity, uint32_t n_rollouts, double alpha,
                                        double v_first, double v_second, void *states, double *pi, uint8_t *mask,
                                        uint8_t *done, float *v, uint8_t *action36, uint8_t *length, int8_t *winner,
                                        uint8_t *actions, uint64_t seed, int64_t board_offset, double temperature,
                                        int sample_plies, uint32_t draw_index, void *stream);

int qttt_selfplay_record_stream_gumbel(const void *tree, int64_t games, int64_t capacity, uint32_t n_rollouts, double alpha,
                                       double v_first, double v_second, void *states, double *pi, uint8_t *mask,
                                       uint8_t *done, float *v, uint8_t *action36, uint8_t *length, int8_t *winner,
                                       uint8_t *actions, const void *rec, double c_visit, double c_scale, void *stream);

int qttt_selfplay_harvest(const void *tree, int64_t games, int64_t capacity, double v_first, double v_second, void *states,
                          double *pi, uint8_t *mask, uint8_t *done, float *v, uint8_t *action36, uint8_t *length,
                          int8_t *winner, uint8_t *actions, uint8_t *harvest_len, uint8_t *finished, int64_t *games_done,
                          int64_t *tally, void *stream);

int qttt_selfplay_restart(void *tree, int64_t games, int64_t capacity, void *state, const uint8_t *finished, void *states,
                          double *pi, uint8_t *mask, uint8_t *done, float *v, uint8_t *action36, uint8_t *length,
                          void *stream);

#ifdef __cplusplus
}
#endif
#endif
