/* qttt_tree_explore.h — root exploration for self-play on the device search trees of qttt_tree.h: Dirichlet noise mixed
 * into the roots' priors before the search of a move, and the move drawn from the visit counts.  Part of
 * the C ABI of libqttt_hip.so (additive entries of QTTT_ABI_VERSION 6; included by qttt.h after qttt_tree_value.h; the
 * buffer layout, conventions and error order of qttt_tree.h and qttt_selfplay.h hold here: device pointers owned by the
 * caller, work enqueued on `stream`, 0 / hipError_t / negative argument error).
 *
 * A searched move of self-play with exploration is
 *   one rollout (so that every live root has priors) -> qttt_tree_root_noise -> the other rollouts ->
 *   qttt_selfplay_record_sampled -> qttt_step -> qttt_tree_sync [-> qttt_tree_compact]
 * with no host synchronisation in between.
 *
 * Draws.  Both entries draw from qttt_hash(seed, board_offset + g, idx) at indices the playouts (idx < 2^31) and
 * select (QTTT_TREE_SELECT_BASE + k, k < 2^24) never use:
 *   noise:  QTTT_TREE_NOISE_BASE + (noise_idx * 36 + a) * QTTT_TREE_NOISE_DRAWS + j for action a and draw j <
 *           QTTT_TREE_NOISE_DRAWS = 2 * QTTT_TREE_NOISE_TRIES + 1.  noise_idx < QTTT_TREE_MAX_NOISE (the caller counts
 *           its calls since qttt_tree_reset), which keeps every noise index below QTTT_SELFPLAY_MOVE_BASE.
 *   move:   QTTT_SELFPLAY_MOVE_BASE + ply, ply < QTTT_SELFPLAY_ROWS.
 * Uniforms, both strictly inside (0, 1):  U53(h) = ((h >> 11) + 0.5) * 2^-53 of a 64-bit h,  U32(w) = (w + 0.5) * 2^-32
 * of a 32-bit w.
 *
 * ---- qttt_tree_root_noise: P <- (1 - epsilon) P + epsilon Dirichlet(alpha) at the root of every game.
 * A game is NOISED when its root has priors (uniform or stored), is not terminal and has a legal action.  Per noised
 * game, in IEEE doubles without contraction into FMAs (log, cos, sqrt and pow are the device library's, a few ulps from
 * the exact functions):
 *   Gamma(alpha) per legal action a, Marsaglia-Tsang:  a' = alpha < 1 ? alpha + 1 : alpha,  d = a' - 1/3,
 *     c = 1 / sqrt(9 d).  Try t = 0 .. QTTT_TREE_NOISE_TRIES - 1 takes h0 = hash(.., base + 2 t) and h1 = hash(.., base +
 *     2 t + 1), base = QTTT_TREE_NOISE_BASE + (noise_idx * 36 + a) * QTTT_TREE_NOISE_DRAWS:
 *       x = sqrt(-2 ln U53(h0)) * cos(2 pi * U32(h1 >> 32)),   u = 1 + c x,   v = u * u * u,
 *       accepted when v > 0 and ln U32((uint32_t)h1) < 0.5 * x * x + d - d * v + d * ln v
 *       (evaluated left to right: ((0.5 x) x + d - d v) + d ln v).
 *     The first accepted try gives y = d v; if none is accepted, y = a'.  For alpha < 1,
 *     y = y * pow(U53(hash(.., base + 2 * QTTT_TREE_NOISE_TRIES)), 1 / alpha).  y = 0 at illegal actions.
 *   S = the sum of y over 64 terms as qttt_selfplay.h takes it (y_0 .. y_35, 28 zeros; s[i] = s[i] + s[i ^ m] for m = 1,
 *     2, 4, 8, 16, 32).  If S is 0 or not finite, the game is not noised after all.
 *   n_a = y_a / S.  The root's prior row (qttt_tree.h: f32[36] of the root's node) becomes
 *     (float)((1 - epsilon) * p_a + epsilon * n_a) on the legal actions and 0.0f elsewhere, p_a = the prior the search
 *     read so far as a double: (double) of the stored f32, or 1 / popcount(legal) of a uniform root.  The node's flags
 *     keep everything but the uniform bit, which is cleared: a uniform root becomes a root with stored priors (which
 *     qttt_tree_compact moves like any other).  noise[g] = n (0 at illegal actions), applied[g] = 1.
 * Nothing else in the tree is written.  A game that is not noised gets applied[g] = 0, a zero noise row, and not one
 * byte of its tree changes.  noise f64[games, 36] and applied u8[games] are both nullable.
 * A second call on the same root mixes again, into the already noised priors; epsilon = 0 leaves stored priors bit for
 * bit (the double of an f32 rounds back to it) but turns a uniform root's 1 / m into (float)(1 / m).
 * Every loop is bounded by the constants below (the try loop may end early once every lane of the wave has accepted);
 * nothing waits on memory and there are no atomics.
 *
 * Errors, in this order, before any device work: QTTT_ERR_SIZE for games < 0, capacity outside
 * 1..QTTT_TREE_MAX_CAPACITY, board_offset < 0, noise_idx >= QTTT_TREE_MAX_NOISE, epsilon outside [0, 1] or not finite,
 * alpha not finite or <= 0; 0 with no device work for games == 0; QTTT_ERR_NULL for a null tree; QTTT_ERR_ACTION for a
 * tree not 16-byte or a noise not 8-byte aligned.
 *
 * ---- qttt_selfplay_record_sampled: qttt_selfplay_record with the move drawn from the visit counts.
 * Every buffer, every field and every rule is qttt_selfplay_record's (qttt_selfplay.h), but for the move of a live root
 * that is not terminal at ply < sample_plies:
 *   w_a = (double)N[a] when temperature == 1.0, else pow((double)N[a], 1.0 / temperature), on the legal actions with
 *     N[a] > 0; 0 elsewhere (lanes 36..63 included).
 *   c = the inclusive scan of w over lanes 0..63: for m = 1, 2, 4, 8, 16, 32 in this order, every lane i >= m adds the old
 *     value of lane i - m.  T = c[63].
 *   t = ((double)(hash(seed, board_offset + g, QTTT_SELFPLAY_MOVE_BASE + ply) >> 11) * 2^-53) * T.
 *   The move is the lowest a with w_a > 0 and t < c[a].  (t < T always; w_a > 0 only matters when two scan orders of
 *   one sum round differently, and keeps the move legal then.)  If T is 0 or not finite, or no such a exists, the move
 *   is MCTS.choose as in qttt_selfplay_record.
 * action36, actions and everything downstream follow the move; pi stays the visit-count target.  With temperature == 1
 * every quantity is an exact integer in a double.  sample_plies == 0 gives qttt_selfplay_record's bytes.
 *
 * Errors: those of qttt_selfplay_record, in its order, with, after alpha's, QTTT_ERR_SIZE for board_offset < 0,
 * temperature not finite or <= 0 and sample_plies outside 0..QTTT_SELFPLAY_ROWS. */
#ifndef QTTT_TREE_EXPLORE_H
#define QTTT_TREE_EXPLORE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QTTT_TREE_NOISE_BASE 0xC0000000u
#define QTTT_TREE_NOISE_TRIES 16
#define QTTT_TREE_NOISE_DRAWS (2 * QTTT_TREE_NOISE_TRIES + 1)      /* per (noise_idx, action) */
#define QTTT_SELFPLAY_MOVE_BASE 0xE0000000u
/* the largest count of noise_idx values whose indices stay below QTTT_SELFPLAY_MOVE_BASE: 451 911 */
#define QTTT_TREE_MAX_NOISE ((QTTT_SELFPLAY_MOVE_BASE - QTTT_TREE_NOISE_BASE) / (36u * QTTT_TREE_NOISE_DRAWS))

int qttt_tree_root_noise(void *tree, int64_t games, int64_t capacity, uint64_t seed, uint32_t noise_idx,
                         int64_t board_offset, double epsilon, double alpha, double *noise, uint8_t *applied,
                         void *stream);

int qttt_selfplay_record_sampled(const void *tree, int64_t games, int64_t capacity, int ply, uint32_t n_rollouts,
                                 double alpha, double v_first, double v_second, void *states, double *pi, uint8_t *mask,
                                 uint8_t *done, float *v, uint8_t *action36, uint8_t *length, int8_t *winner,
                                 uint8_t *actions, uint64_t seed, int64_t board_offset, double temperature,
                                 int sample_plies, void *stream);

#ifdef __cplusplus
}
#endif
#endif
