/* qttt_policy_rollout.h — network-guided playouts, part of the C ABI of libqttt_hip.so (an additive entry of
 * QTTT_ABI_VERSION 6; included by qttt.h, whose conventions hold here: device pointers owned by the caller, work enqueued
 * on `stream`, 0 / hipError_t / negative argument error).
 *
 * AlphaZero._rollout's simulation loop (alphazero.py:173-180) with AlphaZero._simulate (:192-205) under the
 * policy/value network, for n boards x n_sims simulations in ONE launch.  Every ply of a simulation runs
 * Model.forward(node.to_vector()) (get_action_probs, :294-300; the network and weights of qttt_nn.h, `precision` as in
 * qttt_evaluate), samples an action from Categorical(logits) (sample_action, :302-303), steps, and keeps one of the
 * collapse children (:202), until the game is over: the done bit (a line, or nine moves) or fewer than two empty squares,
 * as qttt_rollout.  The boards (`state`, n of them) are not modified.
 *
 * Draws.  Lane j = i * n_sims + s plays simulation s of board i.  Ply p of it takes
 *   (h1, h2) = the low and high 32 bits of qttt_hash(seed, board_offset + i, step_idx0 + s * QTTT_SIM_STRIDE + p)
 *   collapse bit = h1 >> 31 (as qttt_rollout)
 *   u = (h2 >> 8) * 2^-24; over the legal actions a in ascending order, e_a = expf(logit_a - max) and S = sum of e_a
 *   (the expressions of qttt_evaluate's probs, f32); the action is the smallest legal a whose running sum of e_a
 *   exceeds u * S, or the largest legal a if rounding leaves none.  With non-finite weights the same rule holds: where
 *   a NaN or infinite logit makes every comparison fail, the move is the largest legal action, so every move is legal.
 * So simulation s equals a one-simulation call with step_idx0 + s * QTTT_SIM_STRIDE, and board_offset shifts the draws
 * as it does for qttt_rollout_many.
 *
 * Outputs (all but `result` nullable; only those given are written):
 *   result     i8[n, n_sims]     AlphaZero._reward (alphazero.py:207-215) of the final board: +1 winner True,
 *                                -1 winner False, 0 None
 *   plies      u8[n, n_sims]     plies played (0 for a finished leaf)
 *   trace      u8[n, n_sims, 9]  per ply played: action36 | collapse_bit << 6 (action36 as ind2move, qttt_expand);
 *                                0xFF after the last one
 *   leaf_value f32[n]            the network's value of board i and its
 *   leaf_probs f32[n, 36]        Categorical(logits).probs (the node.P that _simulate leaves on the leaf, :197-198),
 *                                bit for bit qttt_evaluate's value and probs at the same precision (NaN rows included)
 * Errors, in this order: QTTT_ERR_SIZE for n < 0, board_offset < 0, an unknown precision or n_sims outside
 * 1..QTTT_POLICY_ROLLOUT_MAX_SIMS; 0 with no device work for n == 0; QTTT_ERR_NULL for a null state, weights or result;
 * QTTT_ERR_ACTION for weights not 16-byte aligned or leaf_value / leaf_probs not 4-byte aligned. */
#ifndef QTTT_POLICY_ROLLOUT_H
#define QTTT_POLICY_ROLLOUT_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QTTT_POLICY_ROLLOUT_MAX_SIMS 128
int qttt_rollout_policy(const void *state, const void *weights, int precision,
                        uint64_t seed, uint32_t step_idx0, int64_t board_offset, int n_sims,
                        int8_t *result, uint8_t *plies, uint8_t *trace,
                        float *leaf_value, float *leaf_probs, int64_t n, void *stream);

#ifdef __cplusplus
}
#endif
#endif
