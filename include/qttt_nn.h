/* qttt_nn.h — the policy/value network part of the C ABI of libqttt_hip.so (QTTT_ABI_VERSION >= 6; included by
 * qttt.h, whose conventions hold here: device pointers owned by the caller, work enqueued on `stream`, 0 / hipError_t /
 * negative argument error).
 *
 * The reference's policy/value network, nn.Model.forward(GameState.to_vector()) (nn.py:7-72, called at every node
 * by alphazero.py:294-300), for n boards in ONE launch on the matrix cores: the 180 -> 256 -> 256 -> 256 ReLU trunk,
 * the value head (-> 1) and the policy head (-> 36), illegal actions masked.
 *   value  f32[n]      V_head output
 *   logits f32[n,36]   pi_head output; -inf where square i or j of action (i,j) = ind2move(a) holds a classical mark
 *                      (nn.py:44-61 get_mask)
 *   probs  f32[n,36]   torch.softmax(logits) = Categorical(logits).probs: 0 at masked actions, NaN in every column of
 *                      a row whose 36 actions are all masked (terminal positions), as torch gives
 * Each output is nullable, at least one must be given; only those given are written.  `state` is not modified.
 * precision QTTT_NN_F32: exact-f32 MFMA (the reference's numerics up to summation order); QTTT_NN_BF16: bf16
 * weights and activations (the input included: 1/3 becomes 0.333984375), f32 accumulation and biases.
 * Non-finite numbers propagate as in torch: the trunk's ReLU keeps a NaN (relu(NaN) = NaN, not 0), 0 * inf = NaN, and an
 * f32 accumulator that overflows gives +-inf, so a NaN or an infinity that torch's forward on the same weights produces
 * appears in value and logits at the same positions; masked logits stay -inf.  probs of a row with a NaN or +inf
 * legal logit are NaN at its legal actions and 0 at its masked ones.
 * Errors: QTTT_ERR_SIZE for n < 0 or an unknown precision, QTTT_ERR_NULL for a null state / weights or no
 * output, QTTT_ERR_ACTION for weights not 16-byte aligned or an output not 4-byte aligned.
 *
 * Packed weight blob: qttt_nn_weights_bytes(precision) bytes of DEVICE memory, 16-byte aligned.  With T = float
 * (QTTT_NN_F32) or bfloat16 (QTTT_NN_BF16, round-to-nearest-even from f32) and the reference's torch.nn.Linear
 * weights W[out][in], the four matrices B_L[k][c] = W_L[c][k] of the layers L = 1, 2, 3, head follow each other
 * as T elements, then the biases as f32:
 *   layer   K (rows k)                          C (columns c)   source
 *   1       180 (f32) / 192 (bf16, rows >= 180 zero)   256      fc.0.weight
 *   2       256                                  256            fc.2.weight
 *   3       256                                  256            fc.4.weight
 *   head    256                                  48             c < 36: pi_head.1.weight[c]; c = 36: V_head.1.weight[0];
 *                                                               c > 36: zero
 * Inside a matrix (C / 16 = NC column tiles), element [k][c] is at T offset
 *   f32:  ((k/4  * NC + c/16) * 64 + (k%4)       * 16 + c%16)
 *   bf16: ((k/32 * NC + c/16) * 64 + (k%32 / 8)  * 16 + c%16) * 8 + k%8
 * from the matrix's start (one 16 x 16 MFMA B fragment per 64-lane group).  Biases, f32, after the last matrix:
 * fc.0.bias[256], fc.2.bias[256], fc.4.bias[256], then 48 head biases (pi_head.1.bias[36], V_head.1.bias[0], 11
 * zeros).  Sizes: 761 024 bytes (f32), 388 288 bytes (bf16).  qtttgym_amd/policy_value.py pack_weights builds it. */
#ifndef QTTT_NN_H
#define QTTT_NN_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QTTT_NN_F32  0
#define QTTT_NN_BF16 1
/* bytes of the packed blob for a precision; -1 for an unknown precision.  Host-callable, no device work. */
int64_t qttt_nn_weights_bytes(int precision);
int qttt_evaluate(const void *state, const void *weights, int precision,
                  float *value, float *logits, float *probs,
                  int64_t n, void *stream);

#ifdef __cplusplus
}
#endif
#endif
