/* qttt_train_weighted.h — importance weights in the training step's loss: qttt_train_gradients (qttt_train.h, whose
 * conventions, layouts, workspace and launches hold here) with one more input, for minibatches drawn by priority
 * (qttt_replay_priority.h).  Part of the C ABI of libqttt_hip.so (an additive entry of QTTT_ABI_VERSION 6;
 * included by qttt.h after qttt_replay_priority.h).
 *
 * ---- qttt_train_gradients_weighted.  `weight` is f32[n] on the device, the importance weight w_i of sample i.
 *   loss = mean_i w_i L_i + (sum over the non-terminal i of w_i J_i) / n_keep
 * with L_i, J_i and n_keep of qttt_train_gradients.  At the outputs, d value_i and d logit_ia are that entry's values,
 * rounded as there, then multiplied by w_i in f32; everything behind the outputs is the same five launches.  L and J
 * receive the UNWEIGHTED per-sample terms: they are what the priorities are made of.  A weight vector of all 1.0f gives
 * grads, L and J bit-identical to qttt_train_gradients; a sample with weight 0 contributes a zero to every sum.  The
 * forward kernel's loss tail is a compile-time variant, so the unweighted entry runs the code it ran before.
 *   Errors, in this order, before any device work: QTTT_ERR_SIZE for n outside 1..QTTT_TRAIN_MAX_SAMPLES; QTTT_ERR_NULL
 * for a null s, pi, mask, v, done, weight, weights, grads or workspace; QTTT_ERR_ACTION for weights or grads not 16-byte,
 * workspace not 256-byte, pi not 8-byte, or s, v, L, J or weight not 4-byte aligned. */
#ifndef QTTT_TRAIN_WEIGHTED_H
#define QTTT_TRAIN_WEIGHTED_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int qttt_train_gradients_weighted(const float *s, const double *pi, const uint8_t *mask, const float *v, const uint8_t *done,
                                  const float *weight, int64_t n, const void *weights, void *grads, float *L, float *J,
                                  void *workspace, void *stream);

#ifdef __cplusplus
}
#endif
#endif
