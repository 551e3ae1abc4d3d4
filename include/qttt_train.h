/* qttt_train.h — the training step of the policy/value network on the device: the reference's loss, its gradients and
 * its AMSGrad step, all on the packed f32 weight blob of qttt_nn.h.  Part of the C ABI of libqttt_hip.so
 * (additive entries of QTTT_ABI_VERSION 6; included by qttt.h after qttt_replay.h; the conventions of qttt_nn.h and
 * qttt_replay.h hold here: device pointers owned by the caller, work enqueued on `stream`, 0 / hipError_t / negative
 * argument error, and no call waits for the device).  f32 only.
 *
 * ---- Parameters, gradients and optimiser state all have ONE layout: the QTTT_NN_F32 blob (qttt_nn.h "packed weight
 * blob", 761 024 bytes = 190 256 f32: the four matrices in MFMA fragment order, then the 816 biases).  `weights` IS the
 * blob qttt_evaluate reads; grads, m, v2 and vmax are buffers of the same size in which element e belongs to weight
 * element e.  The blob's pad elements (the head's columns 37..47 and their biases) receive gradient exactly +0, so a pad
 * that starts at zero stays zero under the optimiser.
 *
 * ---- qttt_train_gradients.  For a minibatch of n samples as qttt_replay_sample (or qttt_encode and the self-play
 * record) gives them, with (value_i, logits_i) = the network on row s_i and its mask applied to the logits:
 *   L_i  = 0.5 (value_i - v_i)^2
 *   J_i  = sum over legal a of pi_ia (log(pi_ia + 1e-7) - log_softmax(masked logits_i)_a);  +0 for a terminal sample
 *   loss = mean_i L_i + mean over the non-terminal i of J_i            (the reference's, self_play.py:226-236)
 * and grads[e] = d loss / d weights[e].  At the outputs: d value_i = (value_i - v_i) / n; on a legal action of a
 * non-terminal sample d logit_ia = (softmax_ia * sum over legal b of pi_ib - pi_ia) / n_keep, n_keep the number of
 * non-terminal samples; exactly +0 everywhere else.  ReLU's derivative is (h > 0): 0 at 0, as torch's.  With n_keep == 0
 * the policy term contributes nothing to grads (the caller's mean of J is then 0/0, as in torch).  L and J (f32[n], each
 * nullable) receive the per-sample terms.  A non-terminal sample needs at least one legal action; NaNs and infinities
 * in s, pi, v or the weights are outside the contract (nothing is promised about grads, L or J then; every loop is
 * still bounded by a compile-time count or by n, and nothing is written outside the buffers below).
 *   The work is five launches that the stream orders, none of which waits on another workgroup: the count of the
 * non-terminal samples (an integer sum); forward + loss per tile of 64 samples, which stores the three post-ReLU
 * activations and the output gradient; the backward pass through the activations per tile; the weight gradients, where
 * a workgroup owns a 64 x 64 block of one matrix for one chunk of QTTT_TRAIN_CHUNK samples and writes its partial sum;
 * and the sum of the partials in ascending chunk order.  No floating-point atomics: the same inputs give the same bits
 * on every call.  Nothing is accumulated into: grads, L, J and the workspace may hold anything on entry.
 *   `workspace`: qttt_train_workspace_bytes(n) bytes of device memory, 256-byte aligned, used by this call only (calls
 * that share one must be ordered by their streams): six f32[n, 256] activation / activation-gradient arrays, the output
 * gradient f32[n, 48], one blob-sized partial per chunk, and the count.  qttt_train_workspace_bytes is host-callable and
 * does no device work; it returns -1 for n outside 1..QTTT_TRAIN_MAX_SAMPLES.
 *   Errors, in this order, before any device work: QTTT_ERR_SIZE for n outside 1..QTTT_TRAIN_MAX_SAMPLES; QTTT_ERR_NULL
 * for a null s, pi, mask, v, done, weights, grads or workspace; QTTT_ERR_ACTION for weights or grads not 16-byte, workspace
 * not 256-byte, pi not 8-byte, or s, v, L or J not 4-byte aligned.
 *
 * ---- qttt_train_adam.  torch.optim.Adam(lr, betas, eps, weight_decay, amsgrad=True) (not AdamW), one launch over the
 * whole blob, biases included; `step` is the 1-based number of this step:
 *   g = grads + weight_decay * w;  m = beta1 m + (1 - beta1) g;  v2 = beta2 v2 + (1 - beta2) g^2;  vmax = max(vmax, v2)
 *   w -= lr / (1 - beta1^step) * m / (sqrt(vmax) / sqrt(1 - beta2^step) + eps)
 * in f32 (the two bias corrections are computed on the host in f64 and rounded once).  weights, m, v2 and vmax are
 * updated in place; grads is read only.  With `weights_bf16` (nullable: a QTTT_NN_BF16 blob) the same launch stores
 * every new weight, rounded to nearest even, at its place in that blob and copies every bias as f32; its layer-1 rows
 * 180..191 are not written (they are zero in every blob pack_weights made, and stay so).  The bf16 blob ends up
 * bit-identical to the packing of the new f32 weights.
 *   Errors, in this order: QTTT_ERR_SIZE for step < 1; QTTT_ERR_NULL for a null weights, grads, m, v2 or vmax;
 * QTTT_ERR_ACTION for any of the six blobs not 16-byte aligned. */
#ifndef QTTT_TRAIN_H
#define QTTT_TRAIN_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QTTT_TRAIN_CHUNK 256                /* samples per partial sum of the weight gradients */
#define QTTT_TRAIN_MAX_SAMPLES (1 << 24)

int64_t qttt_train_workspace_bytes(int64_t n);
int qttt_train_gradients(const float *s, const double *pi, const uint8_t *mask, const float *v, const uint8_t *done,
                         int64_t n, const void *weights, void *grads, float *L, float *J, void *workspace, void *stream);
int qttt_train_adam(void *weights, const void *grads, void *m, void *v2, void *vmax, int64_t step, float lr, float beta1,
                    float beta2, float eps, float weight_decay, void *weights_bf16, void *stream);

#ifdef __cplusplus
}
#endif
#endif
