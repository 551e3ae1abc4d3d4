/* qttt_nn_symmetric.h — the policy/value network averaged over a position's symmetries, in ONE launch on the matrix
 * cores.  Part of the C ABI of libqttt_hip.so (an additive entry of QTTT_ABI_VERSION 6; included by
 * qttt.h after qttt_tree_explore.h; the conventions of qttt.h, the outputs, precisions and weight blob of qttt_nn.h and
 * the group of qttt_symmetry.h hold here: device pointers owned by the caller, work enqueued on `stream`, 0 /
 * hipError_t / negative argument error).
 *
 * Definition of the outputs.  For board i and list position j with symmetry k = symmetries[j]:
 *   let (v_j, l_j[36], p_j[36]) be what qttt_evaluate writes as value, logits and probs for qttt_transform(state_i, k);
 *   map the actions back: l_j'[a] = l_j[tau_k[a]], p_j'[a] = p_j[tau_k[a]] (tau_k of qttt_symmetry.h: action a of the
 *   board is action tau_k[a] of its image);
 *   value[i], logits[i][a] and probs[i][a] are each the arithmetic mean of the n_sym mapped-back images: summed in f32 as
 *   a balanced binary tree over the list positions, ((x0 + x1) + (x2 + x3)) + ((x4 + x5) + (x6 + x7)) for n_sym = 8
 *   (the left half of it for 4, x0 + x1 for 2, x0 for 1), then multiplied by 1.0f / n_sym (not at all for n_sym = 1).
 * n_sym is 1, 2, 4 or 8 — the sizes of the group's subgroups, the sets worth averaging over — so the scale is exact.
 * Consequences: n_sym = 1 with symmetry 0 gives qttt_evaluate's bits; eight equal images give that image's bits (2 x, 4 x
 * and 8 x are exact); an action that is masked is masked in every image, so its logit is -inf and its prob 0; a row whose
 * 36 actions are all masked has NaN probs; non-finite weights propagate as they do through qttt_evaluate.
 *
 * The kernel does not replay the mirrored game: the network's input reads only Board.board, the moves and the set of
 * squares in a qstruct, so the image's encoding is the board's with the block of square v written at sigma_k(v), and
 * its legal mask the mask of the permuted classical squares.  For every state that stepping reaches that is the encoding of
 * qttt_transform's image, bit for bit; the definition above is what the tests hold the kernel to.
 *
 *   state        n boards, not modified
 *   weights      the packed blob of qttt_nn.h for `precision`
 *   symmetries   HOST u8[n_sym], each 0..7, read during the call only
 *   sym          DEVICE u8[n], or NULL.  NULL: the mean over `symmetries`, as defined above.  Given: n_sym must be 1,
 *                `symmetries` is not read, and board i is evaluated under sym[i] alone and mapped back (an entry past 7
 *                is the identity, as in qttt_transform) — one random symmetry per evaluation, with the caller drawing
 *                the symmetries: the library adds no draw range for it.
 *   value f32[n], logits f32[n,36], probs f32[n,36]   each nullable, at least one given; only those given are written.
 *
 * Errors, in this order, before any device work: QTTT_ERR_SIZE for n < 0 (or n * 8 not representable), an unknown
 * precision, n_sym not 1, 2, 4 or 8, sym given with n_sym != 1, or (sym null, symmetries given) a list entry past 7; 0
 * with no device work for n == 0; QTTT_ERR_NULL for a null state or weights, for symmetries null while sym is null, or
 * for no output given; QTTT_ERR_ACTION for weights not 16-byte aligned or an output not 4-byte aligned. */
#ifndef QTTT_NN_SYMMETRIC_H
#define QTTT_NN_SYMMETRIC_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int qttt_evaluate_symmetric(const void *state, const void *weights, int precision,
                            const uint8_t *symmetries, int n_sym, const uint8_t *sym,
                            float *value, float *logits, float *probs, int64_t n, void *stream);

#ifdef __cplusplus
}
#endif
#endif
