// qttt_policy_rollout_kernels.h — AlphaZero._simulate (alphazero.py:192-205) under the policy/value network for a batch of
// (board, simulation) lanes in ONE launch: every ply runs Model.forward(node.to_vector()) (get_action_probs, :294-300),
// samples an action from Categorical(logits) (sample_action, :302-303) and one collapse child (:202), until the game
// ends.  The network part is evaluate_kernel's (qttt_nn_kernels.h: the same encode, trunk, head, mask and softmax
// functions on the same tile mapping); the draw, the stopping rule, the step and the reward are the uniform playout's
// (qttt_search_core.h).
//
// Mapping: a 256-thread workgroup owns a tile of M lanes (64 f32 / 128 bf16), lane j = i * n_sims + s
// plays simulation s of board i (rollout_many_kernel's order).  The tile's packed states stay in LDS for the whole launch
// and thread b < M owns lane b: its state in registers, its draws and its step.  A ply: the to_vector rows in LDS, the
// trunk and the head on the matrix cores, then every live lane samples and steps.  Finished lanes keep their rows until
// the tile ends (no compaction); the loop ends after 9 plies or once no lane of the tile is live (a workgroup-uniform
// test).  Draws: ply p of lane (i, s) uses qttt_hash(seed, board_offset + i, step_idx0 + s * QTTT_SIM_STRIDE + p) =
// (h1, h2): collapse bit h1 >> 31, u = (h2 >> 8) * 2^-24, action = the first legal a whose running exp-sum exceeds u * S
// (include/qttt_policy_rollout.h).  Bounded loops, no atomics, no scratch.
#ifndef QTTT_POLICY_ROLLOUT_KERNELS_H
#define QTTT_POLICY_ROLLOUT_KERNELS_H
#include "qttt_nn_kernels.h"
#include "qttt_search_core.h"

namespace {

// Categorical(logits).sample() by inverse CDF on the head row o with legal mask lm (not empty) and nn_softmax_stats' max
// and exp-sum: the smallest legal a whose running sum of expf(o[a] - mx), in ascending action order (the order of `sum`),
// exceeds u * sum; the largest legal a if rounding leaves none.
__device__ __forceinline__ u32 nn_sample_action(const float *o, u64 lm, float mx, float sum, u32 h2) {
    const float target = (float)(h2 >> 8) * 0x1p-24f * sum;
    float c = 0.f;
    u32 pick = 36u;
    for (u32 a = 0; a < 36u; ++a)
        if (lm >> a & 1ull) {
            c += expf(o[a] - mx);
            if (pick == 36u && c > target) pick = a;
        }
    return pick < 36u ? pick : 63u - (u32)__builtin_clzll(lm);
}

// true in every thread iff v holds in any thread of the workgroup; ends with a barrier.  `wflags` = one word per wave.
__device__ __forceinline__ bool workgroup_any(bool v, u32 *wflags) {
    const u64 b = __ballot(v);
    if ((threadIdx.x & 63u) == 0u) wflags[threadIdx.x >> 6] = b != 0ull ? 1u : 0u;
    __syncthreads();
    u32 any = 0;
#pragma unroll
    for (u32 w = 0; w < QTTT_NN_BLOCK / 64; ++w) any |= wflags[w];
    return any != 0u;
}

template <int PREC>
__global__ __launch_bounds__(QTTT_NN_BLOCK) void rollout_policy_kernel(
    const u64 *pP, const u64 *pQ, const void *weights, u64 seed, u32 step_idx0, u64 board_offset, u32 n_sims,
    int8_t *result, uint8_t *plies, uint8_t *trace, float *leaf_value, float *leaf_probs, int64_t n_lanes) {
    typedef NNCfg<PREC> C;
    typedef typename C::T T;
    typedef NNBlob<PREC> L;
    __shared__ __attribute__((aligned(16))) T H[C::M * C::LD];
    __shared__ __attribute__((aligned(16))) uint8_t lut[LINE_LUT_BYTES];
    __shared__ u64 sP[C::M], sQ[C::M], legal[C::M];
    __shared__ float rmax[C::M], rsum[C::M];
    __shared__ u32 wflags[QTTT_NN_BLOCK / 64];
    const u32 tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const int64_t base = (int64_t)blockIdx.x * C::M;
    const u32 valid = (u32)min((int64_t)C::M, n_lanes - base);
    const bool want_leaf = leaf_value != nullptr || leaf_probs != nullptr;

    // ---- thread b < valid owns lane base + b for the whole launch
    const bool owner = tid < valid;
    const int64_t j = base + tid;
    int64_t board = 0;
    u32 sim = 0, P0 = 0, P1 = 0, Q0 = 0, Q1 = 0, id = 0, t0 = 0, played = 0;
    bool alive = false;
    if (owner) {
        board = j / n_sims;
        sim = (u32)(j - board * n_sims);
        const u64 P = pP[board], Q = pQ[board];               // n_sims neighbouring lanes read the same 16 bytes
        P0 = (u32)P; P1 = (u32)(P >> 32); Q0 = (u32)Q; Q1 = (u32)(Q >> 32);
        sP[tid] = P;
        sQ[tid] = Q;
        id = fold_id(board_offset + (u64)board);
        t0 = step_idx0 + sim * QTTT_SIM_STRIDE;
        alive = playout_live(P1);
    }
    fill_line_lut<QTTT_NN_BLOCK>(lut);                          // ends with the workgroup barrier
    float *O = reinterpret_cast<float *>(H);

#pragma unroll 1
    for (u32 p = 0; p < PLAYOUT_PLIES; ++p) {
        // workgroup-uniform; ply 0 also runs for a tile of finished lanes when the leaf outputs are wanted.  The barrier
        // orders the previous ply's O reads and state writes before this ply's encode.
        if (!workgroup_any(alive, wflags) && !(p == 0u && want_leaf)) break;
        for (u32 b = tid >> 2; b < (u32)C::M; b += QTTT_NN_BLOCK / 4)
            nn_encode_row<PREC>(H + b * C::LD, legal, b, b < valid, sP, sQ, 0, tid & 3u);
        __syncthreads();
        // the weights are the same every ply: an opaque copy of their address keeps the compiler from hoisting their loads
        // out of the ply loop (it did, into spills: 256 VGPRs and scratch)
        u64 waddr = (u64)weights;
        asm volatile("" : "+s"(waddr));
        const T *W = reinterpret_cast<const T *>(waddr);
        const float *bias = reinterpret_cast<const float *>(W + L::END);
        nn_hidden<PREC>(W + L::W1, bias, C::K1 / C::KS, H, wave, lane);
        nn_hidden<PREC>(W + L::W2, bias + QTTT_NN_HIDDEN, QTTT_NN_HIDDEN / C::KS, H, wave, lane);
        nn_hidden<PREC>(W + L::W3, bias + 2 * QTTT_NN_HIDDEN, QTTT_NN_HIDDEN / C::KS, H, wave, lane);
        nn_head<PREC>(W + L::WH, bias + 3 * QTTT_NN_HIDDEN, H, O, wave, lane);

        if (owner) {
            const float *o = O + tid * QTTT_NN_OUT_LD;
            const u64 lm = legal[tid];
            float mx, sum;
            nn_softmax_stats(o, lm, mx, sum);
            if (p == 0u) {                                      // the leaf's node.P and value (alphazero.py:197-198)
                rmax[tid] = mx;
                rsum[tid] = sum;
                if (leaf_value && sim == 0u) leaf_value[board] = o[36];
            }
            if (alive) {
                const Draw d = counter_draw(id, launch_key(seed, t0 + p));
                const u32 a = nn_sample_action(o, lm, mx, sum, d.h2), bit = d.h1 >> 31;
                step_core<false, true>(P0, P1, Q0, Q1, pair_action<false>(a), bit, lut);   // legal and sorted
                if (trace) trace[j * PLAYOUT_PLIES + p] = (uint8_t)(a | bit << 6);
                played += 1u;
                sP[tid] = (u64)P0 | ((u64)P1 << 32);
                sQ[tid] = (u64)Q0 | ((u64)Q1 << 32);
                alive = playout_live(P1);
            }
        }
        if (p == 0u && leaf_probs) {                            // evaluate_kernel's probs rows, for the s == 0 lanes
            __syncthreads();
            for (u32 k = tid; k < valid * 36u; k += QTTT_NN_BLOCK) {
                const u32 b = k / 36u, a = k - b * 36u;
                const int64_t jb = base + b, i = jb / n_sims;
                if (jb != i * n_sims) continue;
                const u64 lm = legal[b];
                leaf_probs[i * 36 + a] = nn_prob(O[b * QTTT_NN_OUT_LD + a], lm >> a & 1ull, lm, rmax[b], rsum[b]);
            }
        }
    }

    if (!owner) return;
    int w, t;
    lite_update_winner(lite_unpack((u64)P0 | ((u64)P1 << 32)), lut, w, t);
    result[j] = (int8_t)reward_of_winner(w);
    if (plies) plies[j] = (uint8_t)played;
    if (trace)
        for (u32 p = played; p < PLAYOUT_PLIES; ++p) trace[j * PLAYOUT_PLIES + p] = 0xFFu;
}

}  // namespace

#endif  // QTTT_POLICY_ROLLOUT_KERNELS_H
