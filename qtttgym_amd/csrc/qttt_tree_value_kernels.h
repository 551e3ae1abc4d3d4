// qttt_tree_value_kernels.h — the value rollout of the device search trees (include/qttt_tree_value.h):
// the leaves that qttt_tree_select wrote are evaluated by the policy/value network and the result is backed up, in ONE
// launch.  The leaf's value comes from the value head and its priors from the policy head of the same evaluation, where
// the playout rollout (qttt_rollout_policy -> qttt_tree_backup) plays n_sims network-guided games to the end.
//
// Mapping: evaluate_kernel's (qttt_nn_kernels.h), with its device functions as they are: a 256-thread workgroup owns a
// tile of NNCfg<PREC>::M games, encodes their leaves into LDS, runs the trunk and the head on the matrix cores and leaves
// the head tile O in LDS, so value and probs are the bits qttt_evaluate gives.  The tree epilogue then works from O: wave
// w takes the tile's games w, w + 4, ..., one game at a time as tree_backup_kernel does (lane d = the d-th edge of the
// path, lane a = the prior of action a), with the edge update and the priors rule that kernel uses
// (tree_edge_load / tree_edge_store / tree_leaf_priors).  A game belongs to one wave: no atomics.  The games of a wave are
// taken TREE_VALUE_CHUNK at a time, every load of a chunk issued before its first store: the epilogue is a chain of
// dependent HBM accesses per game (path -> slot -> store), and a wave that walked its 16 / 32 games one after the other
// would spend longer in it than the bf16 network takes.  What select left in the game header (depth, leaf) is fetched
// into LDS before the matrix work, so that its latency hides behind it: 5 bytes per game.
//
// The value v is seen by the player to move at the leaf.  Not terminal: v = (double)value_f32, whatever it is: a NaN or
// an infinity goes into W as it is (select's comparisons with it then fail, as torch's would; nothing here branches or
// loops on it).  Terminal: the network's row is not consulted; v is the game's reward from the node's winner flag, True
// -> +1 if the leaf's turn is True else -1, False -> the opposite, None -> 0: what playouts from a terminal leaf back up.
// Rows past `games` in the last tile are zero rows whose results go nowhere.  Every loop is bounded by a compile-time
// count (the tile's games per wave); the path depth is clamped to QTTT_TREE_MAX_DEPTH.
#ifndef QTTT_TREE_VALUE_KERNELS_H
#define QTTT_TREE_VALUE_KERNELS_H
#include "qttt_tree_kernels.h"
#include "qttt_nn_kernels.h"
#include "qttt_tree_value.h"

namespace {

constexpr int TREE_VALUE_CHUNK = 4;                              // games of one wave whose loads are in flight together

// the reward of a terminal leaf for the player to move there, from the node's flags (winner + 1 in bits 8-9)
__device__ __forceinline__ double tree_terminal_value(u32 node_flags) {
    const u32 w = (node_flags >> 8) & 3u;                        // 0 None, 1 False, 2 True
    if (w == 0u) return 0.0;
    return ((w == 2u) == ((node_flags & TN_TURN) != 0u)) ? 1.0 : -1.0;
}

template <int PREC>
__global__ __launch_bounds__(QTTT_NN_BLOCK) void tree_value_rollout_kernel(void *tree, int64_t games, int64_t capacity,
                                                                           const u64 *leafP, const u64 *leafQ,
                                                                           const void *weights, float *leaf_value,
                                                                           float *leaf_probs) {
    typedef NNCfg<PREC> C;
    typedef typename C::T T;
    typedef NNBlob<PREC> L;
    static_assert(C::M * QTTT_NN_OUT_LD * 4 <= C::M * C::LD * (int)sizeof(T), "head tile must fit over the activations");
    static_assert(C::M % (4 * TREE_VALUE_CHUNK) == 0, "whole chunks per wave");
    __shared__ __attribute__((aligned(16))) T H[C::M * C::LD];
    __shared__ u64 legal[C::M];
    __shared__ float rmax[C::M], rsum[C::M];
    __shared__ int32_t g_leaf[C::M];                             // the game headers' leaf and depth
    __shared__ uint8_t g_depth[C::M];
    const u32 tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const int64_t base = (int64_t)blockIdx.x * C::M;
    const u32 valid = (u32)min((int64_t)C::M, games - base);
    const T *W = reinterpret_cast<const T *>(weights);
    const float *bias = reinterpret_cast<const float *>(W + L::END);
    const TreeView v = tree_view(tree, games, capacity);

    if (tid < valid) {                                           // what select left; in flight during the encoding
        const TreeGame *gh = &v.games[base + tid];
        const int32_t depth = gh->depth;
        g_leaf[tid] = gh->leaf;
        g_depth[tid] = (uint8_t)(depth < 0 ? 0 : depth > QTTT_TREE_MAX_DEPTH ? QTTT_TREE_MAX_DEPTH : depth);
    }
    for (u32 b = tid >> 2; b < (u32)C::M; b += QTTT_NN_BLOCK / 4)
        nn_encode_row<PREC>(H + b * C::LD, legal, b, b < valid, leafP, leafQ, base, tid & 3u);
    __syncthreads();

    // ---- the network, as evaluate_kernel
    nn_hidden<PREC>(W + L::W1, bias, C::K1 / C::KS, H, wave, lane);
    nn_hidden<PREC>(W + L::W2, bias + QTTT_NN_HIDDEN, QTTT_NN_HIDDEN / C::KS, H, wave, lane);
    nn_hidden<PREC>(W + L::W3, bias + 2 * QTTT_NN_HIDDEN, QTTT_NN_HIDDEN / C::KS, H, wave, lane);
    float *O = reinterpret_cast<float *>(H);
    nn_head<PREC>(W + L::WH, bias + 3 * QTTT_NN_HIDDEN, H, O, wave, lane);
    if (tid < valid) nn_softmax_stats(O + tid * QTTT_NN_OUT_LD, legal[tid], rmax[tid], rsum[tid]);
    __syncthreads();
    const auto prob = [&](u32 b, u32 a) {
        const u64 lm = legal[b];
        return nn_prob(O[b * QTTT_NN_OUT_LD + a], lm >> a & 1ull, lm, rmax[b], rsum[b]);
    };
    if (leaf_value)
        for (u32 b = tid; b < valid; b += QTTT_NN_BLOCK) leaf_value[base + b] = O[b * QTTT_NN_OUT_LD + 36u];
    if (leaf_probs) {
        const u32 cnt = valid * 36u;
        for (u32 k = tid; k < cnt; k += QTTT_NN_BLOCK) leaf_probs[base * 36 + k] = prob(k / 36u, k % 36u);
    }

    // ---- the tree epilogue: _backpropogate and the leaf's priors, wave w for the games w, w + 4, ... of the tile
    for (int i = 0; i < C::M / (4 * TREE_VALUE_CHUNK); ++i) {
        TreeEdge e[TREE_VALUE_CHUNK];
        u32 lf[TREE_VALUE_CHUNK];
        int32_t depth[TREE_VALUE_CHUNK];
#pragma unroll
        for (int c = 0; c < TREE_VALUE_CHUNK; ++c) {
            const u32 b = wave + 4u * (u32)(i * TREE_VALUE_CHUNK + c);
            const bool live = b < valid;                         // wave-uniform
            depth[c] = live ? (int32_t)g_depth[b] : 0;
            e[c] = tree_edge_load(v, base + b, &v.games[live ? base + b : 0], depth[c], lane);
            lf[c] = live ? v.hdr(base + b, g_leaf[b])->flags : (u32)TN_TERMINAL;
        }
#pragma unroll
        for (int c = 0; c < TREE_VALUE_CHUNK; ++c) {
            const u32 b = wave + 4u * (u32)(i * TREE_VALUE_CHUNK + c);
            if (b >= valid) continue;
            const double val = (lf[c] & TN_TERMINAL) ? tree_terminal_value(lf[c]) : (double)O[b * QTTT_NN_OUT_LD + 36u];
            tree_edge_store(e[c], depth[c], lane, val);
            tree_leaf_priors(v, base + b, g_leaf[b], lf[c], lane, true, [&](u32 a) { return prob(b, a); });
        }
    }
}

}  // namespace

#endif  // QTTT_TREE_VALUE_KERNELS_H
