// qttt_tree_explore_kernels.h — root exploration for self-play (include/qttt_tree_explore.h): Dirichlet
// noise mixed into the roots' priors, and the move drawn from the roots' visit counts.
//
// Mapping: the tree kernels' (qttt_tree_kernels.h): ONE WAVEFRONT PER GAME, lane a = action a, TREE_BLOCK threads.  A
// lane draws the Gamma variate of its own action (the draws are addressed by (noise_idx, a), so every lane makes its
// own launch keys), the normalising sum is the record's six-step butterfly, and the root's prior row is one coalesced
// 144-byte store.  A wave writes only its own game's root: no atomics, no LDS, nothing handed from lane to lane through
// memory.  The one loop is the Marsaglia-Tsang try loop, bounded by QTTT_TREE_NOISE_TRIES; it ends early on the
// wave-uniform "every lane accepted".  explore_sample_move is the sampled record's move: an inclusive scan over the
// wave and one ballot (selfplay_record_kernel<RECORD_SAMPLED>, qttt_selfplay_kernels.h).
#ifndef QTTT_TREE_EXPLORE_KERNELS_H
#define QTTT_TREE_EXPLORE_KERNELS_H
#include "qttt_tree_kernels.h"
#include "qttt_tree_explore.h"

namespace {

// qttt_hash(seed, board id folded to `id`, idx) on the device
__device__ __forceinline__ u64 explore_hash(u64 seed, u32 id, u32 idx) {
    const Draw d = counter_draw(id, launch_key(seed, idx));
    return ((u64)d.h2 << 32) | d.h1;
}
// the uniforms of include/qttt_tree_explore.h, both strictly inside (0, 1)
__device__ __forceinline__ double explore_u53(u64 h) { return ((double)(h >> 11) + 0.5) * 0x1p-53; }
__device__ __forceinline__ double explore_u32(u32 w) { return ((double)w + 0.5) * 0x1p-32; }

// the noise of one game's root (the wave's): the body of tree_root_noise_kernel, and of the subset form
// (qttt_tree_subset_kernels.h), whose wave w takes game ids[w]; the outputs' rows are the game's either way
__device__ __forceinline__ void tree_root_noise_game(const TreeView &v, int64_t g, u32 lane, u64 seed, u32 noise_idx,
                                                     u64 board_offset, double epsilon, double alpha, double *noise,
                                                     uint8_t *applied) {
#pragma clang fp contract(off)
    const int32_t root = v.games[g].root;
    const TreeNodeHdr h = *v.hdr(g, root);
    const bool legal = lane < 36u && ((h.legal >> lane) & 1ull);
    bool noised = (h.flags & TN_PRIORS) && !(h.flags & TN_TERMINAL) && h.legal != 0ull;      // wave-uniform
    double n = 0.0;
    if (noised) {
        // Gamma(alpha) of this lane's action, Marsaglia-Tsang
        const double a1 = alpha < 1.0 ? alpha + 1.0 : alpha;
        const double d = a1 - 1.0 / 3.0, c = 1.0 / __builtin_sqrt(9.0 * d);
        const u32 id = fold_id(board_offset + (u64)g);
        const u32 base = QTTT_TREE_NOISE_BASE + (noise_idx * 36u + lane) * (u32)QTTT_TREE_NOISE_DRAWS;
        double y = legal ? a1 : 0.0;
        bool pending = legal;
        for (u32 t = 0; t < (u32)QTTT_TREE_NOISE_TRIES; ++t) {
            if (!__ballot(pending)) break;
            const u64 h0 = explore_hash(seed, id, base + 2u * t), h1 = explore_hash(seed, id, base + 2u * t + 1u);
            const double x = __builtin_sqrt(-2.0 * log(explore_u53(h0))) * cos(6.283185307179586 * explore_u32((u32)(h1 >> 32)));
            const double u = 1.0 + c * x;
            const double w = u * u * u;
            const bool accept = w > 0.0 && log(explore_u32((u32)h1)) < 0.5 * x * x + d - d * w + d * log(w);
            if (pending && accept) { y = d * w; pending = false; }
        }
        if (alpha < 1.0 && legal) y = y * pow(explore_u53(explore_hash(seed, id, base + 2u * (u32)QTTT_TREE_NOISE_TRIES)), 1.0 / alpha);
        const double S = selfplay_wave_sum(y);
        noised = S != 0.0 && __builtin_isfinite(S);
        if (noised) {
            n = y / S;                                           // 0 at illegal actions
            const double p = legal ? tree_prior(v, g, root, h, lane) : 0.0;
            if (lane < 36u) v.prior(g, root)[lane] = legal ? (float)((1.0 - epsilon) * p + epsilon * n) : 0.0f;
            if (lane == 0u && (h.flags & TN_UNIFORM)) v.hdr(g, root)->flags = h.flags & ~TN_UNIFORM;
        }
    }
    if (noise && lane < 36u) noise[g * 36 + lane] = n;
    if (applied && lane == 0u) applied[g] = noised ? 1 : 0;
}

__global__ __launch_bounds__(TREE_BLOCK) void tree_root_noise_kernel(void *tree, int64_t games, int64_t capacity, u64 seed,
                                                                     u32 noise_idx, u64 board_offset, double epsilon,
                                                                     double alpha, double *noise, uint8_t *applied) {
    const int64_t g = (int64_t)blockIdx.x * TREE_GAMES_PER_BLOCK + threadIdx.x / 64;
    const u32 lane = threadIdx.x & 63u;
    if (g >= games) return;
    tree_root_noise_game(tree_view(tree, games, capacity), g, lane, seed, noise_idx, board_offset, epsilon, alpha, noise, applied);
}

// The sampled record's move (include/qttt_tree_explore.h): lane a holds action a of a live root that is not terminal,
// N its visit count (0 where the action is illegal and in lanes 36..63).  Every lane ends with the move, or with -1
// where the caller falls back to choose (no visit at all, or a total that is not finite).
__device__ __forceinline__ int explore_sample_move(u32 N, u32 lane, u64 seed, u64 board_id, int ply, double temperature) {
#pragma clang fp contract(off)
    double w = 0.0;
    if (N) w = temperature == 1.0 ? (double)N : pow((double)N, 1.0 / temperature);
    double c = w;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const double below = __shfl_up(c, m);
        if ((int)lane >= m) c = c + below;
    }
    const double T = __shfl(c, 63);
    if (!(T != 0.0 && __builtin_isfinite(T))) return -1;
    const u64 h = explore_hash(seed, fold_id(board_id), QTTT_SELFPLAY_MOVE_BASE + (u32)ply);
    const double t = ((double)(h >> 11) * 0x1p-53) * T;
    const u64 hit = __ballot(w > 0.0 && t < c);
    return hit ? (int)__builtin_ctzll(hit) : -1;
}

}  // namespace

#endif  // QTTT_TREE_EXPLORE_KERNELS_H
