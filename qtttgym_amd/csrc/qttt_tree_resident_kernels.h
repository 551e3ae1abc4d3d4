// qttt_tree_resident_kernels.h — the resident search of the device search trees (include/qttt_tree_resident.h, DESIGN.md
// §32): every round of a move's leaf-parallel search — select, network, backup, again — in ONE launch, where the rounds of
// qttt_tree_leaves.h are three launches each.  The only thing that connects the three is the game: a game's descents, its
// leaf rows and its backup touch that game's tree and nothing else, so the device-wide boundaries order nothing that a
// workgroup barrier does not.
//
// Mapping: evaluate_kernel's workgroup (256 threads, a network tile of M = NNCfg<PREC>::M rows) owns T = M / K games, the
// games [T * block, T * block + T), for the whole launch.  Row t * K + j of the tile is descent j of the tile's t-th game in
// every round; in the shorter last round of k < K the rows j >= k are dead, and so are the rows of games past `games` and the
// M - T * K rows that no game owns: zero rows of the encoding whose results go nowhere.  One round of k:
//   select   wave w runs tree_select_batch_game (qttt_tree_leaves_kernels.h, the body of qttt_tree_select_batch, with the
//            PUCT root or qttt_tree_forced_kernels.h's ForcedRootRule) for the tile's games w, w + 4, ...: the path records
//            and the leaves go to LDS;
//   network  nn_encode_row of the leaves, nn_hidden x 3, nn_head, nn_softmax_stats (qttt_nn_kernels.h, as
//            tree_value_rollout_kernel calls them): the head tile O stays in LDS;
//   backup   wave w runs tree_backup_batch_game<false> for the same games, the value read from O and the priors made by
//            nn_prob over O, as tree_value_rollout_kernel makes them.
// No body is copied: the three are the existing launches' own device functions.
//
// Order.  A game belongs to one wave for the whole launch, so what a wave's backup stored in the tree is read by the same
// wave's next select, behind tree_wave_sync() as between the descents of one launch.  Between waves only LDS is shared:
// the barrier after the select publishes the records and the leaves to the encoding, the one after the encoding (and those
// inside the layers) order the tile, the one after the softmax statistics publishes O to the backup, and the next round's
// select writes only its own games' records, which no other wave reads before the barrier that follows it.  That barrier
// also separates every wave's reads of O from the next encoding, which overwrites it.  __syncthreads() is a workgroup-scope
// fence and barrier; nothing is handed between workgroups, nothing waits on memory, there are no atomics and the grid is
// correct at any occupancy.
//
// Barriers.  EVERY wave reaches EVERY barrier of EVERY round: the round loop's trip count is made of kernel arguments
// alone, the per-game work is guarded (`if (g < games)` around the call, wave-uniform), never the wave — a wave whose games
// lie past `games`, a wave with no game at all (T < 4, e.g. K = 64 in f32), and a game with a terminal root all run the
// same barriers.  The loops inside a round keep their bounds: K <= 64 descents, depth <= QTTT_TREE_MAX_DEPTH, the layers'
// compile-time trip counts.
//
// LDS (per workgroup; DESIGN.md §32 has the budget against evaluate_kernel's two workgroups per CU): the activation tile,
// legal / rmax / rsum as evaluate_kernel, the 2 KB line table, M path records of 64 B and M leaves of 16 B.  Plain vector
// stores only.
#ifndef QTTT_TREE_RESIDENT_KERNELS_H
#define QTTT_TREE_RESIDENT_KERNELS_H
#include "qttt_tree_forced_kernels.h"
#include "qttt_tree_resident_host.h"
#include "qttt_tree_resident.h"

namespace {

static_assert(NNCfg<0>::M == 64 && NNCfg<1>::M == 128, "resident_tile_rows (qttt_tree_resident_host.h) restates the tiles");

// The lane's index in its wave, made here by two instructions (v_mbcnt counts the lanes below this one whatever EXEC holds)
// that the optimiser can neither hoist nor merge.  Each of a round's three parts starts from a lane index of its own (the
// network also from the weights' base passed through an empty asm statement): what a part computes of them — the layers'
// several hundred fragment and tile addresses, the backup's record addresses — is then made inside the part, as in the
// launch it comes from.  Hoisted out of the round loop and kept alive across the other two parts they took every register
// of the file and scratch besides; a lane index made anew costs two instructions and keeps no register
// alive across the layers, which threadIdx.x would.
__device__ __forceinline__ u32 resident_lane() {
    u32 x;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(x));
    return x;
}

// FORCED: the forced root rule of include/qttt_tree_forced.h with factor forced_k; else the plain PUCT root.
// The launch bounds' second figure is waves per SIMD: f32 is held to the 256 registers of two workgroups per CU (it takes 145);
// bf16, whose layers alone take 228, fits that line only by a register or two that move with the compiler's flags (8 B of
// scratch under some), so it is left its registers and runs one workgroup per CU.
template <int PREC, bool FORCED>
__global__ __launch_bounds__(QTTT_NN_BLOCK, PREC == 0 ? 2 : 1) void tree_search_resident_kernel(void *tree, int64_t games, int64_t capacity,
                                                                             u64 seed, u32 rollout_idx0, u32 leaves,
                                                                             u32 rollouts, u64 board_offset, double c_puct,
                                                                             double vloss, double forced_k,
                                                                             const void *weights) {
    typedef NNCfg<PREC> C;
    typedef typename C::T T;
    typedef NNBlob<PREC> L;
    static_assert(C::M * QTTT_NN_OUT_LD * 4 <= C::M * C::LD * (int)sizeof(T), "head tile must fit over the activations");
    static_assert(QTTT_NN_BLOCK == TREE_BLOCK && C::M <= QTTT_NN_BLOCK && QTTT_TREE_MAX_LEAVES <= NNCfg<0>::M, "one mapping");
    __shared__ __attribute__((aligned(16))) T H[C::M * C::LD];
    __shared__ __attribute__((aligned(16))) TreePathRec paths[C::M];
    __shared__ u64 leafP[C::M], leafQ[C::M], legal[C::M];
    __shared__ float rmax[C::M], rsum[C::M];
    __shared__ __attribute__((aligned(16))) uint8_t lut[LINE_LUT_BYTES];
    fill_line_lut<QTTT_NN_BLOCK>(lut);                           // ends with the workgroup barrier
    const u32 uwave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // the tree parts' loops are scalar
    const u32 tile_games = (u32)C::M / leaves;                   // T of include/qttt_tree_resident.h
    const int64_t g0 = (int64_t)blockIdx.x * tile_games;
    const T *W = reinterpret_cast<const T *>(weights);
    const TreeView v = tree_view(tree, games, capacity);
    float *O = reinterpret_cast<float *>(H);
    const auto value_of = [&](int64_t row) { return O[row * QTTT_NN_OUT_LD + 36]; };
    const auto prob_of = [&](int64_t row, u32 a) {
        const u64 lm = legal[row];
        return nn_prob(O[row * QTTT_NN_OUT_LD + a], lm >> a & 1ull, lm, rmax[row], rsum[row]);
    };

    u32 idx = rollout_idx0;
    for (u32 done = 0; done < rollouts;) {                       // uniform over the grid: kernel arguments alone
        const u32 k = resident_round(leaves, rollouts, done);
        // row b of the tile is live in this round: descent j < k of a game of the tile that exists
        const auto live = [&](u32 b) {
            const u32 t = b / leaves, j = b - t * leaves;
            return t < tile_games && g0 + t < games && j < k;
        };

        // ---- select: wave w for the tile's games w, w + 4, ...
        const u32 sl = resident_lane();
        for (u32 t = uwave; t < tile_games; t += TREE_GAMES_PER_BLOCK) {
            const int64_t g = g0 + t;
            if (g >= games) continue;                            // the work is guarded, not the wave
            const int64_t row0 = (int64_t)(t * leaves);
            if constexpr (FORCED) {
                const float *row = v.prior(g, v.games[g].root);  // select never moves the root
                tree_select_batch_game(v, g, row0, sl, lut, seed, idx, k, board_offset, c_puct, vloss, paths, leafP, leafQ,
                                       [&](u32) { return ForcedRootRule{row, forced_k, c_puct, vloss}; });
            } else {
                tree_select_batch_game(v, g, row0, sl, lut, seed, idx, k, board_offset, c_puct, vloss, paths, leafP, leafQ,
                                       [](u32) { return TreePuctRoot(); });
            }
        }
        __syncthreads();                                         // the records and the leaves; every read of the last O

        // ---- the network, as tree_value_rollout_kernel
        const T *Wr = W;
        asm volatile("" : "+s"(Wr));                             // a base of the round's own: see resident_lane
        const u32 tr = uwave * 64u + resident_lane();
        const float *bias = reinterpret_cast<const float *>(Wr + L::END);
        const u32 nwave = tr >> 6, nlane = tr & 63u;
        for (u32 b = tr >> 2; b < (u32)C::M; b += QTTT_NN_BLOCK / 4)
            nn_encode_row<PREC>(H + b * C::LD, legal, b, live(b), leafP, leafQ, 0, tr & 3u);
        __syncthreads();
        nn_hidden<PREC>(Wr + L::W1, bias, C::K1 / C::KS, H, nwave, nlane);
        nn_hidden<PREC>(Wr + L::W2, bias + QTTT_NN_HIDDEN, QTTT_NN_HIDDEN / C::KS, H, nwave, nlane);
        nn_hidden<PREC>(Wr + L::W3, bias + 2 * QTTT_NN_HIDDEN, QTTT_NN_HIDDEN / C::KS, H, nwave, nlane);
        nn_head<PREC>(Wr + L::WH, bias + 3 * QTTT_NN_HIDDEN, H, O, nwave, nlane);
        if (tr < (u32)C::M && live(tr)) nn_softmax_stats(O + tr * QTTT_NN_OUT_LD, legal[tr], rmax[tr], rsum[tr]);
        __syncthreads();

        // ---- backup: the same wave for the same games
        const u32 bl = resident_lane();
        for (u32 t = uwave; t < tile_games; t += TREE_GAMES_PER_BLOCK) {
            const int64_t g = g0 + t;
            if (g >= games) continue;
            tree_backup_batch_game<false>(v, g, (int64_t)(t * leaves), bl, capacity, k, paths, value_of, prob_of);
        }
        done += k;
        idx += k;
    }
}

}  // namespace

#endif  // QTTT_TREE_RESIDENT_KERNELS_H
