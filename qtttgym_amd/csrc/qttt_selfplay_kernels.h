// qttt_selfplay_kernels.h — the self-play record (include/qttt_selfplay.h): one root of every game of
// the device search trees becomes one row of the trainer's batch, and the move to play comes back.
//
// Mapping: the tree kernels' (qttt_tree_kernels.h): ONE WAVEFRONT PER GAME, lane a = action a.  The root's 36 slots
// are one coalesced 576-byte read, the pi row one coalesced 288-byte store, the mask row 36 bytes; the value back-fill
// of a finished game is at most 10 lanes, one row each.  The tree is read only; a wave touches only its own game's
// columns of the outputs, so there are no atomics, and nothing is handed from lane to lane through memory.  No LDS
// (the winner and the terminal flag are the root's node flags, no line table is needed), no loop but the two six-step
// butterflies (the sum, and choose's argmax).
// selfplay_record_kernel<RECORD_SAMPLED> is the sampled record of include/qttt_tree_explore.h: the same kernel with the
// move of the first plies drawn from the visit counts (explore_sample_move); <RECORD_GUMBEL> is the Gumbel record of
// include/qttt_tree_gumbel.h: the move and the pi row are gumbel_final's (qttt_tree_gumbel_kernels.h), two more
// butterflies and one exp per lane; <RECORD_PLAIN> is qttt_selfplay_record's, whose code the mode does not touch;
// <RECORD_PRUNED> is the pruned record of include/qttt_tree_forced.h: the sampled record whose pi row is made of forced_root's
// pruned visit counts (qttt_tree_forced_kernels.h), the other three instantiations compiling to what they were without it
// (profiles/forced/kernel_resources.txt).
// selfplay_record_kernel<MODE, true> is the stream record of include/qttt_selfplay_stream.h: the same body with the row
// read per game from length[g]; the lockstep instantiations compile to what they were without it
// (profiles/stream/record_kernels_before_after.txt).  A root's row is written by selfplay_row_head and, at a terminal
// root, selfplay_terminal_row: the harvest (qttt_selfplay_stream_kernels.h) writes its terminal rows through the same two.
#ifndef QTTT_SELFPLAY_KERNELS_H
#define QTTT_SELFPLAY_KERNELS_H
#include "qttt_tree_kernels.h"
#include "qttt_tree_explore_kernels.h"
#include "qttt_tree_gumbel_kernels.h"
#include "qttt_tree_forced_kernels.h"
#include "qttt_selfplay.h"
#include "qttt_selfplay_record_host.h"

namespace {

struct SelfPlayOut {
    u64 *states;                       // [ROWS][2][plane_stride(games)]
    double *pi;                        // [ROWS][games][36]
    uint8_t *mask;                     // [ROWS][games][36]
    uint8_t *done;                     // [ROWS][games]
    float *v;                          // [ROWS][games]
    uint8_t *action36;                 // [ROWS][games]
    uint8_t *length;                   // [games]
    int8_t *winner;                    // [games]
    uint8_t *actions;                  // [games][2]
};

// what the sampled and the Gumbel record take besides: nothing at all in the plain one
template <int MODE>
struct SelfPlaySampling {};
template <>
struct SelfPlaySampling<RECORD_SAMPLED> {
    u64 seed, board_offset;
    double temperature;
    int sample_plies;
};
template <>
struct SelfPlaySampling<RECORD_GUMBEL> {
    const GumbelRec *recs;
    double c_visit, c_scale;
};
template <>
struct SelfPlaySampling<RECORD_PRUNED> {                         // the sampled record's, then the prune's
    u64 seed, board_offset;
    double temperature;
    int sample_plies;
    double forced_k, c_puct;
};

// what every recorded root writes first: its packed state, the done byte and the game's new length
// (stride = plane_stride(games), row = ply * games + g: the caller's, which it needs itself)
__device__ __forceinline__ void selfplay_row_head(const SelfPlayOut &o, int64_t stride, int64_t row, int64_t g, int ply,
                                                  const TreeNodeHdr &h, bool terminal, u32 lane) {
    if (lane == 0u) {
        u64 *planes_t = o.states + (int64_t)ply * 2 * stride;
        planes_t[g] = h.P;
        planes_t[stride + g] = h.Q;
        o.done[row] = terminal ? 1 : 0;
        o.length[g] = (uint8_t)(ply + 1);
    }
}

// the rest of a terminal root's row (self_play.py:203-206) and the v of the whole game (:195-216).  BY_STATE
// (include/qttt_selfplay_cap.h: batches in which not every ply is a row): row r is signed by the side to move in row r's
// recorded state, the first player's rows get v0; where every ply is a row that is the row's parity, the default's bits.
template <bool BY_STATE = false>
__device__ __forceinline__ void selfplay_terminal_row(const SelfPlayOut &o, int64_t games, int64_t row, int64_t g, int ply,
                                                      const TreeNodeHdr &h, float v_first, float v_second, u32 lane) {
    uint8_t *act = o.actions + 2 * g;
    if (lane < 36u) {
        o.pi[row * 36 + lane] = 1.0 / 36.0;
        o.mask[row * 36 + lane] = 1;
    }
    const int w = (int)((h.flags >> 8) & 3u) - 1;                // 1 / 0 / -1 = True / False / None
    const float v0 = w > 0 ? v_first : (w == 0 ? v_second : 0.0f);
    if ((int)lane <= ply) {
        u32 odd = lane & 1u;
        if constexpr (BY_STATE) {                                // this row's state is h's, written by lane 0 just now
            const u64 P = (int)lane == ply ? h.P : o.states[(int64_t)lane * 2 * plane_stride(games) + g];
            odd = ((u32)(P >> 32) >> P1_N_SHIFT) & 1u;           // the moves played (no autofill move among them)
        }
        const float x = odd ? -v0 : v0;
        o.v[(int64_t)lane * games + g] = x == 0.0f ? 0.0f : x;            // a zero is +0.0
    }
    if (lane == 0u) {
        o.winner[g] = (int8_t)w;
        o.action36[row] = 255;
        act[0] = 255; act[1] = 255;
    }
}

// One game's record (the wave's), the body of selfplay_record_kernel and of the capped record
// (qttt_selfplay_cap_kernels.h).  STREAM: `ply` is the index of the sampled move's draw and the row is the game's own ply,
// length[g]; a game whose terminal row is recorded (or whose ten rows are full) is not live.  CAPPED
// (include/qttt_selfplay_cap.h, STREAM only): a live game with full[g] == 0 whose root is not terminal writes its move to
// actions[g] and nothing else, and the finished game's v is signed by the rows' states; full is not read otherwise.
template <int MODE, bool STREAM, bool CAPPED>
__device__ __forceinline__ void selfplay_record_game(const void *tree, int64_t games, int64_t capacity, int ply, u32 n_rollouts,
                                                     double alpha, float v_first, float v_second, const SelfPlayOut &o,
                                                     const SelfPlaySampling<MODE> &sampling, const uint8_t *full, int64_t g,
                                                     u32 lane) {
    uint8_t *act = o.actions + 2 * g;
    const int draw = ply;
    if constexpr (STREAM) {
        ply = (int)o.length[g];
        if (ply >= QTTT_SELFPLAY_ROWS || (ply != 0 && o.done[(int64_t)(ply - 1) * games + g] != 0)) {
            if (lane == 0u) { act[0] = 255; act[1] = 255; }
            return;
        }
    } else {
        // live: the row before this one was recorded and was not the terminal one
        if (ply != 0 && ((int)o.length[g] != ply || o.done[(int64_t)(ply - 1) * games + g] != 0)) {
            if (lane == 0u) { act[0] = 255; act[1] = 255; }
            return;
        }
    }
    const TreeView v = tree_view(const_cast<void *>(tree), games, capacity);
    const TreeRootLane r = tree_root_lane(v, g, lane);
    const int64_t stride = plane_stride(games), row = (int64_t)ply * games + g;
    const bool terminal = (r.h.flags & TN_TERMINAL) != 0u;
    bool fast = false;                                           // wave-uniform
    if constexpr (CAPPED) fast = !terminal && full[g] == 0;
    if (!fast) selfplay_row_head(o, stride, row, g, ply, r.h, terminal, lane);
    if (terminal) {
        selfplay_terminal_row<CAPPED>(o, games, row, g, ply, r.h, v_first, v_second, lane);
        return;
    }
    int a;
    double pi;
    if constexpr (MODE == RECORD_GUMBEL) {                       // the Gumbel choice and the improved policy
        const GumbelFinal f = gumbel_final(r, gumbel_lane(sampling.recs + g, lane), lane, sampling.c_visit, sampling.c_scale);
        a = f.choose;
        pi = f.pi;
    } else {
        // self_play.py:208-213: pi[a] = (N / n_rollouts) ** alpha on the legal actions, normalised
        u32 n_pi = r.s.N;
        if constexpr (MODE == RECORD_PRUNED) n_pi = forced_root(v, g, r, lane, sampling.forced_k, sampling.c_puct).n_pruned;
        double x = r.legal ? (double)n_pi / (double)n_rollouts : 0.0;
        if (alpha != 1.0) x = r.legal ? pow(x, alpha) : 0.0;
        const double sum = selfplay_wave_sum(x);
        a = tree_choose(r, lane);
        if constexpr (MODE == RECORD_SAMPLED || MODE == RECORD_PRUNED) {
            if (ply < sampling.sample_plies) {                   // wave-uniform
                const int drawn = explore_sample_move(r.s.N, lane, sampling.seed, sampling.board_offset + (u64)g, draw,
                                                      sampling.temperature);
                a = drawn < 0 ? a : drawn;
            }
        }
        pi = r.legal ? x / sum : 0.0;
    }
    if (lane < 36u && !fast) {
        o.pi[row * 36 + lane] = pi;
        o.mask[row * 36 + lane] = r.legal ? 1 : 0;
    }
    if (lane == 0u) {
        const u32 pr = a < 0 ? 0xFFFFu : pair_action<false>(a < 0 ? 0 : a);      // lo | hi << 8
        if (!fast) o.action36[row] = a < 0 ? (uint8_t)255 : (uint8_t)a;
        act[0] = (uint8_t)pr; act[1] = (uint8_t)(pr >> 8);
    }
}

template <int MODE, bool STREAM = false>
__global__ __launch_bounds__(TREE_BLOCK) void selfplay_record_kernel(const void *tree, int64_t games, int64_t capacity,
                                                                     int ply, u32 n_rollouts, double alpha, float v_first,
                                                                     float v_second, SelfPlayOut o,
                                                                     SelfPlaySampling<MODE> sampling) {
    const int64_t g = (int64_t)blockIdx.x * TREE_GAMES_PER_BLOCK + threadIdx.x / 64;
    const u32 lane = threadIdx.x & 63u;
    if (g >= games) return;
    selfplay_record_game<MODE, STREAM, false>(tree, games, capacity, ply, n_rollouts, alpha, v_first, v_second, o, sampling,
                                              nullptr, g, lane);
}

}  // namespace

#endif  // QTTT_SELFPLAY_KERNELS_H
