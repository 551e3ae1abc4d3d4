// qttt_selfplay_stream_kernels.h — continuous self-play (include/qttt_selfplay_stream.h): what lets a
// finished game hand its rows to the replay ring and start again in its slot while the other slots play on.
//
// Mapping: the record's (qttt_selfplay_kernels.h): ONE WAVEFRONT PER GAME, lane a = action a, TREE_BLOCK threads.
//   selfplay_record_kernel<MODE, true>  the record with the row read per game (the body is qttt_selfplay_kernels.h's)
//   selfplay_harvest_kernel   reads the root's 32-byte header; a terminal root's wave writes the terminal row and the
//                             value back-fill through selfplay_row_head / selfplay_terminal_row, the record's own, and
//                             one lane books the slot's tallies.  Every wave writes its own harvest_len and finished byte.
//   selfplay_restart_kernel   a finished slot's wave zeroes the slot's board and staging rows and writes the root that
//                             tree_reset_kernel writes for the empty board (the same tree_node_of on the same line table).
// A wave touches only its own slot's columns, tallies included (per-slot integers): no atomics, nothing handed from lane
// to lane through memory, no workgroup waits on another.  LDS: the restart's line table; the harvest has none.
#ifndef QTTT_SELFPLAY_STREAM_KERNELS_H
#define QTTT_SELFPLAY_STREAM_KERNELS_H
#include "qttt_selfplay_kernels.h"
#include "qttt_selfplay_stream.h"

namespace {

struct SelfPlayHarvest {
    uint8_t *harvest_len;              // [games]  the rows to append: length[g] of a slot that finished, else 0
    uint8_t *finished;                 // [games]  1 / 0
    int64_t *games_done;               // [games]  finished games of the slot, cumulative
    int64_t *tally;                    // [games][QTTT_SELFPLAY_TALLIES]  first wins, second wins, no winner, rows; cumulative
};

// one slot's harvest (the wave's), the body of selfplay_harvest_kernel and of the capped harvest
// (qttt_selfplay_cap_kernels.h), whose BY_STATE signs the finished game's v by the rows' states
template <bool BY_STATE>
__device__ __forceinline__ void selfplay_harvest_game(const void *tree, int64_t games, int64_t capacity, float v_first,
                                                      float v_second, const SelfPlayOut &o, const SelfPlayHarvest &hv, int64_t g,
                                                      u32 lane) {
    const TreeView v = tree_view(const_cast<void *>(tree), games, capacity);
    const TreeNodeHdr h = *v.hdr(g, v.games[g].root);
    const int ply = (int)o.length[g];
    // (a game is over after nine moves, so a terminal root always finds a row; the test keeps the stores inside the rows)
    if (!(h.flags & TN_TERMINAL) || ply >= QTTT_SELFPLAY_ROWS) {
        if (lane == 0u) { hv.harvest_len[g] = 0; hv.finished[g] = 0; }
        return;
    }
    const int64_t row = (int64_t)ply * games + g;
    selfplay_row_head(o, plane_stride(games), row, g, ply, h, true, lane);
    selfplay_terminal_row<BY_STATE>(o, games, row, g, ply, h, v_first, v_second, lane);
    if (lane == 0u) {
        const int w = (int)((h.flags >> 8) & 3u) - 1;            // 1 / 0 / -1 = True / False / None
        hv.harvest_len[g] = (uint8_t)(ply + 1);
        hv.finished[g] = 1;
        hv.games_done[g] += 1;
        int64_t *t = hv.tally + g * QTTT_SELFPLAY_TALLIES;
        t[w > 0 ? 0 : (w == 0 ? 1 : 2)] += 1;
        t[3] += ply + 1;
    }
}

__global__ __launch_bounds__(TREE_BLOCK) void selfplay_harvest_kernel(const void *tree, int64_t games, int64_t capacity,
                                                                      float v_first, float v_second, SelfPlayOut o,
                                                                      SelfPlayHarvest hv) {
    const int64_t g = (int64_t)blockIdx.x * TREE_GAMES_PER_BLOCK + threadIdx.x / 64;
    const u32 lane = threadIdx.x & 63u;
    if (g >= games) return;
    selfplay_harvest_game<false>(tree, games, capacity, v_first, v_second, o, hv, g, lane);
}

__global__ __launch_bounds__(TREE_BLOCK) void selfplay_restart_kernel(void *tree, int64_t games, int64_t capacity, u64 *pP,
                                                                      u64 *pQ, const uint8_t *finished, SelfPlayOut o) {
    __shared__ __attribute__((aligned(16))) uint8_t lut[LINE_LUT_BYTES];
    fill_line_lut<TREE_BLOCK>(lut);                              // ends with the workgroup barrier
    const int64_t g = (int64_t)blockIdx.x * TREE_GAMES_PER_BLOCK + threadIdx.x / 64;
    const u32 lane = threadIdx.x & 63u;
    if (g >= games || finished[g] == 0) return;
    const TreeView v = tree_view(tree, games, capacity);
    const TreeNodeHdr h = tree_node_of(0ull, 0ull, true, lut);   // the all-zero state is the empty board, the first player's
    tree_write_node(v, g, 0, h, lane, 0u);
    const int64_t stride = plane_stride(games);
    if (lane == 0u) {                                            // as tree_reset_kernel's
        TreeGame *gh = &v.games[g];
        gh->used = 1; gh->root = 0; gh->depth = 0; gh->leaf = 0;
        gh->flags = tree_leaf_flags(h.flags);
        pP[g] = 0ull; pQ[g] = 0ull;
        o.length[g] = 0;
    }
    if (lane < (u32)QTTT_SELFPLAY_ROWS) {                        // lane t: row t's scalars
        const int64_t row = (int64_t)lane * games + g;
        u64 *planes_t = o.states + (int64_t)lane * 2 * stride;
        planes_t[g] = 0ull;
        planes_t[stride + g] = 0ull;
        o.done[row] = 0;
        o.v[row] = 0.0f;
        o.action36[row] = 0;
    }
    for (u32 i = lane; i < 36u * QTTT_SELFPLAY_ROWS; i += 64u) {    // six rounds: the 36 entries of the ten rows
        const int64_t j = ((int64_t)(i / 36u) * games + g) * 36 + i % 36u;
        o.pi[j] = 0.0;
        o.mask[j] = 0;
    }
}

}  // namespace

#endif  // QTTT_SELFPLAY_STREAM_KERNELS_H
