// qttt_selfplay_exact_kernels.h — exact targets for the late rows of a self-play batch (include/qttt_selfplay_exact.h,
// DESIGN.md §25): selfplay_exact_targets_kernel replaces v and pi of every recorded, non-terminal row with enough moves
// played by the solver's value and the uniform policy over its optimal actions.
//
// It is tree_solve_leaves_kernel's sibling (qttt_tree_exact_kernels.h) and the workload is that kernel's: of the 10 * games
// records most need nothing (rows past a game's length, terminal rows, rows with too few moves played, and in a stream ply
// every game that did not finish), and a board that does need enumeration has under 5 * 10^4 positions at six moves played
// and at most 2 000 from seven on.  So the mapping is the sibling's, for its reasons:
//
// Mapping.  ONE LANE PER RECORD, record r = t * games + g, so that a wavefront reads one row's consecutive games: its
// loads of length / rows, done and the state planes are contiguous.  64 records per 256-thread workgroup (its first
// wavefront classifies, all four solve); the grid is ceil(10 * games / 64), known on the host.
//   1. classify: a record that is not relabelled for a reason the staging bytes show (t >= L[g], done, too few moves
//      played) ends here with its `exact` byte, at the cost of one lane's loads and one store — no table is filled.  A lane
//      whose row qualifies appends the board to an LDS list (an integer LDS atomic hands out the slot).
//   2. one barrier; a workgroup whose list is empty returns.  The others fill the line table and the legal-mask table, once.
//   3. solve: the work item is (listed board, action), 36 per board, taken from an LDS counter by all 256 lanes; an item is
//      solve_action<TARGETS_DEPTH> — qttt_solve_kernels.h's recursion, called, not restated — with the board in registers.
//      What differs from the sibling: every item stores its own 16 Q into q16[board][action] (SOLVE_NO_Q where the action is
//      not legal or has no child), because the policy needs every action's value and not only the max.  Each slot has one
//      writer, so there is no atomic on the values at all.
//   4. after the barrier the lane that listed a board takes the max of its 36 slots, counts the k slots that attain it and
//      writes v, the 36 doubles of pi and the exact byte: plain vector stores.  A listed board that turns out to be a leaf
//      of the solver, or to have no action with a child, gets exact = 0 and nothing else.
// Every loop is bounded (64 * 36 items, 36 slots, the recursion's depth a template constant); no scratch; no floating-point
// atomic; nothing waits on memory another workgroup writes, and no two lanes write one address.
#ifndef QTTT_SELFPLAY_EXACT_KERNELS_H
#define QTTT_SELFPLAY_EXACT_KERNELS_H
#include "qttt_selfplay.h"
#include "qttt_selfplay_exact.h"
#include "qttt_solve_kernels.h"

namespace {

static_assert(QTTT_SELFPLAY_EXACT_MAX_PLY == QTTT_SOLVE_MAX_PLY, "the solver's range");

constexpr int TARGETS_BLOCK = 256;
constexpr int TARGETS_RECORDS = 64;                              // records per workgroup: one per lane of its first wavefront
constexpr u32 TARGETS_ITEMS = (u32)TARGETS_RECORDS * 36u;        // (listed board, action)
// plies that can still be played below the children of a listed board: it has at least QTTT_SELFPLAY_EXACT_MIN_PLY moves
// played, its children one more, and a game has nine
constexpr int TARGETS_DEPTH = 9 - QTTT_SELFPLAY_EXACT_MIN_PLY - 1;
static_assert(TARGETS_DEPTH >= 0 && TARGETS_DEPTH <= SOLVE_ITEM_DEPTH, "the recursion is no deeper than solve_kernel's");

struct ExactTargets {
    const u64 *states;                 // [ROWS][2][plane_stride(games)]
    const uint8_t *rows;               // [games], nullable: stands in for length
    const uint8_t *length;             // [games]
    const uint8_t *done;               // [ROWS][games]
    double *pi;                        // [ROWS][games][36]
    float *v;                          // [ROWS][games]
    uint8_t *exact;                    // [ROWS][games], nullable
};

// Records rec0 .. rec0 + TARGETS_RECORDS * gridDim.x of the QTTT_SELFPLAY_ROWS * games records.
__global__ __launch_bounds__(TARGETS_BLOCK) void selfplay_exact_targets_kernel(ExactTargets o, int64_t games, int64_t rec0,
                                                                               int min_ply, int policy) {
    __shared__ __attribute__((aligned(16))) uint8_t lut[LINE_LUT_BYTES];
    __shared__ u64 ltbl[512];
    __shared__ uint16_t act[36];
    __shared__ u64 boardP[TARGETS_RECORDS], boardQ[TARGETS_RECORDS], boardLegal[TARGETS_RECORDS];
    __shared__ int16_t q16[TARGETS_RECORDS][36];                 // 16 Q of (listed board, action): one writer per slot
    __shared__ u32 n_boards, next_item;

    const u32 tid = threadIdx.x;
    const int64_t records = (int64_t)QTTT_SELFPLAY_ROWS * games;
    const int64_t r = rec0 + (int64_t)blockIdx.x * TARGETS_RECORDS + tid;
    if (tid == 0u) n_boards = next_item = 0u;
    __syncthreads();

    // ---- 1. classify: a lane per record
    int slot = -1;                                               // this lane's board in the list
    if (tid < (u32)TARGETS_RECORDS && r < records) {
        const int64_t t = r / games, g = r - t * games;          // t < QTTT_SELFPLAY_ROWS: r < records
        const int64_t L = (int64_t)(o.rows ? o.rows[g] : o.length[g]);
        if (t < L && o.done[r] == 0) {
            const int64_t stride = plane_stride(games);
            const u64 *planes_t = o.states + t * 2 * stride;
            const u64 P = planes_t[g];
            const u32 n_played = ((u32)(P >> 32) >> P1_N_SHIFT) & 0xFu;
            if ((int)n_played >= min_ply) {
                slot = (int)atomicAdd(&n_boards, 1u);            // < TARGETS_RECORDS: one per classifying lane at most
                boardP[slot] = P;
                boardQ[slot] = planes_t[stride + g];
            }
        }
        if (slot < 0 && o.exact) o.exact[r] = 0;                 // finished here
    }
    __syncthreads();
    const u32 nb = n_boards;                                     // workgroup-uniform
    if (nb == 0u) return;

    // ---- 2. the tables, only where something is enumerated
    fill_legal_lut<TARGETS_BLOCK>(ltbl);
    if (tid < 36u) act[tid] = (uint16_t)pair_action<false>(tid);
    fill_line_lut<TARGETS_BLOCK>(lut);                           // ends with the workgroup barrier
    const SolveTables tb = {lut, ltbl, act};

    // ---- 3. the listed boards' legal masks (none for a leaf of the solver), then the items
    if (tid < nb) {
        const u64 P = boardP[tid];
        int winner, terminal;
        lite_update_winner(lite_unpack(P), lut, winner, terminal);
        const u64 legal = ltbl[classical_with_autofill(P)];
        boardLegal[tid] = terminal ? 0ull : legal;
    }
    __syncthreads();
    const u32 count = nb * 36u;
    for (u32 it = 0; it < TARGETS_ITEMS; ++it) {
        const u32 k = atomicAdd(&next_item, 1u);
        if (k >= count) break;
        const u32 b = k / 36u, a = k - b * 36u;
        int qv = SOLVE_NO_Q;
        if ((boardLegal[b] >> a) & 1ull) {
            u32 nodes = 0u;
            qv = solve_action<TARGETS_DEPTH>(boardP[b], boardQ[b], a, tb, nodes);
        }
        q16[b][a] = (int16_t)qv;
    }
    __syncthreads();

    // ---- 4. the row: the lane that listed the board
    if (slot >= 0) {
        int v16 = SOLVE_NO_Q;
        for (u32 a = 0; a < 36u; ++a) v16 = max(v16, (int)q16[slot][a]);
        const bool relabel = v16 != SOLVE_NO_Q;                  // else a leaf, or no action had a child: the row stays
        if (relabel) {
            o.v[r] = solve_to_float(v16);
            if (policy) {
                u32 k = 0u;
                for (u32 a = 0; a < 36u; ++a) k += (int)q16[slot][a] == v16 ? 1u : 0u;
                const double w = 1.0 / (double)k;                // k >= 1: the max is attained
                double *row = o.pi + r * 36;
                for (u32 a = 0; a < 36u; ++a) row[a] = (int)q16[slot][a] == v16 ? w : 0.0;
            }
        }
        if (o.exact) o.exact[r] = relabel ? 1 : 0;
    }
}

}  // namespace

#endif  // QTTT_SELFPLAY_EXACT_KERNELS_H
