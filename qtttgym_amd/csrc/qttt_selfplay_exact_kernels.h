// qttt_selfplay_exact_kernels.h — exact targets for the late rows of a self-play batch (include/qttt_selfplay_exact.h,
// DESIGN.md §25): selfplay_exact_targets_kernel replaces v and pi of every recorded, non-terminal row with enough moves
// played by the solver's value and the uniform policy over its optimal actions.
//
// The mapping, the list of boards and the item loop are qttt_solve_kernels.h's SolveList, shared with
// tree_solve_leaves_kernel.  This kernel's own: of the 10 * games records most need nothing (rows past a game's length,
// terminal rows, rows with too few moves played, and in a stream ply every game that did not finish) and end in step 1
// with their `exact` byte.  Record r = t * games + g, so that a wavefront reads one row's consecutive games: its loads of
// length / rows, done and the state planes are contiguous.  Every item stores its own 16 Q into q16[board][action],
// because the policy needs every action's value and not only the max; each slot has one writer, so there is no atomic on
// the values at all.  The lane that listed a board takes the max of its 36 slots, counts the k slots that attain it and
// writes v, the 36 doubles of pi and the exact byte: plain vector stores, and no two lanes write one address.  A listed
// board that turns out to be a leaf of the solver, or to have no action with a child, gets exact = 0 and nothing else.
#ifndef QTTT_SELFPLAY_EXACT_KERNELS_H
#define QTTT_SELFPLAY_EXACT_KERNELS_H
#include "qttt_selfplay.h"
#include "qttt_selfplay_exact.h"
#include "qttt_solve_kernels.h"

namespace {

static_assert(QTTT_SELFPLAY_EXACT_MAX_PLY == QTTT_SOLVE_MAX_PLY, "the solver's range");
static_assert(QTTT_SELFPLAY_EXACT_MIN_PLY == SOLVE_LIST_MIN_PLY, "a listed board's depth: SOLVE_LIST_DEPTH");

struct ExactTargets {
    const u64 *states;                 // [ROWS][2][plane_stride(games)]
    const uint8_t *rows;               // [games], nullable: stands in for length
    const uint8_t *length;             // [games]
    const uint8_t *done;               // [ROWS][games]
    double *pi;                        // [ROWS][games][36]
    float *v;                          // [ROWS][games]
    uint8_t *exact;                    // [ROWS][games], nullable
};

// Records rec0 .. rec0 + SOLVE_LIST_RECORDS * gridDim.x of the QTTT_SELFPLAY_ROWS * games records.
__global__ __launch_bounds__(SOLVE_BLOCK) void selfplay_exact_targets_kernel(ExactTargets o, int64_t games, int64_t rec0,
                                                                             int min_ply, int policy) {
    __shared__ __attribute__((aligned(16))) SolveList list;
    __shared__ int16_t q16[SOLVE_LIST_RECORDS][36];               // 16 Q of (listed board, action): one writer per slot

    const u32 tid = threadIdx.x;
    const int64_t records = (int64_t)QTTT_SELFPLAY_ROWS * games;
    const int64_t r = rec0 + (int64_t)blockIdx.x * SOLVE_LIST_RECORDS + tid;
    list.open();

    // ---- 1. classify: a lane per record
    int slot = -1;                                               // this lane's board in the list
    if (tid < (u32)SOLVE_LIST_RECORDS && r < records) {
        const int64_t t = r / games, g = r - t * games;          // t < QTTT_SELFPLAY_ROWS: r < records
        const int64_t L = (int64_t)(o.rows ? o.rows[g] : o.length[g]);
        if (t < L && o.done[r] == 0) {
            const int64_t stride = plane_stride(games);
            const u64 *planes_t = o.states + t * 2 * stride;
            const u64 P = planes_t[g];
            const u32 n_played = ((u32)(P >> 32) >> P1_N_SHIFT) & 0xFu;
            if ((int)n_played >= min_ply) slot = list.append(P, planes_t[stride + g]);
        }
        if (slot < 0 && o.exact) o.exact[r] = 0;                 // finished here
    }
    __syncthreads();
    if (list.n_boards == 0u) return;                             // workgroup-uniform

    // ---- 2. the tables, only where something is enumerated
    const SolveTables tb = list.fill_tables();

    // ---- 3. the listed boards' legal masks (none for a leaf of the solver), then the items: every action's Q
    if (tid < list.n_boards) list.root(tid, tb);
    list.items(tb, [&](u32 b, u32 a, int qv) { q16[b][a] = (int16_t)qv; });

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
