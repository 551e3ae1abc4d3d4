// qttt_tree_exact_kernels.h — exact leaves in the device search trees (include/qttt_tree_exact.h):
// tree_solve_leaves_kernel stands between qttt_evaluate and the backup of a leaf-parallel round and replaces the network's
// value of every eligible leaf by its exact expectimax value, enumerating a leaf's tree the first time a round meets it
// and keeping the result in the node's flags.  (The backup that honours solved nodes is the EXACT instantiation of
// tree_backup_batch_kernel, qttt_tree_leaves_kernels.h.)
//
// The mapping, the list of boards and the item loop are qttt_solve_kernels.h's SolveList, shared with
// selfplay_exact_targets_kernel.  This kernel's own: of the games * K records of a round most are ineligible (too few
// moves played, a terminal leaf, a leaf that has priors) or already solved, and those end in step 1 without a table; an
// item's Q goes into its board's value by an integer LDS max; the lane that listed a board writes its node's flags (one
// 32-bit vector store) and its row of the outputs.  The classification's loop over a record's edges is bounded (10).
// Two records naming one node: see the header — every writer stores the same word.
#ifndef QTTT_TREE_EXACT_KERNELS_H
#define QTTT_TREE_EXACT_KERNELS_H
#include "qttt_tree_exact.h"
#include "qttt_tree_leaves_kernels.h"
#include "qttt_solve_kernels.h"

namespace {

static_assert(TN_SOLVED == QTTT_TREE_NODE_SOLVED && TN_VALUE_SHIFT == QTTT_TREE_NODE_VALUE_SHIFT &&
              TN_VALUE_MASK == QTTT_TREE_NODE_VALUE_MASK, "node flags of qttt_tree_exact.h");
static_assert(QTTT_TREE_EXACT_MIN_PLY == SOLVE_LIST_MIN_PLY, "a listed board's depth: SOLVE_LIST_DEPTH");

// Rows row0 .. row0 + SOLVE_LIST_RECORDS * gridDim.x of the round's `rows` = games * leaves records.
__global__ __launch_bounds__(SOLVE_BLOCK) void tree_solve_leaves_kernel(void *tree, int64_t games, int64_t capacity, u32 leaves,
                                                                        const TreePathRec *paths, const u64 *leafP,
                                                                        const u64 *leafQ, int64_t row0, int64_t rows,
                                                                        int min_ply, float *leaf_value, uint8_t *leaf_exact) {
    __shared__ __attribute__((aligned(16))) SolveList list;
    __shared__ int boardV[SOLVE_LIST_RECORDS];                    // 16 V of a listed board: the max over its items

    const u32 tid = threadIdx.x;
    const int64_t row = row0 + (int64_t)blockIdx.x * SOLVE_LIST_RECORDS + tid;
    list.open();

    // ---- 1. classify: a lane per record
    int slot = -1;                                               // this lane's board in the list
    u32 lf = 0u;
    u32 *flags = nullptr;
    if (tid < (u32)SOLVE_LIST_RECORDS && row < rows) {
        const TreeView v = tree_view(tree, games, capacity);
        const TreePathRec *rec = paths + row;
        const int64_t g = row / (int64_t)leaves;
        const int32_t leaf = rec->leaf;
        const u32 depth = rec->depth;
        // the backup's check of the record, and the rule's: depth >= 1, not overflowed
        bool ok = depth >= 1u && depth <= (u32)QTTT_TREE_MAX_DEPTH && leaf >= 0 && (int64_t)leaf < capacity &&
                  !(rec->flags & TG_OVERFLOW);
#pragma unroll
        for (u32 d = 0; d < (u32)QTTT_TREE_MAX_DEPTH; ++d) {
            const int32_t node = rec->node[d];
            const u32 a = rec->action[d];
            if (d < depth && (node < 0 || (int64_t)node >= capacity || a >= 36u)) ok = false;
        }
        bool eligible = false;
        if (ok) {
            flags = &v.hdr(g, leaf)->flags;
            lf = *flags;
            const u64 P = leafP[row];
            const u32 n_played = ((u32)(P >> 32) >> P1_N_SHIFT) & 0xFu;
            eligible = (lf & (TN_TERMINAL | TN_PRIORS)) == 0u && (int)n_played >= min_ply;
            if (eligible && !(lf & TN_SOLVED)) slot = list.append(P, leafQ[row]);
        }
        if (slot < 0) {                                          // finished here: ineligible, or solved already
            if (eligible && leaf_value)
                leaf_value[row] = solve_to_float((int)((lf & TN_VALUE_MASK) >> TN_VALUE_SHIFT) - SOLVE_ONE);
            if (leaf_exact) leaf_exact[row] = eligible ? 1 : 0;
        }
    }
    __syncthreads();
    const u32 nb = list.n_boards;                                // workgroup-uniform
    if (nb == 0u) return;

    // ---- 2. the tables, only where something is enumerated
    const SolveTables t = list.fill_tables();

    // ---- 3. the listed boards' roots, then the items: the board's value is the max over them
    if (tid < nb) {
        const SolveRoot r = list.root(tid, t);
        boardV[tid] = r.legal == 0ull ? solve_leaf_value(r.winner, list.boardP[tid]) : SOLVE_NO_Q;
    }
    list.items(t, [&](u32 b, u32, int qv) {
        if (qv != SOLVE_NO_Q) atomicMax(&boardV[b], qv);
    });

    // ---- 4. the node and the round's rows
    if (slot >= 0) {
        const int v16 = boardV[slot];
        const bool solved = v16 >= -SOLVE_ONE && v16 <= SOLVE_ONE;       // else no action had a child: left unsolved
        if (solved) {
            *flags = (lf & ~TN_VALUE_MASK) | TN_SOLVED | ((u32)(v16 + SOLVE_ONE) << TN_VALUE_SHIFT);
            if (leaf_value) leaf_value[row] = solve_to_float(v16);
        }
        if (leaf_exact) leaf_exact[row] = solved ? 1 : 0;
    }
}

}  // namespace

#endif  // QTTT_TREE_EXACT_KERNELS_H
