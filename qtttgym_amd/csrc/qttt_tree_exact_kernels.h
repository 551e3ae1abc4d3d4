// qttt_tree_exact_kernels.h — exact leaves in the device search trees (include/qttt_tree_exact.h):
// tree_solve_leaves_kernel stands between qttt_evaluate and the backup of a leaf-parallel round and replaces the network's
// value of every eligible leaf by its exact expectimax value, enumerating a leaf's tree the first time a round meets it
// and keeping the result in the node's flags.  (The backup that honours solved nodes is the EXACT instantiation of
// tree_backup_batch_kernel, qttt_tree_leaves_kernels.h.)
//
// The workload is not solve_kernel's.  Of the games * K records of a round most are ineligible (too few moves played, a
// terminal leaf, a leaf that has priors) or already solved, and a board that does need enumeration has under 5 * 10^4
// positions at six moves played and at most 2 000 from seven on, where solve_kernel's boards have up to 10^7.  So:
//
// Mapping.  ONE LANE PER RECORD, 64 records per 256-thread workgroup (its first wavefront classifies, all four solve); the
// grid is ceil(games * K / 64), known on the host.  64 and not 256 records: a round of 4 096 games * 8 leaves is then 512
// workgroups, two per CU, where 128 would leave half the device idle while each ran several boards' items in turn.
//   1. classify: every lane reads its record and its leaf's flags word.  An ineligible record, or one whose node is
//      solved, is finished here, at the cost of one lane's loads and stores — no table is filled, no barrier beyond the
//      one that counts the boards.  A lane whose leaf needs enumeration appends the board to an LDS list (an integer LDS
//      atomic hands out the slot).
//   2. a workgroup whose list is empty returns.  The others fill the line table and the legal-mask table, once.
//   3. solve: the work item is (board of the list, root action), 36 per board, taken from an LDS counter by all 256
//      lanes; an item is solve_action<EXACT_DEPTH> — qttt_solve_kernels.h's recursion, called, not restated — with the
//      board in registers, and its Q goes into the board's value by an integer LDS max (16 V is an integer: no
//      floating-point atomic anywhere, and no order of evaluation can change a bit).  One level of items, not
//      solve_kernel's two: below a root action of a six-move board lie at most a few thousand positions, a fraction of a
//      solve_kernel item, and 36 items per board already spread one board over more than half a wave.
//   4. the lane that listed a board writes its node's flags (one 32-bit vector store) and its row of the outputs.
// Every loop is bounded (10 edges, 64 * 36 items, the recursion's depth a template constant); no scratch; nothing waits
// on memory another workgroup writes.  Two records naming one node: see the header — every writer stores the same word.
#ifndef QTTT_TREE_EXACT_KERNELS_H
#define QTTT_TREE_EXACT_KERNELS_H
#include "qttt_tree_exact.h"
#include "qttt_tree_leaves_kernels.h"
#include "qttt_solve_kernels.h"

namespace {

static_assert(TN_SOLVED == QTTT_TREE_NODE_SOLVED && TN_VALUE_SHIFT == QTTT_TREE_NODE_VALUE_SHIFT &&
              TN_VALUE_MASK == QTTT_TREE_NODE_VALUE_MASK, "node flags of qttt_tree_exact.h");

constexpr int EXACT_BLOCK = 256;
constexpr int EXACT_RECORDS = 64;                                // records per workgroup: one per lane of its first wavefront
constexpr u32 EXACT_ITEMS = (u32)EXACT_RECORDS * 36u;            // (listed board, root action)
// plies that can still be played below the children of a listed board: it has at least QTTT_TREE_EXACT_MIN_PLY moves
// played, its children one more, and a game has nine
constexpr int EXACT_DEPTH = 9 - QTTT_TREE_EXACT_MIN_PLY - 1;
static_assert(EXACT_DEPTH >= 0 && EXACT_DEPTH <= SOLVE_ITEM_DEPTH, "the recursion is no deeper than solve_kernel's");

// Rows row0 .. row0 + EXACT_RECORDS * gridDim.x of the round's `rows` = games * leaves records.
__global__ __launch_bounds__(EXACT_BLOCK) void tree_solve_leaves_kernel(void *tree, int64_t games, int64_t capacity, u32 leaves,
                                                                        const TreePathRec *paths, const u64 *leafP,
                                                                        const u64 *leafQ, int64_t row0, int64_t rows,
                                                                        int min_ply, float *leaf_value, uint8_t *leaf_exact) {
    __shared__ __attribute__((aligned(16))) uint8_t lut[LINE_LUT_BYTES];
    __shared__ u64 ltbl[512];
    __shared__ uint16_t act[36];
    __shared__ u64 boardP[EXACT_RECORDS], boardQ[EXACT_RECORDS], boardLegal[EXACT_RECORDS];
    __shared__ int boardV[EXACT_RECORDS];                         // 16 V of a listed board: the max over its items
    __shared__ u32 n_boards, next_item;

    const u32 tid = threadIdx.x;
    const int64_t row = row0 + (int64_t)blockIdx.x * EXACT_RECORDS + tid;
    if (tid == 0u) n_boards = next_item = 0u;
    __syncthreads();

    // ---- 1. classify: a lane per record
    int slot = -1;                                               // this lane's board in the list
    u32 lf = 0u;
    u32 *flags = nullptr;
    if (tid < (u32)EXACT_RECORDS && row < rows) {
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
            if (eligible && !(lf & TN_SOLVED)) {
                slot = (int)atomicAdd(&n_boards, 1u);            // < EXACT_RECORDS: one per classifying lane at most
                boardP[slot] = P;
                boardQ[slot] = leafQ[row];
            }
        }
        if (slot < 0) {                                          // finished here: ineligible, or solved already
            if (eligible && leaf_value)
                leaf_value[row] = solve_to_float((int)((lf & TN_VALUE_MASK) >> TN_VALUE_SHIFT) - SOLVE_ONE);
            if (leaf_exact) leaf_exact[row] = eligible ? 1 : 0;
        }
    }
    __syncthreads();
    const u32 nb = n_boards;                                     // workgroup-uniform
    if (nb == 0u) return;

    // ---- 2. the tables, only where something is enumerated
    fill_legal_lut<EXACT_BLOCK>(ltbl);
    if (tid < 36u) act[tid] = (uint16_t)pair_action<false>(tid);
    fill_line_lut<EXACT_BLOCK>(lut);                             // ends with the workgroup barrier
    const SolveTables t = {lut, ltbl, act};

    // ---- 3. the listed boards' roots, then the items
    if (tid < nb) {
        const u64 P = boardP[tid];
        int winner, terminal;
        lite_update_winner(lite_unpack(P), lut, winner, terminal);
        const u64 legal = ltbl[classical_with_autofill(P)];
        const bool leaf = terminal || legal == 0ull;             // a leaf of the solver (an empty legal mask)
        boardLegal[tid] = leaf ? 0ull : legal;
        boardV[tid] = leaf ? solve_leaf_value(winner, P) : SOLVE_NO_Q;
    }
    __syncthreads();
    const u32 count = nb * 36u;
    for (u32 it = 0; it < EXACT_ITEMS; ++it) {
        const u32 k = atomicAdd(&next_item, 1u);
        if (k >= count) break;
        const u32 b = k / 36u, a = k - b * 36u;
        if ((boardLegal[b] >> a) & 1ull) {
            u32 nodes = 0u;
            const int qv = solve_action<EXACT_DEPTH>(boardP[b], boardQ[b], a, t, nodes);
            if (qv != SOLVE_NO_Q) atomicMax(&boardV[b], qv);
        }
    }
    __syncthreads();

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
