// qttt_solve_kernels.h — the exact endgame solver (include/qttt_solve.h): the full expectimax tree of a
// late position, one board per 256-thread workgroup.  The two plies below the root are laid out in LDS — the root's
// children, then one item per (child, legal action of that child) — the lanes take items from an LDS counter and solve
// each item's subtree depth first with the board in registers, and the two top levels are reduced in LDS.  Values are
// held as the integer 16 V (every value is a multiple of 1/16: qttt_solve.h), so max, negation and the halving of a
// collapse are exact integer operations and no order of evaluation can change a bit.  Nothing is pruned.
// The rules are the shared ones: expand_pair and pair_action (qttt_search_core.h), update_winner_from_step /
// lite_update_winner and the legal-mask table (qttt_board_forms.h), leaf_turn_signed and reward_of_winner.
// Shared with tree_solve_leaves_kernel and selfplay_exact_targets_kernel, which call the recursion on many small boards:
// SolveList, the workgroup's list of boards with its table fill, its roots' classification and its item loop.
#ifndef QTTT_SOLVE_KERNELS_H
#define QTTT_SOLVE_KERNELS_H
#include "qttt_solve.h"
#include "qttt_search_core.h"

namespace {

constexpr int SOLVE_BLOCK = 256;
constexpr int SOLVE_ONE = QTTT_SOLVE_DENOMINATOR;        // the value 1 in the kernel's fixed point
constexpr int SOLVE_NO_Q = -1024;                        // the Q of an action that is not legal
constexpr u32 SOLVE_CHILDREN = 72u;                      // 36 root actions x 2 collapse children
constexpr u32 SOLVE_SLOTS = SOLVE_CHILDREN * 36u;        // (child, action of the child)
// plies a lane's recursion can still play below the positions an item's expansion yields: those have at least
// QTTT_SOLVE_MIN_PLY + 2 moves played, and a game has nine
constexpr int SOLVE_ITEM_DEPTH = 9 - QTTT_SOLVE_MIN_PLY - 2;

struct SolveTables {
    const uint8_t *lut;         // the line table (fill_line_lut)
    const u64 *legal;           // legal mask by classical mask (fill_legal_lut)
    const uint16_t *act;        // the step's action word of pair index a (pair_action)
};

// the leaf rule: the value, times 16, of a leaf with this winner, seen by the player to move
__device__ __forceinline__ int solve_leaf_value(int winner, u64 P) {
    return SOLVE_ONE * leaf_turn_signed(reward_of_winner(winner), (u32)(P >> 32));
}
// Q from the sum of the children's values: 0 - V(child0), or 0 - (V(child0) + V(child1)) / 2 (the sum is even: qttt_solve.h)
__device__ __forceinline__ int solve_q_of_children(u32 kids, int sum) { return kids == 2u ? -(sum / 2) : -sum; }

template <int DEPTH>
__device__ __forceinline__ int solve_position(u64 P, u64 Q, u64 legal, const SolveTables &t, u32 &nodes);

// 16 Q(a) of the position (P, Q), SOLVE_NO_Q where the expansion has no child; `nodes` += the positions visited below.
// DEPTH: the plies that can still be played below the children; at 0 they have nine moves played and are leaves.
// The children go through ONE copy of the code below them (a select picks the child, not an unrolled loop): the
// recursion is inlined to its full depth, and two copies per level would be sixteen of the deepest.
template <int DEPTH>
__device__ __forceinline__ int solve_action(u64 P, u64 Q, u32 a, const SolveTables &t, u32 &nodes) {
    const Expansion e = expand_pair(P, Q, (u32)t.act[a], t.lut);
    if (e.kids == 0u) return SOLVE_NO_Q;
    int sum = 0;
    for (u32 k = 0; k < 2u && k < e.kids; ++k) {
        const u64 Pk = k ? e.P[1] : e.P[0];
        const u32 xo = k ? e.xo[1] : e.xo[0];
        int winner, terminal;
        update_winner_from_step(Pk, xo, t.lut, winner, terminal);
        nodes += 1u;
        if constexpr (DEPTH == 0) {
            sum += solve_leaf_value(winner, Pk);
        } else {
            const u64 legal = t.legal[classical_with_autofill(Pk)];
            if (terminal || legal == 0ull) sum += solve_leaf_value(winner, Pk);
            else sum += solve_position<DEPTH - 1>(Pk, e.Q, legal, t, nodes);
        }
    }
    return solve_q_of_children(e.kids, sum);
}

// 16 V of the non-leaf (P, Q) with legal mask `legal`: the max over its legal actions, at most 36 of them
template <int DEPTH>
__device__ __forceinline__ int solve_position(u64 P, u64 Q, u64 legal, const SolveTables &t, u32 &nodes) {
    int best = SOLVE_NO_Q;
    for (u32 it = 0; it < 36u && legal != 0ull; ++it) {
        const u32 a = (u32)__builtin_ctzll(legal);
        legal &= legal - 1ull;
        best = max(best, solve_action<DEPTH>(P, Q, a, t, nodes));
    }
    return best;
}

// ---------------------------------------------------------------- many small boards: a list per workgroup
// The kernels that solve the records of a batch (a round's leaves, a self-play batch's rows) have another workload than
// solve_kernel: most records need nothing, and a board that does need enumeration has under 5 * 10^4 positions at six
// moves played and at most 2 000 from seven on, where solve_kernel's boards have up to 10^7.  So:
// Mapping.  ONE LANE PER RECORD, 64 records per SOLVE_BLOCK-thread workgroup (its first wavefront classifies, all four
// solve); the grid is ceil(records / 64), known on the host.  64 and not 256 records: a round of 4 096 games * 8 leaves is
// then 512 workgroups, two per CU, where 128 would leave half the device idle while each ran several boards' items in turn.
//   1. classify (the kernel's own): a record that needs no enumeration is finished by its lane, at the cost of that lane's
//      loads and stores; a lane whose board needs it appends the board to the list (an integer LDS atomic hands out the slot).
//   2. one barrier; a workgroup whose list is empty returns.  The others fill the tables, once.
//   3. root() of every listed board, then the work item is (listed board, action), 36 per board, taken from an LDS counter
//      by all 256 lanes; an item is solve_action<SOLVE_LIST_DEPTH> — the recursion above, called, not restated — with the
//      board in registers, and its 16 Q goes to the kernel's callable: an integer, so there is no floating-point atomic and
//      no order of evaluation can change a bit.  One level of items, not solve_kernel's two: below a root action of a
//      six-move board lie at most a few thousand positions, a fraction of a solve_kernel item, and 36 items per board
//      already spread one board over more than half a wave.
//   4. write back (the kernel's own): the lane that listed a board writes its row.
// Every loop is bounded (64 * 36 items, the recursion's depth a constant); no scratch; no wait on another workgroup.
constexpr int SOLVE_LIST_RECORDS = 64;                           // records per workgroup: one per lane of its first wavefront
constexpr u32 SOLVE_LIST_ITEMS = (u32)SOLVE_LIST_RECORDS * 36u;  // (listed board, action)
// a listed board has SOLVE_LIST_MIN_PLY moves played or more (each kernel asserts its header's), its children one more
constexpr int SOLVE_LIST_MIN_PLY = 6;
constexpr int SOLVE_LIST_DEPTH = 9 - SOLVE_LIST_MIN_PLY - 1;
static_assert(SOLVE_LIST_DEPTH >= 0 && SOLVE_LIST_DEPTH <= SOLVE_ITEM_DEPTH, "the recursion is no deeper than solve_kernel's");

// The root of a listed board: its winner and its legal mask, the mask 0 for a leaf of the solver (a terminal position, or
// one without a legal action: its value is solve_leaf_value(winner, P)).
struct SolveRoot {
    int winner;
    u64 legal;
};

// Holds its tables too: ONE __shared__ variable per kernel, aligned(16) for the line table, and no LDS padding inside.
struct SolveList {
    uint8_t lut[LINE_LUT_BYTES];
    u64 ltbl[512];
    uint16_t act[36];
    u64 boardP[SOLVE_LIST_RECORDS], boardQ[SOLVE_LIST_RECORDS], boardLegal[SOLVE_LIST_RECORDS];
    u32 n_boards, next_item;

    // empty, for every lane after the barrier
    __device__ __forceinline__ void open() {
        if (threadIdx.x == 0u) n_boards = next_item = 0u;
        __syncthreads();
    }
    // the three tables, by all SOLVE_BLOCK lanes; ends with the workgroup barrier
    __device__ __forceinline__ SolveTables fill_tables() {
        fill_legal_lut<SOLVE_BLOCK>(ltbl);
        if (threadIdx.x < 36u) act[threadIdx.x] = (uint16_t)pair_action<false>(threadIdx.x);
        fill_line_lut<SOLVE_BLOCK>(lut);
        return {lut, ltbl, act};
    }
    // by a classifying lane, once at most: the board's slot, < SOLVE_LIST_RECORDS
    __device__ __forceinline__ int append(u64 P, u64 Q) {
        const int slot = (int)atomicAdd(&n_boards, 1u);
        boardP[slot] = P;
        boardQ[slot] = Q;
        return slot;
    }
    // by the lane b < n_boards, before items(): the listed board's legal mask into the list, none for a leaf of the solver
    __device__ __forceinline__ SolveRoot root(u32 b, const SolveTables &t) {
        int winner, terminal;
        lite_update_winner(lite_unpack(boardP[b]), t.lut, winner, terminal);
        const u64 legal = t.legal[classical_with_autofill(boardP[b])];
        boardLegal[b] = terminal ? 0ull : legal;
        return {winner, terminal ? 0ull : legal};
    }
    // by all lanes, between two workgroup barriers: f(b, a, 16 Q) for every action a of every listed board b, once each;
    // SOLVE_NO_Q for an action that is not legal or has no child
    template <typename F>
    __device__ __forceinline__ void items(const SolveTables &t, F &&f) {
        __syncthreads();
        const u32 count = n_boards * 36u;
        for (u32 it = 0; it < SOLVE_LIST_ITEMS; ++it) {
            const u32 k = atomicAdd(&next_item, 1u);
            if (k >= count) break;
            const u32 b = k / 36u, a = k - b * 36u;
            int qv = SOLVE_NO_Q;
            if ((boardLegal[b] >> a) & 1ull) {
                u32 nodes = 0u;
                qv = solve_action<SOLVE_LIST_DEPTH>(boardP[b], boardQ[b], a, t, nodes);
            }
            f(b, a, qv);
        }
        __syncthreads();
    }
};

struct SolveOut {
    float *value;               // [n]
    float *q;                   // [n, 36]
    uint8_t *best;              // [n]
    int64_t *nodes;             // [n]
    uint8_t *status;            // [n]
};

__device__ __forceinline__ float solve_to_float(int v16) { return (float)v16 * (1.0f / (float)SOLVE_ONE); }

// Board i0 + blockIdx.x of the planes pP / pQ.  Its table fill and root classification are spelled out here on purpose.
__global__ __launch_bounds__(SOLVE_BLOCK) void solve_kernel(const u64 *pP, const u64 *pQ, int64_t i0, int min_ply, SolveOut out) {
    __shared__ __attribute__((aligned(16))) uint8_t lut[LINE_LUT_BYTES];
    __shared__ u64 ltbl[512];
    __shared__ uint16_t act[36];
    __shared__ u64 childP[SOLVE_CHILDREN], childQ[SOLVE_CHILDREN], childLegal[SOLVE_CHILDREN];
    __shared__ int childV[SOLVE_CHILDREN];                 // a leaf child's value; the reduced value of the others
    __shared__ u32 childNodes[SOLVE_CHILDREN];
    __shared__ uint8_t childKind[SOLVE_CHILDREN];          // 0 absent, 1 leaf, 2 to be solved
    __shared__ uint8_t rootKids[36];
    __shared__ uint16_t items[SOLVE_SLOTS];
    __shared__ int16_t slotQ[SOLVE_SLOTS];
    __shared__ u32 slotNodes[SOLVE_SLOTS];
    __shared__ int rootQ[36];
    __shared__ u32 n_items, next_item;

    const u32 tid = threadIdx.x;
    const int64_t i = i0 + (int64_t)blockIdx.x;
    const u64 P = pP[i], Q = pQ[i];                        // every lane the same board
    fill_legal_lut<SOLVE_BLOCK>(ltbl);
    if (tid < 36u) act[tid] = (uint16_t)pair_action<false>(tid);
    if (tid < SOLVE_CHILDREN) childKind[tid] = 0;
    if (tid == 0u) n_items = next_item = 0u;
    for (u32 s = tid; s < SOLVE_SLOTS; s += SOLVE_BLOCK) slotQ[s] = (int16_t)SOLVE_NO_Q;
    fill_line_lut<SOLVE_BLOCK>(lut);                       // ends with the workgroup barrier
    const SolveTables t = {lut, ltbl, act};

    // ---- the root: workgroup-uniform
    int root_winner, root_terminal;
    lite_update_winner(lite_unpack(P), lut, root_winner, root_terminal);
    const u64 root_legal = ltbl[classical_with_autofill(P)];
    const u32 n_played = ((u32)(P >> 32) >> P1_N_SHIFT) & 0xFu;
    const bool leaf = root_terminal || root_legal == 0ull;
    if (leaf || (int)n_played < min_ply) {
        const float qv = leaf ? -__builtin_inff() : __builtin_nanf("");
        if (out.q && tid < 36u) out.q[i * 36 + tid] = qv;
        if (tid == 0u) {
            if (out.value) out.value[i] = leaf ? solve_to_float(solve_leaf_value(root_winner, P)) : __builtin_nanf("");
            if (out.best) out.best[i] = 255;
            if (out.nodes) out.nodes[i] = leaf ? 1 : 0;
            if (out.status) out.status[i] = leaf ? 0 : 1;
        }
        return;
    }

    // ---- ply 1: a lane per root action; child 2a + k
    if (tid < 36u) {
        u32 kids = 0u;
        if ((root_legal >> tid) & 1ull) {
            const Expansion e = expand_pair(P, Q, (u32)act[tid], lut);
            kids = e.kids;
#pragma unroll
            for (u32 k = 0; k < 2u; ++k) {
                if (k < kids) {
                    int winner, terminal;
                    update_winner_from_step(e.P[k], e.xo[k], lut, winner, terminal);
                    const u64 legal = ltbl[classical_with_autofill(e.P[k])];
                    const u32 c = 2u * tid + k;
                    const bool child_leaf = terminal || legal == 0ull;
                    childP[c] = e.P[k];
                    childQ[c] = e.Q;
                    childLegal[c] = legal;
                    childV[c] = child_leaf ? solve_leaf_value(winner, e.P[k]) : SOLVE_NO_Q;
                    childNodes[c] = 1u;
                    childKind[c] = child_leaf ? 1 : 2;
                }
            }
        }
        rootKids[tid] = (uint8_t)kids;
    }
    __syncthreads();

    // ---- ply 2: the work list, one item per legal action of a child that is no leaf
    for (u32 s = tid; s < SOLVE_SLOTS; s += SOLVE_BLOCK) {
        const u32 c = s / 36u, a = s - c * 36u;
        if (childKind[c] == 2 && ((childLegal[c] >> a) & 1ull)) items[atomicAdd(&n_items, 1u)] = (uint16_t)s;   // < SOLVE_SLOTS: one per s
    }
    __syncthreads();
    const u32 count = n_items;
    for (u32 it = 0; it < SOLVE_SLOTS; ++it) {
        const u32 k = atomicAdd(&next_item, 1u);
        if (k >= count) break;
        const u32 s = items[k], c = s / 36u, a = s - c * 36u;
        u32 nodes = 0u;
        const int qv = solve_action<SOLVE_ITEM_DEPTH>(childP[c], childQ[c], a, t, nodes);
        slotQ[s] = (int16_t)qv;
        slotNodes[s] = nodes;
    }
    __syncthreads();

    // ---- back up: the children from their slots, then the root actions from their children
    if (tid < SOLVE_CHILDREN && childKind[tid] == 2) {
        int v = SOLVE_NO_Q;
        u32 nodes = 1u;
        for (u32 a = 0; a < 36u; ++a) {
            const int qv = slotQ[tid * 36u + a];
            if (qv != SOLVE_NO_Q) {
                v = max(v, qv);
                nodes += slotNodes[tid * 36u + a];
            }
        }
        childV[tid] = v;
        childNodes[tid] = nodes;
    }
    __syncthreads();
    if (tid < 36u) {
        const u32 kids = rootKids[tid];
        const int qv = kids ? solve_q_of_children(kids, childV[2u * tid] + (kids == 2u ? childV[2u * tid + 1u] : 0)) : SOLVE_NO_Q;
        rootQ[tid] = qv;
        if (out.q) out.q[i * 36 + tid] = qv == SOLVE_NO_Q ? -__builtin_inff() : solve_to_float(qv);
    }
    __syncthreads();
    if (tid == 0u) {
        int v = SOLVE_NO_Q;
        u32 best = 255u;
        u64 nodes = 1ull;
        for (u32 a = 0; a < 36u; ++a) {
            if (rootQ[a] > v) { v = rootQ[a]; best = a; }                 // strict: the lowest action that attains the max
            for (u32 k = 0; k < (u32)rootKids[a]; ++k) nodes += childNodes[2u * a + k];
        }
        if (out.value) out.value[i] = solve_to_float(v);
        if (out.best) out.best[i] = (uint8_t)best;
        if (out.nodes) out.nodes[i] = (int64_t)nodes;
        if (out.status) out.status[i] = 0;
    }
}

}  // namespace

#endif  // QTTT_SOLVE_KERNELS_H
