// qttt_solve_kernels.h — the exact endgame solver (include/qttt_solve.h): the full expectimax tree of a
// late position, one board per 256-thread workgroup.  The two plies below the root are laid out in LDS — the root's
// children, then one item per (child, legal action of that child) — the lanes take items from an LDS counter and solve
// each item's subtree depth first with the board in registers, and the two top levels are reduced in LDS.  Values are
// held as the integer 16 V (every value is a multiple of 1/16: qttt_solve.h), so max, negation and the halving of a
// collapse are exact integer operations and no order of evaluation can change a bit.  Nothing is pruned.
// The rules are the shared ones: expand_pair and pair_action (qttt_search_core.h), update_winner_from_step /
// lite_update_winner and the legal-mask table (qttt_board_forms.h), leaf_turn_signed and reward_of_winner.
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

struct SolveOut {
    float *value;               // [n]
    float *q;                   // [n, 36]
    uint8_t *best;              // [n]
    int64_t *nodes;             // [n]
    uint8_t *status;            // [n]
};

__device__ __forceinline__ float solve_to_float(int v16) { return (float)v16 * (1.0f / (float)SOLVE_ONE); }

// Board i0 + blockIdx.x of the planes pP / pQ.
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
