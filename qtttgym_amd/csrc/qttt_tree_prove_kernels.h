// qttt_tree_prove_kernels.h — proven interior nodes in the device search trees (include/qttt_tree_prove.h, DESIGN.md
// §26): tree_prove_kernel is the fifth launch of a round with exact leaves and walks every record of the round from its
// leaf's parent up to the root, solving each node all of whose legal actions lead to terminal or solved children;
// tree_root_exact_kernel reads what the proofs say of the roots.
//
// Mapping: qttt_tree_leaves_kernels.h's.  ONE WAVEFRONT PER GAME, lane a = action a, four games per 256-thread workgroup.
// A level of a walk is one node x: lane a loads its slot's child word and the flags words of the one or two children, one
// ballot against the legal mask decides whether x is provable, an integer butterfly over the wave gives 16 V(x), and lane
// 0 stores the flags word with one plain 32-bit vector store.  The next level's node is x's parent, whose lanes load the
// word just stored, and the next record may pass the same nodes: tree_wave_sync() follows every store, as in
// tree_backup_batch_kernel.  A level that is not provable stores nothing and ends the record's walk (wave-uniform: x, the
// legal mask and the ballot are).
//
// Integers only: the values are sixteenths in -16..16, a collapse halves an even sum, and nothing here is a floating-point
// operation (tree_root_exact_kernel converts its results to f32 once, exactly).  Every loop is bounded: leaves <=
// QTTT_TREE_MAX_LEAVES records, depth <= QTTT_TREE_MAX_DEPTH levels.  No atomics, no scratch, no LDS, no waiting on
// memory.  A child word is followed only where its nodes lie in the pool; an action whose word does not is unproven.
#ifndef QTTT_TREE_PROVE_KERNELS_H
#define QTTT_TREE_PROVE_KERNELS_H
#include "qttt_tree_prove.h"
#include "qttt_tree_exact_kernels.h"

namespace {

constexpr int PROVE_NO_Q = -64;                                  // below every 16 Q: an action that is not legal

// 16 * tree_terminal_value(node_flags) (qttt_tree_value_kernels.h), the value for the player to move at the node
__device__ __forceinline__ int tree_terminal_sixteenths(u32 node_flags) {
    const u32 w = (node_flags >> 8) & 3u;                        // 0 None, 1 False, 2 True
    if (w == 0u) return 0;
    return ((w == 2u) == ((node_flags & TN_TURN) != 0u)) ? SOLVE_ONE : -SOLVE_ONE;
}

// Action `lane` of node x with the legal mask `legal`: q16 = 16 Q(a) where the action is legal, expanded and all its
// children are terminal or solved (the return value), PROVE_NO_Q otherwise.
__device__ __forceinline__ bool tree_action_proven(const TreeView &v, int64_t g, int32_t x, u64 legal, u32 lane, int &q16) {
    q16 = PROVE_NO_Q;
    if (lane >= 36u || !((legal >> lane) & 1ull)) return false;
    const int32_t child = v.slots(g, x)[lane].child;
    if (child < 0) return false;
    const int32_t c0 = child & (TREE_CHILD_PAIR - 1);
    const int n = (child & TREE_CHILD_PAIR) ? 2 : 1;
    if ((int64_t)c0 + n > v.capacity) return false;             // not a word of a well-formed tree: never followed
    int sum = 0;
    bool known = true;
    for (int c = 0; c < n; ++c) {
        const u32 f = v.hdr(g, c0 + c)->flags;
        if (f & TN_TERMINAL) sum += tree_terminal_sixteenths(f);
        else if (f & TN_SOLVED) sum += (int)((f & TN_VALUE_MASK) >> TN_VALUE_SHIFT) - SOLVE_ONE;
        else known = false;
    }
    if (!known) return false;
    q16 = n == 2 ? -(sum / 2) : -sum;                            // the sum of a collapse is even (include/qttt_tree_prove.h)
    return true;
}

// every lane ends with the maximum over the wave
__device__ __forceinline__ int wave_max_int(int x) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const int o = __shfl_xor(x, m);
        x = o > x ? o : x;
    }
    return x;
}

__global__ __launch_bounds__(TREE_BLOCK) void tree_prove_kernel(void *tree, int64_t games, int64_t capacity, u32 leaves,
                                                                const TreePathRec *paths, int32_t *proved) {
    const int64_t g = (int64_t)blockIdx.x * TREE_GAMES_PER_BLOCK + threadIdx.x / 64;
    const u32 lane = threadIdx.x & 63u;
    if (g >= games) return;
    const TreeView v = tree_view(tree, games, capacity);
    const int64_t row0 = g * (int64_t)leaves;
    int32_t first = 0;                                           // nodes whose solved bit this launch set
    for (u32 j = 0; j < leaves; ++j) {
        const TreePathRec *rec = paths + (row0 + j);
        const int32_t leaf = rec->leaf;
        const u32 depth = rec->depth;
        const int32_t node = lane < (u32)QTTT_TREE_MAX_DEPTH ? rec->node[lane] : 0;
        const u32 action = lane < (u32)QTTT_TREE_MAX_DEPTH ? rec->action[lane] : 0u;
        // tree_backup_batch_kernel's check of the record (wave-uniform), and the rule's: depth >= 1
        const bool bad_edge = lane < depth && (node < 0 || (int64_t)node >= capacity || action >= 36u);
        if (depth == 0u || depth > (u32)QTTT_TREE_MAX_DEPTH || leaf < 0 || (int64_t)leaf >= capacity || __ballot(bad_edge) != 0ull)
            continue;
        for (int d = (int)depth - 1; d >= 0; --d) {
            const int32_t x = __shfl(node, d);
            TreeNodeHdr *xh = v.hdr(g, x);
            const u64 legal = xh->legal;
            const u32 xf = xh->flags;
            if ((xf & TN_TERMINAL) || legal == 0ull) break;
            int q16;
            const bool known = tree_action_proven(v, g, x, legal, lane, q16);
            if (__ballot(known) != legal) break;                 // an action of x is still open (known implies legal)
            const int v16 = wave_max_int(q16);
            u32 nf = (xf & ~TN_VALUE_MASK) | TN_SOLVED | ((u32)(v16 + SOLVE_ONE) << TN_VALUE_SHIFT);
            if (d >= 1) nf &= ~(TN_PRIORS | TN_UNIFORM);         // below the root: every later descent ends here
            if (lane == 0u) xh->flags = nf;
            first += (xf & TN_SOLVED) ? 0 : 1;
            tree_wave_sync();                                    // x's parent reads this word next, and so may the next record
        }
    }
    if (proved && lane == 0u) proved[g] = first;
}

__global__ __launch_bounds__(TREE_BLOCK) void tree_root_exact_kernel(const void *tree, int64_t games, int64_t capacity, float *q,
                                                                     uint8_t *proven, float *value, uint8_t *solved) {
    const int64_t g = (int64_t)blockIdx.x * TREE_GAMES_PER_BLOCK + threadIdx.x / 64;
    const u32 lane = threadIdx.x & 63u;
    if (g >= games) return;
    const TreeView v = tree_view(const_cast<void *>(tree), games, capacity);
    const int32_t root = v.games[g].root;
    const TreeNodeHdr *rh = v.hdr(g, root);
    const u32 rf = rh->flags;
    int q16;
    const bool known = tree_action_proven(v, g, root, rh->legal, lane, q16);
    if (lane < 36u) {
        if (proven) proven[g * 36 + lane] = known ? 1 : 0;
        if (q) q[g * 36 + lane] = known ? 0.0f - (float)(-q16) / (float)SOLVE_ONE : __builtin_nanf("");
    }
    if (lane == 0u) {
        const bool s = (rf & TN_SOLVED) != 0u;
        if (solved) solved[g] = s ? 1 : 0;
        if (value) value[g] = s ? (float)((int)((rf & TN_VALUE_MASK) >> TN_VALUE_SHIFT) - SOLVE_ONE) / (float)SOLVE_ONE : __builtin_nanf("");
    }
}

}  // namespace

#endif  // QTTT_TREE_PROVE_KERNELS_H
