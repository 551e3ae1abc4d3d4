// qttt_tree_kernels.h — batched MCTS / AlphaZero search trees on the device (include/qttt_tree.h).
//
// Mapping: ONE WAVEFRONT PER GAME, lane a = action a (lanes 36..63 idle).  A tree level is one node: its 36 action
// slots are read as one coalesced 576-byte load (16 B per lane), every lane scores its action in f64, and a butterfly
// over the wave picks the argmax.  The one-lane-per-board mapping of the step kernels fits a state that
// lives in registers; a tree node is 36-wide and lives in HBM, so here a lane per action is the natural unit.
// A wave owns its game: node allocation needs no atomics, and no kernel here re-reads what it wrote itself.  The one
// descent, tree_descend (called by tree_select_kernel, and K times per game by tree_select_batch_kernel of
// qttt_tree_leaves_kernels.h), reads nothing that it stored: a freshly expanded child has no priors, so the descent ends
// on it with the child's header still in registers, and the path stays in lane registers until the caller stores it.  The
// one exception is tree_compact_kernel, whose lanes hand each other marks through memory, with tree_wave_sync() in between.
// Buffer layout: include/qttt_tree.h.
#ifndef QTTT_TREE_KERNELS_H
#define QTTT_TREE_KERNELS_H
#include "qttt_step_core.h"
#include "qttt_board_forms.h"
#include "qttt_search_core.h"
#include "qttt_tree.h"
#include "qttt_tree_compact.h"

namespace {

constexpr int TREE_BLOCK = 256;                                 // 4 games per workgroup
constexpr int TREE_GAMES_PER_BLOCK = TREE_BLOCK / 64;
constexpr u32 TN_PRIORS = 1u, TN_UNIFORM = 2u, TN_TERMINAL = 4u, TN_TURN = 8u;      // node flags
constexpr u32 TN_SOLVED = 16u, TN_VALUE_SHIFT = 16u, TN_VALUE_MASK = 63u << TN_VALUE_SHIFT;   // include/qttt_tree_exact.h
constexpr u32 TG_OVERFLOW = 1u, TG_LEAF_TURN = 2u, TG_LEAF_TERMINAL = 4u;          // game-header and path-record flags
constexpr int TREE_CHILD_PAIR = 1 << 30;

struct TreeGame {                      // 128 B, include/qttt_tree.h
    int32_t used, root, depth, leaf;
    u32 flags, pad[3];
    int32_t path_node[QTTT_TREE_MAX_DEPTH];
    uint8_t path_action[QTTT_TREE_MAX_DEPTH];
    uint8_t pad2[128 - 82];
};
static_assert(sizeof(TreeGame) == QTTT_TREE_GAME_BYTES, "game header");
struct TreeNodeHdr {                   // 32 B
    u64 P, Q, legal;
    u32 Ntot, flags;
};
struct TreeSlot {                      // 16 B: one action of one node
    double W;
    u32 N;
    int32_t child;
};
static_assert(sizeof(TreeNodeHdr) + 36 * sizeof(TreeSlot) == QTTT_TREE_NODE_BYTES, "node record");
typedef u32 __attribute__((ext_vector_type(4), may_alias)) TreeVec;      // 16 B of a node record, whatever they hold

struct TreeView {
    TreeGame *games;
    uint8_t *nodes;                    // [games][capacity] records of QTTT_TREE_NODE_BYTES
    float *priors;                     // [games][capacity][36]
    int64_t capacity;
    __device__ __forceinline__ TreeNodeHdr *hdr(int64_t g, int32_t i) const {
        return reinterpret_cast<TreeNodeHdr *>(nodes + (g * capacity + i) * (int64_t)QTTT_TREE_NODE_BYTES);
    }
    __device__ __forceinline__ TreeSlot *slots(int64_t g, int32_t i) const {
        return reinterpret_cast<TreeSlot *>(nodes + (g * capacity + i) * (int64_t)QTTT_TREE_NODE_BYTES + 32);
    }
    __device__ __forceinline__ float *prior(int64_t g, int32_t i) const { return priors + (g * capacity + i) * 36; }
};
__host__ __device__ inline TreeView tree_view(void *tree, int64_t games, int64_t capacity) {
    TreeView v;
    uint8_t *b = reinterpret_cast<uint8_t *>(tree);
    v.games = reinterpret_cast<TreeGame *>(b);
    v.nodes = b + games * (int64_t)QTTT_TREE_GAME_BYTES;
    v.priors = reinterpret_cast<float *>(v.nodes + games * capacity * (int64_t)QTTT_TREE_NODE_BYTES);
    v.capacity = capacity;
    return v;
}

// 1 / len(actions) (mcts.py:289) for 0..36 legal actions, rounded by the host compiler
struct UniformPriors {
    double p[37];
    constexpr UniformPriors() : p() {
        for (int k = 1; k <= 36; ++k) p[k] = 1.0 / (double)k;
    }
};
__constant__ UniformPriors g_uniform_priors = UniformPriors();

// The selection score's sqrt(Ntot) (mcts.py:283).  llvm.sqrt.f64 is lowered correctly rounded on gfx950;
// tests/test_tree_gpu.py checks it for every Ntot below QTTT_TREE_MAX_ROLLOUTS against the host's sqrt.
__device__ __forceinline__ double tree_sqrt(u32 ntot) { return __builtin_sqrt((double)ntot); }

// a fresh node's record from GameState's bookkeeping (mcts.py:20-27,52-65): winner w, terminal t, the legal-action mask
__device__ __forceinline__ TreeNodeHdr tree_node(u64 P, u64 Q, bool turn, int w, int t, u64 legal) {
    TreeNodeHdr h;
    h.P = P; h.Q = Q;
    h.legal = legal;
    h.Ntot = 0;
    h.flags = (t ? TN_TERMINAL : 0u) | (turn ? TN_TURN : 0u) | ((u32)(w + 1) << 8);
    return h;
}
// the node record of a position given as its packed state alone
__device__ __forceinline__ TreeNodeHdr tree_node_of(u64 P, u64 Q, bool turn, const uint8_t *lut) {
    const Lite s = lite_unpack(P);
    int w, t;
    lite_update_winner(s, lut, w, t);
    return tree_node(P, Q, turn, w, t, legal_mask_of(s.cl));
}

// what the game header and a path record say of a leaf with these node flags
__device__ __forceinline__ u32 tree_leaf_flags(u32 node_flags) {
    return (node_flags & TN_TURN ? TG_LEAF_TURN : 0u) | (node_flags & TN_TERMINAL ? TG_LEAF_TERMINAL : 0u);
}

// a fresh node: header (by lane `writer`) and 36 empty slots (lanes 0..35)
__device__ __forceinline__ void tree_write_node(const TreeView &v, int64_t g, int32_t i, const TreeNodeHdr &h, u32 lane,
                                                u32 writer) {
    if (lane == writer) *v.hdr(g, i) = h;
    if (lane < 36u) {
        TreeSlot s;
        s.W = 0.0; s.N = 0u; s.child = -1;
        v.slots(g, i)[lane] = s;
    }
}

// wave argmax of (valid, score) with ties to the lowest lane: every lane ends with the winning lane, or -1
__device__ __forceinline__ int wave_argmax(bool valid, double score, u32 lane) {
    int idx = valid ? (int)lane : -1;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const double os = __shfl_xor(score, m);
        const int oi = __shfl_xor(idx, m);
        const bool take = oi >= 0 && (idx < 0 || os > score || (os == score && oi < idx));
        score = take ? os : score;
        idx = take ? oi : idx;
    }
    return idx;
}

// the sum of include/qttt_selfplay.h (the record's pi, and the noise of qttt_tree_explore.h): 64 terms (lanes 36..63
// hold 0), s[i] += s[i ^ m] for m = 1 .. 32; every lane ends with the same double
__device__ __forceinline__ double selfplay_wave_sum(double x) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) x = x + __shfl_xor(x, m);
    return x;
}

__device__ __forceinline__ double tree_prior(const TreeView &v, int64_t g, int32_t node, const TreeNodeHdr &h, u32 a) {
    if (h.flags & TN_UNIFORM) return g_uniform_priors.p[__builtin_popcountll(h.legal)];
    return (double)v.prior(g, node)[a];
}

// _uct_select's score (mcts.py:282-284) in the reference's order, no contraction into FMAs
__device__ __forceinline__ double tree_score(double W, u32 N, double prior, double sq, double c_puct) {
#pragma clang fp contract(off)
    const double q = N ? W / (double)N : 0.0;
    const double u = prior * sq / (double)(1u + N);
    return q + c_puct * u;
}

__global__ __launch_bounds__(TREE_BLOCK) void tree_reset_kernel(void *tree, int64_t games, int64_t capacity,
                                                                const u64 *pP, const u64 *pQ) {
    __shared__ __attribute__((aligned(16))) uint8_t lut[LINE_LUT_BYTES];
    fill_line_lut<TREE_BLOCK>(lut);
    const int64_t g = (int64_t)blockIdx.x * TREE_GAMES_PER_BLOCK + threadIdx.x / 64;
    const u32 lane = threadIdx.x & 63u;
    if (g >= games) return;
    const TreeView v = tree_view(tree, games, capacity);
    const u64 P = pP[g], Q = pQ[g];
    const TreeNodeHdr h = tree_node_of(P, Q, (lite_unpack(P).n & 1u) == 0u, lut);       // mcts.py:141
    tree_write_node(v, g, 0, h, lane, 0u);
    if (lane == 0u) {
        TreeGame *gh = &v.games[g];
        gh->used = 1; gh->root = 0; gh->depth = 0; gh->leaf = 0;
        gh->flags = tree_leaf_flags(h.flags);
    }
}

// _expand_child (mcts.py:210-221) of action a of `node` (header h): both collapse children at once, as qttt_expand
// (expand_pair: one step_core_both() for the two), in the records `used` and `used + 1`, and the one that `bit` picks becomes (node, h): a fresh node has no priors, so it is
// the leaf and its header stays in registers.  False when nothing was allocated: the action is not legal (cannot happen
// for one that the descent chose), or the children do not fit the pool (`overflow`).
__device__ __forceinline__ bool tree_expand_child(const TreeView &v, int64_t g, int32_t &node, TreeNodeHdr &h, int a, u32 bit,
                                                  int32_t &used, const uint8_t *lut, u32 lane, bool &overflow) {
    const Expansion e = expand_pair(h.P, h.Q, pair_action<false>(a), lut);
    if (e.kids == 0u || (int64_t)used + e.kids > v.capacity) {
        overflow = e.kids != 0u;
        return false;
    }
    const bool turn = !(h.flags & TN_TURN);
    TreeNodeHdr c[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        int w, t;
        update_winner_from_step(e.P[k], e.xo[k], lut, w, t);
        c[k] = tree_node(e.P[k], e.Q, turn, w, t, legal_mask_of(classical_with_autofill(e.P[k])));
    }
    tree_write_node(v, g, used, c[0], lane, 0u);
    if (e.kids == 2u) tree_write_node(v, g, used + 1, c[1], lane, 1u);
    if (lane == 0u) v.slots(g, node)[a].child = used | (e.kids == 2u ? TREE_CHILD_PAIR : 0);
    const u32 pick = e.kids == 2u ? bit : 0u;
    node = used + (int32_t)pick;
    h = pick ? c[1] : c[0];
    used += (int32_t)e.kids;
    return true;
}

// _select (mcts.py:269-280): one path of game g from `root` to a leaf, the only descent of the device trees.  bits = the
// collapse choices, bit d = the child at path depth d; score(W, N word, prior, Ntot word, c_puct) = the selection score
// of a legal action, tree_score or its in-flight form.  The path lives in lane registers: lane d < depth holds edge d as
// (edge_node, edge_action), and the caller stores it where it belongs.  An expansion that does not fit ends the descent
// on the node it stands on, and that edge is not on the path.
// The winner is lane 0's for the whole wave: under NaN scores the lanes of wave_argmax disagree, and the path, the
// expansion and whatever the caller marks must be one path (with ordinary scores every lane holds the same a).
// Against the two copies of the loop that this replaced (profiles/tree_descent/treebench_parent_vs_change.txt: one
// MI355X, the two libraries alternating, medians of three processes, us; [the old code's max - min]):
//   qttt_tree_select per launch   4 096 games uniform 14.03 -> 13.94 [0.10], bf16 15.10 -> 14.82 [0.31]; 65 536 games
//                                 93.46 -> 92.58 [1.69], 113.89 -> 112.44 [0.93]; 262 144 games 375.16 -> 370.31 [2.12],
//                                 446.22 -> 442.11 [2.09]
//   a value rollout, bf16         4 096 games K = 1 / 8 / 32: 78.36 -> 78.22 [0.13], 14.28 -> 14.17 [0.02], 9.78 -> 9.68 [0.12];
//                                 65 536 games 180.88 -> 179.43 [0.66], 152.55 -> 150.76 [0.37], 124.93 -> 123.63 [0.29]
//   a value rollout, f32          4 096 games 102.36 -> 102.19 [0.37], 26.87 -> 26.65 [0.16], 23.66 -> 23.50 [0.03];
//                                 65 536 games 393.57 -> 392.25 [1.84], 361.64 -> 360.06 [0.85], 331.05 -> 330.09 [0.17]
// Both kernels keep their registers, their 2 048 B of LDS and no scratch (device_code_parent_vs_change.txt there).
// The rule at the root of a descent.  TreePuctRoot: none, the root is scored like every node (`on` is a constant, so the
// descents that use it hold no trace of the hook).  A rule with on = true is asked once, at depth 0, with the root's header
// and every lane's slot, and returns the wave-uniform action to take, or -1 for the ordinary score
// (qttt_tree_gumbel_kernels.h's GumbelRootRule).
struct TreePuctRoot {
    static constexpr bool on = false;
    __device__ __forceinline__ int operator()(const TreeNodeHdr &, const TreeSlot &, u32) const { return -1; }
};
struct TreeDescent {
    int32_t leaf, depth;
    TreeNodeHdr h;                     // the leaf's header
    bool overflow;                     // the expansion did not fit
    int32_t edge_node;                 // lane d < depth: edge d
    u32 edge_action;
};
template <typename Score, typename Root = TreePuctRoot>
__device__ __forceinline__ TreeDescent tree_descend(const TreeView &v, int64_t g, int32_t root, u32 bits, int32_t &used,
                                                    const uint8_t *lut, u32 lane, double c_puct, Score &&score,
                                                    const Root &root_rule = Root()) {
    TreeDescent d;
    d.leaf = root; d.depth = 0;
    d.overflow = false;
    d.edge_node = 0; d.edge_action = 0u;
    d.h = *v.hdr(g, root);
    while ((d.h.flags & TN_PRIORS) && !(d.h.flags & TN_TERMINAL) && d.h.legal != 0ull && d.depth < QTTT_TREE_MAX_DEPTH) {
        const bool legal = lane < 36u && ((d.h.legal >> lane) & 1ull);
        TreeSlot s;
        s.W = 0.0; s.N = 0u; s.child = -1;
        if (lane < 36u) s = v.slots(g, d.leaf)[lane];
        int a = -1;
        if constexpr (Root::on) {
            if (d.depth == 0) a = root_rule(d.h, s, lane);
        }
        if (a < 0) {                                             // always, but at a root whose rule has chosen
            double sc = 0.0;
            if (legal) sc = score(s.W, s.N, tree_prior(v, g, d.leaf, d.h, lane), d.h.Ntot, c_puct);
            a = __builtin_amdgcn_readfirstlane(wave_argmax(legal, sc, lane));
        }
        const int32_t child = __shfl(s.child, a);
        const u32 bit = (bits >> d.depth) & 1u;
        const int32_t parent = d.leaf;
        if (child >= 0) {                                        // descend (mcts.py:275-276)
            d.leaf = (child & (TREE_CHILD_PAIR - 1)) + ((child & TREE_CHILD_PAIR) ? (int32_t)bit : 0);
            d.h = *v.hdr(g, d.leaf);
        } else if (!tree_expand_child(v, g, d.leaf, d.h, a, bit, used, lut, lane, d.overflow)) {
            break;
        }
        if ((int32_t)lane == d.depth) { d.edge_node = parent; d.edge_action = (u32)a; }
        ++d.depth;
        if (child < 0) break;                                    // a fresh node has no priors: it is the leaf
    }
    return d;
}

__global__ __launch_bounds__(TREE_BLOCK) void tree_select_kernel(void *tree, int64_t games, int64_t capacity, u64 seed,
                                                                 u32 rollout_idx, u64 board_offset, double c_puct,
                                                                 u64 *leafP, u64 *leafQ) {
    __shared__ __attribute__((aligned(16))) uint8_t lut[LINE_LUT_BYTES];
    fill_line_lut<TREE_BLOCK>(lut);                              // ends with the workgroup barrier
    const int64_t g = (int64_t)blockIdx.x * TREE_GAMES_PER_BLOCK + threadIdx.x / 64;
    const u32 lane = threadIdx.x & 63u;
    if (g >= games) return;
    const TreeView v = tree_view(tree, games, capacity);
    TreeGame *gh = &v.games[g];
    int32_t used = gh->used;
    // the collapse choices of this rollout: bit d = the child at path depth d (qttt_hash's low word)
    const u64 key = launch_key(seed, QTTT_TREE_SELECT_BASE + rollout_idx);
    const u32 bits = lowbias32(fold_id(board_offset + (u64)g) ^ (u32)key);
    const TreeDescent d = tree_descend(v, g, gh->root, bits, used, lut, lane, c_puct,
                                       [](double W, u32 N, double prior, u32 Ntot, double c) {
                                           return tree_score(W, N, prior, tree_sqrt(Ntot), c);
                                       });
    if ((int32_t)lane < d.depth) {                               // entries at and past depth stay as they were
        gh->path_node[lane] = d.edge_node;
        gh->path_action[lane] = (uint8_t)d.edge_action;
    }
    if (lane == 0u) {
        gh->used = used;
        gh->depth = d.depth;
        gh->leaf = d.leaf;
        gh->flags = (gh->flags & TG_OVERFLOW) | (d.overflow ? TG_OVERFLOW : 0u) | tree_leaf_flags(d.h.flags);
        leafP[g] = d.h.P;
        leafQ[g] = d.h.Q;
    }
}

// _backpropogate (mcts.py:175-183), shared by tree_backup_kernel and tree_value_rollout_kernel
// (qttt_tree_value_kernels.h).  Lane d < depth owns the d-th edge of the recorded path: tree_edge_load reads its
// statistics, tree_edge_store writes them back with a value `val` seen by the player to move at the leaf: the deepest
// edge gets -val (r = -r, mcts.py:179), the one above +val, ...  Two halves, so that a kernel with several games per
// wave can have the loads of all of them in flight before the first store.
struct TreeEdge {
    TreeSlot *slot;
    TreeNodeHdr *hdr;
    double W;
    u32 N, Ntot;
    bool on;
};
__device__ __forceinline__ TreeEdge tree_edge_load(const TreeView &v, int64_t g, const TreeGame *gh, int32_t depth, u32 lane) {
    TreeEdge e;
    e.on = (int32_t)lane < depth;
    e.slot = nullptr; e.hdr = nullptr;
    e.W = 0.0; e.N = 0u; e.Ntot = 0u;
    if (e.on) {
        const int32_t node = gh->path_node[lane];
        const u32 a = gh->path_action[lane];
        e.slot = &v.slots(g, node)[a];
        e.hdr = v.hdr(g, node);
        e.W = e.slot->W;
        e.N = e.slot->N;
        e.Ntot = e.hdr->Ntot;
    }
    return e;
}
// what edge `lane` of a path of `depth` edges gets of the leaf's value: r = -r per level, deepest first (mcts.py:179)
__device__ __forceinline__ double tree_edge_value(int32_t depth, u32 lane, double val) {
    return ((depth - (int32_t)lane) & 1) ? -val : val;
}
__device__ __forceinline__ void tree_edge_store(const TreeEdge &e, int32_t depth, u32 lane, double val) {
#pragma clang fp contract(off)
    if (e.on) {
        e.slot->W = e.W + tree_edge_value(depth, lane, val);
        e.slot->N = e.N + 1u;
        e.hdr->Ntot = e.Ntot + 1u;
    }
}
// _simulate's priors (mcts.py:188-191): a leaf with flags lf that is not terminal and has no priors gets them, lane
// a < 36 writing prob(a) of the network's row, or (network = false) the uniform flag alone; any other leaf is left alone
template <typename F>
__device__ __forceinline__ void tree_leaf_priors(const TreeView &v, int64_t g, int32_t leaf, u32 lf, u32 lane, bool network,
                                                 F &&prob) {
    if ((lf & (TN_PRIORS | TN_TERMINAL)) == 0u) {
        if (network && lane < 36u) v.prior(g, leaf)[lane] = prob(lane);
        if (lane == 0u) v.hdr(g, leaf)->flags = lf | TN_PRIORS | (network ? 0u : TN_UNIFORM);
    }
}

// lane d < depth updates the d-th edge of the path; the leaf's priors go in with it
__global__ __launch_bounds__(TREE_BLOCK) void tree_backup_kernel(void *tree, int64_t games, int64_t capacity,
                                                                 const int8_t *result, u32 n_sims,
                                                                 const float *leaf_probs) {
    const int64_t g = (int64_t)blockIdx.x * TREE_GAMES_PER_BLOCK + threadIdx.x / 64;
    const u32 lane = threadIdx.x & 63u;
    if (g >= games) return;
    const TreeView v = tree_view(tree, games, capacity);
    const TreeGame *gh = &v.games[g];
    const int32_t depth = gh->depth, leaf = gh->leaf;
    const u32 gflags = gh->flags;
    int r = 0;
    for (u32 s = lane; s < n_sims; s += 64u) r += (int)result[g * (int64_t)n_sims + s];
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) r += __shfl_xor(r, m);
    if (!(gflags & TG_LEAF_TURN)) r = -r;                        // r if leaf.turn else -r (mcts.py:171)
    tree_edge_store(tree_edge_load(v, g, gh, depth, lane), depth, lane, (double)r / (double)n_sims);      // mcts.py:173
    tree_leaf_priors(v, g, leaf, v.hdr(g, leaf)->flags, lane, leaf_probs != nullptr,
                     [&](u32 a) { return leaf_probs[g * 36 + a]; });
}

__global__ __launch_bounds__(TREE_BLOCK) void tree_sync_kernel(void *tree, int64_t games, int64_t capacity,
                                                               const u64 *pP, const u64 *pQ) {
    __shared__ __attribute__((aligned(16))) uint8_t lut[LINE_LUT_BYTES];
    fill_line_lut<TREE_BLOCK>(lut);
    const int64_t g = (int64_t)blockIdx.x * TREE_GAMES_PER_BLOCK + threadIdx.x / 64;
    const u32 lane = threadIdx.x & 63u;
    if (g >= games) return;
    const TreeView v = tree_view(tree, games, capacity);
    TreeGame *gh = &v.games[g];
    const int32_t root = gh->root, used = gh->used;
    const u64 P = pP[g], Q = pQ[g];
    const TreeNodeHdr h = *v.hdr(g, root);
    if (h.P == P && h.Q == Q) return;                            // the game did not move
    // the root child equal to the position (mcts.py:325-329): lane a looks at action a's children
    int32_t found = -1;
    if (lane < 36u) {
        const int32_t c = v.slots(g, root)[lane].child;
        if (c >= 0) {
            const int32_t c0 = c & (TREE_CHILD_PAIR - 1);
            const TreeNodeHdr *h0 = v.hdr(g, c0);
            if (h0->P == P && h0->Q == Q) found = c0;
            else if (c & TREE_CHILD_PAIR) {
                const TreeNodeHdr *h1 = v.hdr(g, c0 + 1);
                if (h1->P == P && h1->Q == Q) found = c0 + 1;
            }
        }
    }
    const u64 hit = __ballot(found >= 0);
    if (hit) {
        const int32_t nr = __shfl(found, __builtin_ctzll(hit));
        if (lane == 0u) gh->root = nr;
        return;
    }
    if ((int64_t)used + 1 > capacity) {                          // a fresh root does not fit
        if (lane == 0u) gh->flags |= TG_OVERFLOW;
        return;
    }
    const TreeNodeHdr f = tree_node_of(P, Q, !(h.flags & TN_TURN), lut);      // _expand_child of the move (:320-323)
    tree_write_node(v, g, used, f, lane, 0u);
    if (lane == 0u) { gh->root = used; gh->used = used + 1; }
}

// Everything one lane stored before this point is what every lane of the wave loads after it (the forwarding table
// and the LDS window of tree_compact_kernel are handed from lane to lane of one wave, never between waves).
__device__ __forceinline__ void tree_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// a child word's nodes as [c0, c0 + n), or n = 0 when it is -1 or does not lie in (parent, used): the compaction
// never follows an index that a well-formed tree cannot hold
__device__ __forceinline__ int tree_child_span(int32_t child, int32_t parent, int32_t used, int32_t &c0) {
    c0 = child & (TREE_CHILD_PAIR - 1);
    const int n = (child & TREE_CHILD_PAIR) ? 2 : 1;
    return (child >= 0 && c0 > parent && c0 <= used - n) ? n : 0;
}

// MCTS._prune as done by sync (mcts.py:222-231, 330-337): stable, in-place compaction of the nodes reachable from the
// root.  fwd = i32[games][capacity] scratch, fwd[g][i] = the new index of node i or -1.
//
// Why two ascending sweeps are enough: a child's index is larger than its parent's (bump allocation) and a node has one
// parent, so when sweep A reaches node i every mark i can ever get has been made, and fwd[i] = the number of reachable
// nodes before it.  Sweep B moves record i to fwd[i] <= i; it holds one record at a time: every lane's loads of record
// i are in registers before its stores (the stored values depend on them), the destination fwd[i] is either i itself
// (each lane rewrites exactly the bytes it loaded) or a record below i, and every reachable record below i has been
// read already, so a store never lands on a record that is still to be read.
//
// Sweep A reads the marks 64 at a time: lane l of a chunk holds node base + l.  Marks made by parents of earlier chunks
// come from fwd (-2 = marked); a child that falls into its parent's own chunk is marked in the wave's 64-entry LDS
// window instead, and the chunk's reachable set is re-read from the window after every node.  The nodes of a chunk
// are taken in ascending order and a child lies above its parent, so a window bit set while node j is processed
// belongs to a node above j that has not been passed yet: nothing is missed and nothing is visited twice.
//
// Every loop is bounded by `used` (the chunk loops) or by 64 (the nodes of a chunk); no atomics, no waiting on memory.
__global__ __launch_bounds__(TREE_BLOCK) void tree_compact_kernel(void *tree, int64_t games, int64_t capacity,
                                                                  int32_t *fwd_all) {
    __shared__ int32_t window[TREE_GAMES_PER_BLOCK][64];
    const int64_t g = (int64_t)blockIdx.x * TREE_GAMES_PER_BLOCK + threadIdx.x / 64;
    const u32 lane = threadIdx.x & 63u;
    if (g >= games) return;
    const TreeView v = tree_view(tree, games, capacity);
    TreeGame *gh = &v.games[g];
    const int32_t root = gh->root, used = gh->used;
    if (used < 1 || (int64_t)used > capacity || root < 0 || root >= used) return;      // not a tree of this pool
    if (root == 0 && used == 1) return;                                               // already compact
    int32_t *fwd = fwd_all + g * capacity;
    int32_t *win = window[threadIdx.x / 64];
    const u32 gflags = gh->flags, rflags = v.hdr(g, root)->flags;

    // ---- sweep A: reachability and the new indices
    for (int32_t i = root + (int32_t)lane; i < used; i += 64) fwd[i] = -1;
    int32_t count = 0;
    for (int32_t base = root; base < used; base += 64) {
        tree_wave_sync();                                        // the -1s and the marks of the earlier chunks
        const int32_t i = base + (int32_t)lane;
        win[lane] = (i == root || (i < used && fwd[i] != -1)) ? 1 : 0;
        u64 reach = 0ull, passed = 0ull;
        for (int it = 0; it <= 64; ++it) {                       // a node per turn, and the turn that finds none left
            tree_wave_sync();
            reach = __ballot(win[lane] != 0);
            const u64 pending = reach & ~passed;
            if (!pending) break;
            const int j = __builtin_ctzll(pending);
            passed = j == 63 ? ~0ull : (2ull << j) - 1ull;
            const int32_t node = base + j;
            if (lane < 36u) {
                int32_t c0;
                const int n = tree_child_span(v.slots(g, node)[lane].child, node, used, c0);
                if (n) {
                    if (c0 < base + 64) win[c0 - base] = 1;
                    else fwd[c0] = -2;
                }
                if (n == 2) {                                    // the other half of a pair
                    if (c0 + 1 < base + 64) win[c0 + 1 - base] = 1;
                    else fwd[c0 + 1] = -2;
                }
            }
        }
        if (i < used && ((reach >> lane) & 1ull)) fwd[i] = count + __builtin_popcountll(reach & ((1ull << lane) - 1ull));
        count += __builtin_popcountll(reach);
    }
    if (root == 0 && count == used) return;                      // already compact: not a byte of the tree changes
    tree_wave_sync();

    // ---- sweep B: move the reachable records down, in ascending order, with their child words rewritten.  A record
    // is 38 vectors of 16 B: the header is two (lane 36 and 37), slot a is vector 2 + a (lane a), its child the last word
    int32_t dst = 0;
    for (int32_t base = root; base < used; base += 64) {
        const int32_t i = base + (int32_t)lane;
        const u64 reach = __ballot(i < used && fwd[i] >= 0);
        for (u64 pending = reach; pending; pending &= pending - 1ull, ++dst) {      // at most 64 nodes
            const int32_t node = base + __builtin_ctzll(pending);
            const u32 nflags = v.hdr(g, node)->flags;
            const bool network = (nflags & TN_PRIORS) && !(nflags & TN_UNIFORM);
            const u32 vec = lane < 36u ? lane + 2u : lane - 36u;
            TreeVec r = {0u, 0u, 0u, 0u};
            float p = 0.0f;
            if (lane < 38u) r = reinterpret_cast<const TreeVec *>(v.hdr(g, node))[vec];
            if (lane < 36u) {
                int32_t c0;
                const int32_t child = (int32_t)r.w;
                const int n = tree_child_span(child, node, used, c0);
                r.w = n ? (u32)(fwd[c0] | (child & TREE_CHILD_PAIR)) : ~0u;
                if (network) p = v.prior(g, node)[lane];
            }
            if (lane < 38u) reinterpret_cast<TreeVec *>(v.hdr(g, dst))[vec] = r;
            if (lane < 36u && network) v.prior(g, dst)[lane] = p;
        }
    }
    if (lane == 0u) {                                            // as tree_reset_kernel's, for this root
        gh->used = count; gh->root = 0; gh->depth = 0; gh->leaf = 0;
        gh->flags = (gflags & TG_OVERFLOW) | tree_leaf_flags(rflags);
    }
}

struct TreeRootOut {
    int32_t *N;
    double *W, *Q, *P;
    int32_t *Ntot;
    uint8_t *choose;
    int32_t *nodes_used;
    uint8_t *overflow;
};

// what lane a sees of game g's root: the node's header, whether action a is legal, and its slot (empty when it is not)
struct TreeRootLane {
    TreeNodeHdr h;
    TreeSlot s;
    bool legal;
};
__device__ __forceinline__ TreeRootLane tree_root_lane(const TreeView &v, int64_t g, u32 lane) {
    TreeRootLane r;
    const int32_t root = v.games[g].root;
    r.h = *v.hdr(g, root);
    r.legal = lane < 36u && ((r.h.legal >> lane) & 1ull);
    r.s.W = 0.0; r.s.N = 0u; r.s.child = -1;
    if (r.legal) r.s = v.slots(g, root)[lane];
    return r;
}
// Q of a slot (mcts.py:181: W / N, 0 while unvisited) and MCTS.choose over the wave (mcts.py:308-315): -inf for
// unvisited actions, ties to the lowest; -1 when no action is legal
__device__ __forceinline__ double tree_slot_q(const TreeSlot &s) { return s.N ? s.W / (double)s.N : 0.0; }
__device__ __forceinline__ int tree_choose(const TreeRootLane &r, u32 lane) {
    return wave_argmax(r.legal, r.s.N ? tree_slot_q(r.s) : -__builtin_inf(), lane);
}

__global__ __launch_bounds__(TREE_BLOCK) void tree_root_kernel(const void *tree, int64_t games, int64_t capacity,
                                                               TreeRootOut o) {
    const int64_t g = (int64_t)blockIdx.x * TREE_GAMES_PER_BLOCK + threadIdx.x / 64;
    const u32 lane = threadIdx.x & 63u;
    if (g >= games) return;
    const TreeView v = tree_view(const_cast<void *>(tree), games, capacity);
    const TreeGame *gh = &v.games[g];
    const TreeRootLane r = tree_root_lane(v, g, lane);
    if (lane < 36u) {
        const int64_t j = g * 36 + lane;
        if (o.N) o.N[j] = (int32_t)r.s.N;
        if (o.W) o.W[j] = r.s.W;
        if (o.Q) o.Q[j] = tree_slot_q(r.s);
        if (o.P) o.P[j] = (r.legal && (r.h.flags & TN_PRIORS)) ? tree_prior(v, g, gh->root, r.h, lane) : 0.0;
    }
    const int a = tree_choose(r, lane);
    if (lane == 0u) {
        if (o.Ntot) o.Ntot[g] = (int32_t)r.h.Ntot;
        if (o.choose) o.choose[g] = a < 0 ? (uint8_t)255 : (uint8_t)a;
        if (o.nodes_used) o.nodes_used[g] = gh->used;
        if (o.overflow) o.overflow[g] = (gh->flags & TG_OVERFLOW) ? 1 : 0;
    }
}

__global__ __launch_bounds__(256) void tree_sqrt_kernel(u32 first, int64_t n, double *out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = tree_sqrt(first + (u32)i);
}

__global__ __launch_bounds__(256) void tree_score_kernel(const double *W, const u32 *N, const double *prior, const u32 *Ntot,
                                                         double c_puct, int64_t n, double *out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = tree_score(W[i], N[i], prior[i], tree_sqrt(Ntot[i]), c_puct);
}

}  // namespace

#endif  // QTTT_TREE_KERNELS_H
