// qttt_tree_leaves_kernels.h — leaf-parallel rounds of the device search trees (include/qttt_tree_leaves.h, DESIGN.md
// §17): tree_select_batch_kernel makes K descents per game, kept apart by virtual loss, and tree_backup_batch_kernel backs
// the K evaluated leaves up; qttt_evaluate runs between the two on the games * K leaves, as it is.
//
// Mapping: qttt_tree_kernels.h's.  ONE WAVEFRONT PER GAME, lane a = action a, four games per 256-thread workgroup, the LDS
// line table for the expansions.  The K descents of a game are sequential by construction (descent j + 1 scores what
// descent j left in flight); the parallelism is across games and in the games * K-row network launch.
//
// Unlike tree_select_kernel, a wave here re-reads what its own lanes wrote earlier in the launch: the in-flight bits of N
// and Ntot (written by lane d for edge d, read by lane a for action a), a child word written by lane 0, a fresh child's
// header and slots, Ntot of the root that all K paths share, and, in the backup, the leaf's priors flag.  Every such
// store is separated from its loads by tree_wave_sync(), as in tree_compact_kernel: one at the top of every descent and
// one after every backed-up record.  WITHIN a descent nothing written is read again: a fresh child is the leaf and its
// header stays in registers, and the in-flight marks touch the N and Ntot words only, which the descent's expansion
// (child word, fresh records) does not write.
//
// In flight: bits 24-31 of a slot's N word and of a node's Ntot word count the round's descents through them; N and Ntot
// proper stay below 2^24 (QTTT_TREE_MAX_ROLLOUTS), K <= 64 < 256, and W is never touched by select.  Every loop is
// bounded: K <= QTTT_TREE_MAX_LEAVES, depth <= QTTT_TREE_MAX_DEPTH.  No atomics, no waiting on memory.
#ifndef QTTT_TREE_LEAVES_KERNELS_H
#define QTTT_TREE_LEAVES_KERNELS_H
#include "qttt_tree_value_kernels.h"
#include "qttt_tree_leaves.h"

namespace {

constexpr u32 TREE_FLIGHT_SHIFT = 24u, TREE_FLIGHT_ONE = 1u << TREE_FLIGHT_SHIFT, TREE_COUNT_MASK = TREE_FLIGHT_ONE - 1u;
constexpr u32 TP_OVERFLOW = 1u, TP_LEAF_TURN = 2u, TP_LEAF_TERMINAL = 4u;        // path-record flags: the TG_ bits

struct TreePathRec {                   // 64 B, include/qttt_tree_leaves.h
    int32_t leaf;
    uint8_t depth, flags, pad[2];
    uint8_t action[QTTT_TREE_MAX_DEPTH];
    uint8_t pad2[6];
    int32_t node[QTTT_TREE_MAX_DEPTH];
};
static_assert(sizeof(TreePathRec) == QTTT_TREE_PATH_BYTES && offsetof(TreePathRec, action) == 8 &&
              offsetof(TreePathRec, node) == 24, "path record");
static_assert(TP_OVERFLOW == TG_OVERFLOW && TP_LEAF_TURN == TG_LEAF_TURN && TP_LEAF_TERMINAL == TG_LEAF_TERMINAL, "flag bits");

// a statistics word with its in-flight visits counted in: n + f
__device__ __forceinline__ u32 tree_effective(u32 word) { return (word & TREE_COUNT_MASK) + (word >> TREE_FLIGHT_SHIFT); }

// tree_score on effective statistics (include/qttt_tree_leaves.h): with no visit in flight, tree_score bit for bit
// (W - vloss * 0.0 is W)
__device__ __forceinline__ double tree_score_in_flight(double W, u32 Nword, double prior, double sq, double c_puct, double vloss) {
#pragma clang fp contract(off)
    const u32 Ne = tree_effective(Nword);
    const double We = W - vloss * (double)(Nword >> TREE_FLIGHT_SHIFT);
    const double q = Ne ? We / (double)Ne : 0.0;
    const double u = prior * sq / (double)(1u + Ne);
    return q + c_puct * u;
}

__global__ __launch_bounds__(TREE_BLOCK) void tree_select_batch_kernel(void *tree, int64_t games, int64_t capacity, u64 seed,
                                                                       u32 rollout_idx0, u32 leaves, u64 board_offset,
                                                                       double c_puct, double vloss, TreePathRec *paths,
                                                                       u64 *leafP, u64 *leafQ) {
    __shared__ __attribute__((aligned(16))) uint8_t lut[LINE_LUT_BYTES];
    fill_line_lut<TREE_BLOCK>(lut);                              // ends with the workgroup barrier
    const int64_t g = (int64_t)blockIdx.x * TREE_GAMES_PER_BLOCK + threadIdx.x / 64;
    const u32 lane = threadIdx.x & 63u;
    if (g >= games) return;
    const TreeView v = tree_view(tree, games, capacity);
    TreeGame *gh = &v.games[g];
    const int32_t root = gh->root;
    int32_t used = gh->used;
    const u32 id = fold_id(board_offset + (u64)g);
    u32 overflow = 0u;
    for (u32 j = 0; j < leaves; ++j) {
        tree_wave_sync();                                        // what the earlier descents stored
        const u32 bits = lowbias32(id ^ (u32)launch_key(seed, QTTT_TREE_SELECT_BASE + rollout_idx0 + j));
        int32_t node = root, depth = 0;
        int32_t my_node = 0;                                     // lane d: edge d of this descent's path
        u32 my_action = 0u, over = 0u;
        TreeNodeHdr h = *v.hdr(g, node);
        while ((h.flags & TN_PRIORS) && !(h.flags & TN_TERMINAL) && h.legal != 0ull && depth < QTTT_TREE_MAX_DEPTH) {
            const bool legal = lane < 36u && ((h.legal >> lane) & 1ull);
            TreeSlot s;
            s.W = 0.0; s.N = 0u; s.child = -1;
            if (lane < 36u) s = v.slots(g, node)[lane];
            double score = 0.0;
            if (legal)
                score = tree_score_in_flight(s.W, s.N, tree_prior(v, g, node, h, lane), tree_sqrt(tree_effective(h.Ntot)), c_puct, vloss);
            // lane 0's winner for the whole wave: under NaN scores the lanes of wave_argmax disagree, and the marks, the
            // record and the expansion of a descent must be one path (with ordinary scores every lane holds the same a)
            const int a = __builtin_amdgcn_readfirstlane(wave_argmax(legal, score, lane));
            const int32_t child = __shfl(s.child, a);
            const u32 bit = (bits >> depth) & 1u;
            if (child >= 0) {                                    // descend
                if ((int32_t)lane == depth) { my_node = node; my_action = (u32)a; }
                ++depth;
                node = (child & (TREE_CHILD_PAIR - 1)) + ((child & TREE_CHILD_PAIR) ? (int32_t)bit : 0);
                h = *v.hdr(g, node);
                continue;
            }
            // the expansion of tree_select_kernel: both collapse children at once
            u32 Q0 = (u32)h.Q, Q1 = (u32)(h.Q >> 32), P0a, P1a, P0b, P1b, xo0, xo1;
            const u32 kids = step_core_both((u32)h.P, (u32)(h.P >> 32), Q0, Q1, pair_action<false>(a), lut, P0a, P1a, P0b, P1b, xo0, xo1);
            if (kids == 0u || (int64_t)used + kids > capacity) { // cannot happen for a legal action / does not fit
                over = kids == 0u ? 0u : TP_OVERFLOW;
                break;
            }
            const bool turn = !(h.flags & TN_TURN);
            TreeNodeHdr c[2];
            const u64 kidP[2] = {(u64)P0a | ((u64)P1a << 32), (u64)P0b | ((u64)P1b << 32)};
            const u32 xo[2] = {xo0, xo1};
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                int w, t;
                update_winner_from_step(kidP[k], xo[k], lut, w, t);
                c[k] = tree_node(kidP[k], (u64)Q0 | ((u64)Q1 << 32), turn, w, t, legal_mask_of(classical_with_autofill(kidP[k])));
            }
            tree_write_node(v, g, used, c[0], lane, 0u);
            if (kids == 2u) tree_write_node(v, g, used + 1, c[1], lane, 1u);
            if (lane == 0u) v.slots(g, node)[a].child = used | (kids == 2u ? TREE_CHILD_PAIR : 0);
            if ((int32_t)lane == depth) { my_node = node; my_action = (u32)a; }
            ++depth;
            const u32 pick = kids == 2u ? bit : 0u;
            node = used + (int32_t)pick;
            h = pick ? c[1] : c[0];
            used += (int32_t)kids;
            break;                                               // a fresh node has no priors: it is the leaf
        }
        overflow |= over;
        // one in-flight visit on every edge of the path: lane d owns edge d, and the edges lie in different nodes
        TreePathRec *rec = paths + (g * (int64_t)leaves + j);
        if ((int32_t)lane < depth) {
            TreeSlot *slot = &v.slots(g, my_node)[my_action];
            TreeNodeHdr *nh = v.hdr(g, my_node);
            slot->N = slot->N + TREE_FLIGHT_ONE;
            nh->Ntot = nh->Ntot + TREE_FLIGHT_ONE;
            rec->node[lane] = my_node;
            rec->action[lane] = (uint8_t)my_action;
        }
        if (lane == 0u) {
            rec->leaf = node;
            rec->depth = (uint8_t)depth;
            rec->flags = (uint8_t)(over | (h.flags & TN_TURN ? TP_LEAF_TURN : 0u) | (h.flags & TN_TERMINAL ? TP_LEAF_TERMINAL : 0u));
            leafP[g * (int64_t)leaves + j] = h.P;
            leafQ[g * (int64_t)leaves + j] = h.Q;
        }
    }
    if (lane == 0u) {                                            // the recorded path as tree_compact_kernel leaves it
        const u32 rflags = v.hdr(g, root)->flags;                // (select never writes a node's flags)
        gh->used = used;
        gh->depth = 0;
        gh->leaf = root;
        gh->flags = (gh->flags & TG_OVERFLOW) | overflow | (rflags & TN_TURN ? TG_LEAF_TURN : 0u) |
                    (rflags & TN_TERMINAL ? TG_LEAF_TERMINAL : 0u);
    }
}

// record j + 1 is fetched while record j is backed up: the records are not written here, so their loads need no order
struct TreePathLane {
    int32_t leaf, node;
    u32 depth, action;
    float value;
};
__device__ __forceinline__ TreePathLane tree_path_lane(const TreePathRec *paths, const float *leaf_value, int64_t row, u32 lane) {
    const TreePathRec *rec = paths + row;
    TreePathLane p;
    p.leaf = rec->leaf;
    p.depth = rec->depth;
    p.node = lane < (u32)QTTT_TREE_MAX_DEPTH ? rec->node[lane] : 0;
    p.action = lane < (u32)QTTT_TREE_MAX_DEPTH ? rec->action[lane] : 0u;
    p.value = leaf_value[row];
    return p;
}

__global__ __launch_bounds__(TREE_BLOCK) void tree_backup_batch_kernel(void *tree, int64_t games, int64_t capacity, u32 leaves,
                                                                       const TreePathRec *paths, const float *leaf_value,
                                                                       const float *leaf_probs) {
#pragma clang fp contract(off)
    const int64_t g = (int64_t)blockIdx.x * TREE_GAMES_PER_BLOCK + threadIdx.x / 64;
    const u32 lane = threadIdx.x & 63u;
    if (g >= games) return;
    const TreeView v = tree_view(tree, games, capacity);
    const int64_t row0 = g * (int64_t)leaves;
    TreePathLane next = tree_path_lane(paths, leaf_value, row0, lane);
    for (u32 j = 0; j < leaves; ++j) {
        const TreePathLane p = next;
        if (j + 1u < leaves) next = tree_path_lane(paths, leaf_value, row0 + j + 1u, lane);
        // a record that does not lie in the pool is skipped (wave-uniform: every lane sees every lane's entry)
        const bool edge = lane < p.depth;
        const bool bad_edge = edge && (p.node < 0 || (int64_t)p.node >= capacity || p.action >= 36u);
        if (p.depth > (u32)QTTT_TREE_MAX_DEPTH || p.leaf < 0 || (int64_t)p.leaf >= capacity || __ballot(bad_edge) != 0ull) continue;
        const u32 lf = v.hdr(g, p.leaf)->flags;
        const double val = (lf & TN_TERMINAL) ? tree_terminal_value(lf) : (double)p.value;
        if (edge) {                                              // tree_edge_store's signs: the deepest edge gets -val
            TreeSlot *slot = &v.slots(g, p.node)[p.action];
            TreeNodeHdr *nh = v.hdr(g, p.node);
            const double rv = ((p.depth - lane) & 1u) ? -val : val;
            slot->W = slot->W + rv;
            slot->N = slot->N + 1u - TREE_FLIGHT_ONE;
            nh->Ntot = nh->Ntot + 1u - TREE_FLIGHT_ONE;
        }
        tree_leaf_priors(v, g, p.leaf, lf, lane, true, [&](u32 a) { return leaf_probs[(row0 + j) * 36 + a]; });
        tree_wave_sync();                                        // the next record may pass the same edges and leaf
    }
}

}  // namespace

#endif  // QTTT_TREE_LEAVES_KERNELS_H
