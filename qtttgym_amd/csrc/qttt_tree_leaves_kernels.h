// qttt_tree_leaves_kernels.h — leaf-parallel rounds of the device search trees (include/qttt_tree_leaves.h, DESIGN.md
// §17): tree_select_batch_kernel makes K descents per game, kept apart by virtual loss, and tree_backup_batch_kernel backs
// the K evaluated leaves up; qttt_evaluate runs between the two on the games * K leaves, as it is.
//
// Mapping: qttt_tree_kernels.h's.  ONE WAVEFRONT PER GAME, lane a = action a, four games per 256-thread workgroup, the LDS
// line table for the expansions.  The K descents of a game are sequential by construction (descent j + 1 scores what
// descent j left in flight); the parallelism is across games and in the games * K-row network launch.
//
// A descent is qttt_tree_kernels.h's tree_descend, the one tree_select_kernel makes, scored by tree_score_in_flight.
// Unlike tree_select_kernel, a wave here re-reads what its own lanes wrote earlier in the launch: the in-flight bits of N
// and Ntot (written by lane d for edge d, read by lane a for action a), a child word written by lane 0, a fresh child's
// header and slots, Ntot of the root that all K paths share, and, in the backup, the leaf's priors flag.  Every such
// store is separated from its loads by tree_wave_sync(), as in tree_compact_kernel: one at the top of every descent and
// one after every backed-up record.  WITHIN a descent nothing written is read again (tree_descend keeps the fresh child's
// header and the path in registers), and the in-flight marks, made after it, touch the N and Ntot words only, which the
// descent's expansion (child word, fresh records) does not write.
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

struct TreePathRec {                   // 64 B, include/qttt_tree_leaves.h
    int32_t leaf;
    uint8_t depth, flags, pad[2];
    uint8_t action[QTTT_TREE_MAX_DEPTH];
    uint8_t pad2[6];
    int32_t node[QTTT_TREE_MAX_DEPTH];
};
static_assert(sizeof(TreePathRec) == QTTT_TREE_PATH_BYTES && offsetof(TreePathRec, action) == 8 &&
              offsetof(TreePathRec, node) == 24, "path record");

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

// The K descents of one game (the wave's), the body of tree_select_batch_kernel and of the Gumbel select
// (qttt_tree_gumbel_kernels.h): root_of(j) = the root rule of descent j, TreePuctRoot for the plain round.  row0 = the
// game's first row of paths and leaves: g * leaves in a round of all games, w * leaves for wave w of a subset round
// (qttt_tree_subset_kernels.h).
template <typename RootOf>
__device__ __forceinline__ void tree_select_batch_game(const TreeView &v, int64_t g, int64_t row0, u32 lane, const uint8_t *lut,
                                                       u64 seed, u32 rollout_idx0, u32 leaves, u64 board_offset, double c_puct,
                                                       double vloss, TreePathRec *paths, u64 *leafP, u64 *leafQ,
                                                       RootOf &&root_of) {
    TreeGame *gh = &v.games[g];
    const int32_t root = gh->root;
    int32_t used = gh->used;
    const u32 id = fold_id(board_offset + (u64)g);
    u32 overflow = 0u;
    for (u32 j = 0; j < leaves; ++j) {
        tree_wave_sync();                                        // what the earlier descents stored
        const u32 bits = lowbias32(id ^ (u32)launch_key(seed, QTTT_TREE_SELECT_BASE + rollout_idx0 + j));
        const TreeDescent d = tree_descend(v, g, root, bits, used, lut, lane, c_puct,
                                           [vloss](double W, u32 N, double prior, u32 Ntot, double c) {
                                               return tree_score_in_flight(W, N, prior, tree_sqrt(tree_effective(Ntot)), c, vloss);
                                           }, root_of(j));
        const u32 over = d.overflow ? TG_OVERFLOW : 0u;
        overflow |= over;
        // one in-flight visit on every edge of the path: lane d owns edge d, and the edges lie in different nodes
        TreePathRec *rec = paths + (row0 + j);
        if ((int32_t)lane < d.depth) {
            TreeSlot *slot = &v.slots(g, d.edge_node)[d.edge_action];
            TreeNodeHdr *nh = v.hdr(g, d.edge_node);
            slot->N = slot->N + TREE_FLIGHT_ONE;
            nh->Ntot = nh->Ntot + TREE_FLIGHT_ONE;
            rec->node[lane] = d.edge_node;
            rec->action[lane] = (uint8_t)d.edge_action;
        }
        if (lane == 0u) {
            rec->leaf = d.leaf;
            rec->depth = (uint8_t)d.depth;
            rec->flags = (uint8_t)(over | tree_leaf_flags(d.h.flags));
            leafP[row0 + j] = d.h.P;
            leafQ[row0 + j] = d.h.Q;
        }
    }
    if (lane == 0u) {                                            // the recorded path as tree_compact_kernel leaves it
        gh->used = used;                                         // (select never writes a node's flags)
        gh->depth = 0;
        gh->leaf = root;
        gh->flags = (gh->flags & TG_OVERFLOW) | overflow | tree_leaf_flags(v.hdr(g, root)->flags);
    }
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
    tree_select_batch_game(tree_view(tree, games, capacity), g, g * (int64_t)leaves, lane, lut, seed, rollout_idx0, leaves,
                           board_offset, c_puct, vloss, paths, leafP, leafQ, [](u32) { return TreePuctRoot(); });
}

// record j + 1 is fetched while record j is backed up: the records are not written here, so their loads need no order
struct TreePathLane {
    int32_t leaf, node;
    u32 depth, action;
    float value;
};
template <typename ValueOf>
__device__ __forceinline__ TreePathLane tree_path_lane(const TreePathRec *paths, ValueOf &&value_of, int64_t row, u32 lane) {
    const TreePathRec *rec = paths + row;
    TreePathLane p;
    p.leaf = rec->leaf;
    p.depth = rec->depth;
    p.node = lane < (u32)QTTT_TREE_MAX_DEPTH ? rec->node[lane] : 0;
    p.action = lane < (u32)QTTT_TREE_MAX_DEPTH ? rec->action[lane] : 0u;
    p.value = value_of(row);
    return p;
}

// The backup of one game's K records (the wave's), rows row0 .. row0 + K - 1 of paths, of the values and of the priors: the
// body of tree_backup_batch_kernel, of the subset round's backup (qttt_tree_subset_kernels.h), where row0 is not g * K, and
// of the resident search (qttt_tree_resident_kernels.h), where the records and the network's rows are in LDS.
// value_of(row) = the network's value of a row, prob_of(row, a) = its prior of action a: TreeLeafRows for the two arrays of
// the C ABI.
// EXACT: qttt_tree_backup_batch_exact (include/qttt_tree_exact.h): a record of depth >= 1 that ends on a solved leaf is
// backed up with the node's stored value and the leaf gets no priors; EXACT = false is qttt_tree_backup_batch.
struct TreeLeafRows {                  // leaf_value f32[rows], leaf_probs f32[rows, 36]
    const float *leaf_value, *leaf_probs;
    __device__ __forceinline__ float operator()(int64_t row) const { return leaf_value[row]; }
    __device__ __forceinline__ float operator()(int64_t row, u32 a) const { return leaf_probs[row * 36 + a]; }
};
template <bool EXACT, typename ValueOf, typename ProbOf>
__device__ __forceinline__ void tree_backup_batch_game(const TreeView &v, int64_t g, int64_t row0, u32 lane, int64_t capacity,
                                                       u32 leaves, const TreePathRec *paths, ValueOf &&value_of,
                                                       ProbOf &&prob_of) {
#pragma clang fp contract(off)
    TreePathLane next = tree_path_lane(paths, value_of, row0, lane);
    for (u32 j = 0; j < leaves; ++j) {
        const TreePathLane p = next;
        if (j + 1u < leaves) next = tree_path_lane(paths, value_of, row0 + j + 1u, lane);
        // a record that does not lie in the pool is skipped (wave-uniform: every lane sees every lane's entry)
        const bool edge = lane < p.depth;
        const bool bad_edge = edge && (p.node < 0 || (int64_t)p.node >= capacity || p.action >= 36u);
        if (p.depth > (u32)QTTT_TREE_MAX_DEPTH || p.leaf < 0 || (int64_t)p.leaf >= capacity || __ballot(bad_edge) != 0ull) continue;
        const u32 lf = v.hdr(g, p.leaf)->flags;
        double val = (lf & TN_TERMINAL) ? tree_terminal_value(lf) : (double)p.value;
        bool solved = false;
        if constexpr (EXACT) {
            solved = p.depth >= 1u && (lf & (TN_SOLVED | TN_TERMINAL | TN_PRIORS)) == TN_SOLVED;
            if (solved) val = (double)((int32_t)((lf & TN_VALUE_MASK) >> TN_VALUE_SHIFT) - 16) / 16.0;
        }
        if (edge) {
            TreeSlot *slot = &v.slots(g, p.node)[p.action];
            TreeNodeHdr *nh = v.hdr(g, p.node);
            slot->W = slot->W + tree_edge_value((int32_t)p.depth, lane, val);
            slot->N = slot->N + 1u - TREE_FLIGHT_ONE;
            nh->Ntot = nh->Ntot + 1u - TREE_FLIGHT_ONE;
        }
        if (!solved) tree_leaf_priors(v, g, p.leaf, lf, lane, true, [&](u32 a) { return prob_of(row0 + j, a); });
        tree_wave_sync();                                        // the next record may pass the same edges and leaf
    }
}

template <bool EXACT>
__global__ __launch_bounds__(TREE_BLOCK) void tree_backup_batch_kernel(void *tree, int64_t games, int64_t capacity, u32 leaves,
                                                                       const TreePathRec *paths, const float *leaf_value,
                                                                       const float *leaf_probs) {
    const int64_t g = (int64_t)blockIdx.x * TREE_GAMES_PER_BLOCK + threadIdx.x / 64;
    const u32 lane = threadIdx.x & 63u;
    if (g >= games) return;
    const TreeLeafRows rows = {leaf_value, leaf_probs};
    tree_backup_batch_game<EXACT>(tree_view(tree, games, capacity), g, g * (int64_t)leaves, lane, capacity, leaves, paths,
                                  rows, rows);
}

}  // namespace

#endif  // QTTT_TREE_LEAVES_KERNELS_H
