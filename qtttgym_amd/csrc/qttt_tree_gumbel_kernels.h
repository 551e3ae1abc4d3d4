// qttt_tree_gumbel_kernels.h — the Gumbel root of the device search trees (include/qttt_tree_gumbel.h):
// tree_gumbel_begin_kernel draws the Gumbel noise and picks the actions to consider, tree_select_batch_gumbel_kernel is the
// leaf-parallel select with sequential halving at the root, tree_gumbel_root_kernel gives the move, the completed Q and
// the improved policy; gumbel_final is also what selfplay_record_kernel<RECORD_GUMBEL> records (qttt_selfplay_kernels.h).
//
// Mapping: the tree kernels' (qttt_tree_kernels.h).  ONE WAVEFRONT PER GAME, lane a = action a, four games per workgroup.
// A game's record is read as the lane's own column (gumbel, prior, logit, n0 of action a) and three wave-uniform words;
// every reduction is a six-step butterfly (selfplay_wave_sum for the doubles, so the order is the record's), the rank of
// begin is 36 broadcasts of s0.  The select is tree_select_batch_game, the body of qttt_tree_select_batch, with
// GumbelRootRule as the root rule of the one tree_descend: there is no second descent.  The rule reads the root's slots
// that tree_descend has loaded already and the record; it stores nothing.  begin and root write only their game's rows of
// their outputs: no atomics, no LDS of their own, nothing handed between lanes through memory.
#ifndef QTTT_TREE_GUMBEL_KERNELS_H
#define QTTT_TREE_GUMBEL_KERNELS_H
#include "qttt_tree_leaves_kernels.h"
#include "qttt_tree_explore_kernels.h"
#include "qttt_tree_gumbel.h"

namespace {

struct GumbelRec {                     // 880 B, include/qttt_tree_gumbel.h
    double gumbel[36], prior[36];
    float logits[36];
    u32 n0[36];
    u64 considered;
    float root_value;
    u32 m_eff;
};
static_assert(sizeof(GumbelRec) == QTTT_TREE_GUMBEL_BYTES && offsetof(GumbelRec, logits) == 576 &&
              offsetof(GumbelRec, n0) == 720 && offsetof(GumbelRec, considered) == 864, "gumbel record");

// what lane a holds of its game's record; m_eff and root_value are the whole wave's.  A record whose m_eff cannot be
// (it indexes the visit table) counts as one with nothing considered.
struct GumbelLane {
    double s0, prior, logit, root_value;
    u32 n0, m_eff;
    bool considered;
};
__device__ __forceinline__ GumbelLane gumbel_lane(const GumbelRec *r, u32 lane) {
#pragma clang fp contract(off)
    GumbelLane l;
    l.m_eff = r->m_eff <= 36u ? r->m_eff : 0u;
    l.root_value = (double)r->root_value;
    l.s0 = 0.0; l.prior = 0.0; l.logit = 0.0; l.n0 = 0u; l.considered = false;
    if (lane < 36u) {
        l.logit = (double)r->logits[lane];
        l.s0 = r->gumbel[lane] + l.logit;
        l.prior = r->prior[lane];
        l.n0 = r->n0[lane];
        l.considered = ((r->considered >> lane) & 1ull) != 0ull;
    }
    return l;
}

__device__ __forceinline__ u32 gumbel_wave_max(u32 x) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) { const u32 o = __shfl_xor(x, m); x = o > x ? o : x; }
    return x;
}
__device__ __forceinline__ u32 gumbel_wave_sum(u32 x) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) x += __shfl_xor(x, m);
    return x;
}
__device__ __forceinline__ double gumbel_wave_max(double x) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) { const double o = __shfl_xor(x, m); x = o > x ? o : x; }
    return x;
}

// completed Q and sigma of the header, for lane a's action of a root whose slot is s
struct GumbelQ {
    double qhat, sigma;
    u32 n;                             // the action's visits, 0 where it is not legal
};
__device__ __forceinline__ GumbelQ gumbel_completed(const TreeSlot &s, bool legal, const GumbelLane &l, double c_visit,
                                                    double c_scale) {
#pragma clang fp contract(off)
    GumbelQ o;
    o.n = legal ? (s.N & TREE_COUNT_MASK) : 0u;
    const u32 S = gumbel_wave_sum(o.n), n_max = gumbel_wave_max(o.n);
    const double q = o.n ? s.W / (double)o.n : 0.0;
    const double A = selfplay_wave_sum(o.n ? l.prior * q : 0.0);
    const double B = selfplay_wave_sum(o.n ? l.prior : 0.0);
    const double Sd = (double)S;
    const double v_mix = S ? (l.root_value + (Sd * A) / B) / (1.0 + Sd) : l.root_value;
    o.qhat = o.n ? q : v_mix;
    o.sigma = ((c_visit + (double)n_max) * c_scale) * o.qhat;
    return o;
}

// the root rule of descent j of a Gumbel round: sequential halving by the visit table's entry c
struct GumbelRootRule {
    static constexpr bool on = true;
    GumbelLane l;
    u32 c;
    double c_visit, c_scale;
    __device__ __forceinline__ int operator()(const TreeNodeHdr &h, const TreeSlot &s, u32 lane) const {
#pragma clang fp contract(off)
        if (l.m_eff == 0u) return -1;                            // wave-uniform
        const bool legal = lane < 36u && ((h.legal >> lane) & 1ull);
        const GumbelQ q = gumbel_completed(s, legal, l, c_visit, c_scale);
        const bool cons = legal && l.considered;
        const bool match = cons && (q.n - l.n0) + (s.N >> TREE_FLIGHT_SHIFT) == c;
        const bool pick = __ballot(match) ? match : cons;
        return __builtin_amdgcn_readfirstlane(wave_argmax(pick, l.s0 + q.sigma, lane));
    }
};

__global__ __launch_bounds__(TREE_BLOCK) void tree_root_states_kernel(const void *tree, int64_t games, int64_t capacity,
                                                                      u64 *outP, u64 *outQ) {
    const int64_t g = (int64_t)blockIdx.x * TREE_BLOCK + threadIdx.x;
    if (g >= games) return;
    const TreeView v = tree_view(const_cast<void *>(tree), games, capacity);
    const TreeNodeHdr *h = v.hdr(g, v.games[g].root);
    outP[g] = h->P;
    outQ[g] = h->Q;
}

__global__ __launch_bounds__(TREE_BLOCK) void tree_gumbel_begin_kernel(const void *tree, int64_t games, int64_t capacity,
                                                                       u64 seed, u32 move_idx, u64 board_offset,
                                                                       u32 max_considered, const float *root_value,
                                                                       const float *root_logits, GumbelRec *recs) {
#pragma clang fp contract(off)
    const int64_t g = (int64_t)blockIdx.x * TREE_GAMES_PER_BLOCK + threadIdx.x / 64;
    const u32 lane = threadIdx.x & 63u;
    if (g >= games) return;
    const TreeView v = tree_view(const_cast<void *>(tree), games, capacity);
    const TreeRootLane r = tree_root_lane(v, g, lane);
    const bool live = !(r.h.flags & TN_TERMINAL) && r.h.legal != 0ull;                  // wave-uniform
    const bool legal = live && r.legal;
    const float logit_f = lane < 36u ? root_logits[g * 36 + lane] : -__builtin_inff();
    const double logit = (double)logit_f;
    double gumbel = 0.0;
    if (legal) {
        const u64 h = explore_hash(seed, fold_id(board_offset + (u64)g), QTTT_TREE_GUMBEL_BASE + move_idx * 36u + lane);
        gumbel = -log(-log(explore_u53(h)));
    }
    const double s0 = gumbel + logit;
    const double mx = gumbel_wave_max(legal ? logit : -__builtin_inf());
    const double e = legal ? exp(logit - mx) : 0.0;
    const double Z = selfplay_wave_sum(e);
    const u32 legal_count = (u32)__builtin_popcountll(r.h.legal);
    const u32 m_eff = live ? (max_considered < legal_count ? max_considered : legal_count) : 0u;
    u32 rank = 0u;
    for (u32 b = 0; b < 36u; ++b) {                              // how many legal actions come before this lane's
        const double sb = __shfl(s0, (int)b);
        if (((r.h.legal >> b) & 1ull) && (sb > s0 || (sb == s0 && b < lane))) ++rank;
    }
    const u64 considered = __ballot(legal && rank < m_eff);
    GumbelRec *rec = recs + g;
    if (lane < 36u) {
        rec->gumbel[lane] = gumbel;
        rec->prior[lane] = legal ? e / Z : 0.0;
        rec->logits[lane] = logit_f;
        rec->n0[lane] = r.s.N & TREE_COUNT_MASK;
    }
    if (lane == 0u) {
        rec->considered = considered;
        rec->root_value = root_value[g];
        rec->m_eff = m_eff;
    }
}

__global__ __launch_bounds__(TREE_BLOCK) void tree_select_batch_gumbel_kernel(void *tree, int64_t games, int64_t capacity,
                                                                              u64 seed, u32 rollout_idx0, u32 leaves,
                                                                              u64 board_offset, double c_puct, double vloss,
                                                                              TreePathRec *paths, u64 *leafP, u64 *leafQ,
                                                                              const GumbelRec *recs, const int32_t *visit_table,
                                                                              u32 n_sims, u32 sim_idx0, double c_visit,
                                                                              double c_scale) {
    __shared__ __attribute__((aligned(16))) uint8_t lut[LINE_LUT_BYTES];
    fill_line_lut<TREE_BLOCK>(lut);                              // ends with the workgroup barrier
    const int64_t g = (int64_t)blockIdx.x * TREE_GAMES_PER_BLOCK + threadIdx.x / 64;
    const u32 lane = threadIdx.x & 63u;
    if (g >= games) return;
    const GumbelLane l = gumbel_lane(recs + g, lane);
    // row m_eff <= 36 of i32[37, n_sims], entries sim_idx0 + j < n_sims (the host's check)
    const int32_t *row = visit_table + (int64_t)l.m_eff * n_sims + sim_idx0;
    tree_select_batch_game(tree_view(tree, games, capacity), g, g * (int64_t)leaves, lane, lut, seed, rollout_idx0, leaves, board_offset, c_puct,
                           vloss, paths, leafP, leafQ,
                           [&](u32 j) { return GumbelRootRule{l, (u32)row[j], c_visit, c_scale}; });
}

// the move, the completed Q and the improved policy of a root after its search
struct GumbelFinal {
    int choose;                        // every lane: the move, -1 where nothing is considered
    double pi, qhat;                   // lane a: of action a, 0 where it is not legal
};
__device__ __forceinline__ GumbelFinal gumbel_final(const TreeRootLane &r, const GumbelLane &l, u32 lane, double c_visit,
                                                    double c_scale) {
#pragma clang fp contract(off)
    const GumbelQ q = gumbel_completed(r.s, r.legal, l, c_visit, c_scale);
    const bool cons = r.legal && l.considered;
    const u32 visits = q.n - l.n0;
    const u32 most = gumbel_wave_max(cons ? visits : 0u);
    GumbelFinal f;
    f.choose = wave_argmax(cons && visits == most, l.s0 + q.sigma, lane);
    const double x = l.logit + q.sigma;
    const double mx = gumbel_wave_max(r.legal ? x : -__builtin_inf());
    const double e = r.legal ? exp(x - mx) : 0.0;
    const double Z = selfplay_wave_sum(e);
    f.pi = r.legal ? e / Z : 0.0;
    f.qhat = r.legal ? q.qhat : 0.0;
    return f;
}

__global__ __launch_bounds__(TREE_BLOCK) void tree_gumbel_root_kernel(const void *tree, const GumbelRec *recs, int64_t games,
                                                                      int64_t capacity, double c_visit, double c_scale,
                                                                      uint8_t *choose, double *pi, double *q_completed) {
    const int64_t g = (int64_t)blockIdx.x * TREE_GAMES_PER_BLOCK + threadIdx.x / 64;
    const u32 lane = threadIdx.x & 63u;
    if (g >= games) return;
    const TreeView v = tree_view(const_cast<void *>(tree), games, capacity);
    const GumbelFinal f = gumbel_final(tree_root_lane(v, g, lane), gumbel_lane(recs + g, lane), lane, c_visit, c_scale);
    if (lane < 36u) {
        if (pi) pi[g * 36 + lane] = f.pi;
        if (q_completed) q_completed[g * 36 + lane] = f.qhat;
    }
    if (choose && lane == 0u) choose[g] = f.choose < 0 ? (uint8_t)255 : (uint8_t)f.choose;
}

}  // namespace

#endif  // QTTT_TREE_GUMBEL_KERNELS_H
