// qttt_search_core.h — rules of the reference's MCTS / AlphaZero that more than one kernel applies, once each: the
// counter draw, the pair-action decode, the expansion of a pair and its children's bookkeeping facts, the uniform
// playout with its stopping rule and its slot -> step-index arithmetic, the playout's reward and the leaf.turn sign.
// All of them are bit-exactness rules; the kernels of qttt_mcts_kernels.h, qttt_tree_kernels.h and
// qttt_policy_rollout_kernels.h and the sampler of qttt_aux_kernels.h call them, as do tools/rowbench.cpp and
// tools/xr_sims_per_lane.cpp.  Where a kernel spells one of them out instead, a comment at the site says why.
#ifndef QTTT_SEARCH_CORE_H
#define QTTT_SEARCH_CORE_H
#include "qttt_step_core.h"
#include "qttt_board_forms.h"

namespace {

// The two-word counter draw of (board id folded by fold_id, launch key) = qttt_hash: h1's top bit is
// the collapse bit, h2 picks the action.  step_random_fused_kernel and step_body (qttt_step_kernels.h) keep their own
// spelling of it: that file is fingerprinted by bench.py and does not change.
struct Draw {
    u32 h1, h2;
};
__host__ __device__ __forceinline__ Draw counter_draw(u32 id, u64 key) {
    Draw d;
    d.h1 = lowbias32(id ^ (u32)key);
    d.h2 = lowbias32(d.h1 ^ (u32)(key >> 32));
    return d;
}

// ind2move (mcts.py:339-343): lexicographic pairs (0,1),(0,2)..(7,8) as lo | hi<<4
struct PairLut {
    uint8_t b[36];
    constexpr PairLut() : b() {
        int a = 0;
        for (int i = 0; i < 9; ++i)
            for (int j = i + 1; j < 9; ++j) b[a++] = (uint8_t)(i | (j << 4));
    }
};
__constant__ PairLut g_pair_lut = PairLut();

// the step's action word lo | hi << 8 of pair index a.  GUARDED: a caller's action36, where an index past 35 becomes
// (0,0), a noop; unguarded for an index the kernel itself found legal.
template <bool GUARDED, typename Index>
__device__ __forceinline__ u32 pair_action(Index a) {
    const u32 pr = (!GUARDED || a < 36u) ? (u32)g_pair_lut.b[a] : 0u;
    return (pr & 0xFu) | ((pr >> 4) << 8);
}

// MCTS._step (mcts.py:233-267) of one (state, action): both values of the collapse bit computed directly instead of
// re-sampling make_move until the other branch appears.  Validity, components, append, qstructs and classical update
// are shared, only the path reversal and the line test run per child (step_core_both).  Child 1 is a valid state even
// when there is no collapse: it equals child 0.
struct Expansion {
    u32 kids;               // 0 = make_move raises, 1 = no collapse, 2 = collapse
    u64 P[2], Q;            // the children's plane-P words; plane Q is the same for both
    u32 xo[2];              // who holds a line in each child (step_line_xo)
};
__device__ __forceinline__ Expansion expand_pair(u64 P, u64 Q, u32 act, const uint8_t *lut) {
    Expansion e;
    u32 Q0 = (u32)Q, Q1 = (u32)(Q >> 32), P0a, P1a, P0b, P1b;
    e.kids = step_core_both((u32)P, (u32)(P >> 32), Q0, Q1, act, lut, P0a, P1a, P0b, P1b, e.xo[0], e.xo[1]);   // mcts.py:245
    e.P[0] = (u64)P0a | ((u64)P1a << 32);
    e.P[1] = (u64)P0b | ((u64)P1b << 32);
    e.Q = (u64)Q0 | ((u64)Q1 << 32);
    return e;
}
// (a child's winner / terminal from the line test the step just made: update_winner_from_step(e.P[k], e.xo[k], ...),
// qttt_board_forms.h)
// the classical mask GameState.actions (mcts.py:20-27) sees in plane word P: the implicit autofill (eight classical
// squares) counted as the ninth
__device__ __forceinline__ u32 classical_with_autofill(u64 P) {
    const u32 cl = (u32)(P >> (32u + P1_CL_SHIFT)) & 0x1FFu;
    return __builtin_popcount(cl) == 8 ? 0x1FFu : cl;
}

// MCTS._simulate (mcts.py:185-198) under the uniform priors of mcts.py:287-292: play uniform-legal
// random moves to the end with the board in registers.  Ply p uses the counter hash of
// (seed, board id, step_idx0 + p) exactly like qttt_sample_actions + qttt_step would.
// The launch keys of a playout's plies come from a table in LDS (splitmix64 of (seed, step index): 25 scalar instructions
// per ply when the step index is wave-uniform, and ~30 VECTOR instructions per ply when it differs per lane — the
// simulations of rollout_many / expand_rollout use step_idx0 + slot * QTTT_SIM_STRIDE + ply).  A table row = the nine keys
// of one slot; PLAYOUT_KEY_SLOTS rows fit one key per thread of a 256-thread workgroup.  More slots than that: the keys are
// computed in the loop (TABLE = false).
constexpr u32 PLAYOUT_PLIES = 9u, PLAYOUT_KEY_SLOTS = 28u;
template <int BLOCK>
__device__ __forceinline__ void fill_playout_keys_nosync(u64 *keytab, u64 seed, u32 step_idx0, u32 n_slots) {
    for (u32 k = threadIdx.x; k < n_slots * PLAYOUT_PLIES; k += BLOCK) {
        const u32 slot = k / PLAYOUT_PLIES, ply = k - slot * PLAYOUT_PLIES;
        keytab[k] = launch_key(seed, step_idx0 + slot * QTTT_SIM_STRIDE + ply);
    }
}
// is the board with plane word P1 still playing?  Not once it is terminal (the done bit, mcts.py:188) or has fewer than
// two empty squares (nothing legal)
__device__ __forceinline__ bool playout_live(u32 P1) {
    const u32 empty = ~(P1 >> P1_CL_SHIFT) & 0x1FFu;
    return !(P1 >> 31) && (empty & (empty - 1u)) != 0u;
}
// one playout of the board in (P0, P1, Q0, Q1) to the end; returns the number of plies played.  TABLE: `keys` = the nine
// keys of this lane's slot (LDS); else they are launch_key(seed, step_idx0 + ply).
template <bool TABLE>
__device__ __forceinline__ u32 playout(u32 &P0, u32 &P1, u32 &Q0, u32 &Q1, u32 id, u64 seed, u32 step_idx0, const u64 *keys,
                                       const uint8_t *lut, const uint8_t *plut, const uint8_t *nth9) {
    u32 played = 0;
    u64 key_tab = TABLE ? keys[0] : 0ull;
    for (u32 p = 0; p < PLAYOUT_PLIES; ++p) {
        const u32 empty = ~(P1 >> P1_CL_SHIFT) & 0x1FFu;
        // !playout_live(P1), spelled out: through the helper the two tests fold into one branch and every playout kernel's
        // instruction stream changes
        if ((P1 >> 31) || (empty & (empty - 1u)) == 0u) break;
        const u64 key = TABLE ? key_tab : launch_key(seed, step_idx0 + p);
        if (TABLE) key_tab = keys[p + 1u < PLAYOUT_PLIES ? p + 1u : p];      // the next ply's, requested a ply ahead
        const Draw d = counter_draw(id, key);
        const u32 act = policy_action_nth9(plut, nth9, empty, d.h2);   // the k-th legal pair, squares a < b
        step_core<false, true>(P0, P1, Q0, Q1, act, d.h1 >> 31, lut);   // legal and sorted
        played += 1u;
    }
    return played;
}
// the playout of simulation slot `slot` of a launch whose slots use the step indices step_idx0 + slot * QTTT_SIM_STRIDE:
// from the key table (filled for step_idx0 by fill_playout_keys_nosync) if the launch's slots fit it (`table`,
// wave-uniform), else with the keys computed in the loop
__device__ __forceinline__ u32 playout_slot(u32 &P0, u32 &P1, u32 &Q0, u32 &Q1, u32 id, u64 seed, u32 step_idx0, u32 slot,
                                            bool table, const u64 *keytab, const uint8_t *lut, const uint8_t *plut,
                                            const uint8_t *nth9) {
    return table ? playout<true>(P0, P1, Q0, Q1, id, seed, 0u, keytab + slot * PLAYOUT_PLIES, lut, plut, nth9)
                 : playout<false>(P0, P1, Q0, Q1, id, seed, step_idx0 + slot * QTTT_SIM_STRIDE, nullptr, lut, plut, nth9);
}
// MCTS._reward (mcts.py:200-209) / AlphaZero._reward (alphazero.py:207-215) from update_winner's winner (1 True,
// 0 False, -1 None), and of the board with plane word P that a playout ended on
__device__ __forceinline__ int reward_of_winner(int w) { return w < 0 ? 0 : (w ? 1 : -1); }
__device__ __forceinline__ int playout_reward(u64 P, const uint8_t *lut) {
    int w, t;
    lite_update_winner(lite_unpack(P), lut, w, t);
    return reward_of_winner(w);
}
// `r if leaf.turn else -r` (mcts.py:174) for the leaf with plane word P1: leaf.turn is True after an even number of
// real moves (reset's len(moves) % 2 == 0 flipped once per _step, mcts.py:140,243)
__device__ __forceinline__ int leaf_turn_signed(int r, u32 leaf_P1) {
    return (((leaf_P1 >> P1_N_SHIFT) & 0xFu) & 1u) ? -r : r;
}

}  // namespace

#endif  // QTTT_SEARCH_CORE_H
