// qttt_kernels.hip — gfx950 (MI355X / CDNA4) kernels + the C ABI of include/qttt.h.
//
// Mapping: ONE LANE PER BOARD (64 boards per wavefront, BPL consecutive boards per lane),
// everything in VGPRs, structure-of-arrays state so that every load/store of a wave is one
// contiguous 16-byte-per-lane segment.  No MFMA; LDS holds one lookup table (and, in the kernels
// that return the observation, the output tiles).  DESIGN.md §2 explains why the wave-per-board
// mapping was rejected after measurement and why the kernel is written for minimum VALU
// *instruction count* (measured issue cost ~4 cycles per wave-instruction for this instruction mix,
// tools/valu_rates.cpp).
//
// Formulation — deliberately NOT the reference's algorithm:
//   * the un-collapsed moves of a board form a forest on the 9 squares (a move that closes a
//     cycle collapses its whole component at once, board.py:42-56).  The forest is kept ROOTED:
//     nibble sq[v] of a non-classical square v is the round of the move joining v to its parent
//     (root / isolated = none).  For a classical square, sq[v] is the round that landed there
//     (= Board.board[v]).
//   * QEvalClassic.eval (qeval.py:5-51: leaf-peel + forced walk round the cycle) is equivalent
//     to: re-root the tree at the square t the closing move lands on (bit picks lo/hi), then
//     every other square of the component receives its parent edge.  So a collapse is one path
//     reversal + `classical |= component`; no per-edge work.
//   * Every move ever played is therefore HELD by exactly one square c (sq[c] = its round): the
//     child end of an un-collapsed move, the landing square of a collapsed one.  The move itself
//     is then (c, c ^ x) with x = lo ^ hi, so the state stores only the 4-bit x of each move — the
//     re-rooting walk needs nothing else ("other end of edge e" = v ^ x_e) and the cold kernels
//     rebuild Board.moves from the holders.
//   * Board.qstructs (board.py:6) is cached as 4 slots x 9-bit square masks, in the reference's
//     list order, so "same component?" is two shifts and an AND.
//
// Packed state, 16 B/board = 39 algorithmic bytes per step, planes
// P[s] u64 | Q[s] u64 (s = n rounded up to 64).  The all-zero state is the empty board.
//   P bits [2,38)  nine nibbles, square v at bits [4v+2, 4v+6), COMPLEMENT-coded: 0 = root /
//                  isolated / empty, round e is stored as 15-e.  The 2-bit offset makes
//                  `(P >> 4v) & 0x3C` the code times four, the unit every shift amount below wants.
//   P1 = P >> 32:  [0,6) nibbles | [6,8) 0 | [8,12) n = moves PLAYED | [12,16) comps bits 32..35 |
//                  [16,20) x of the last move | [20,22) 0 | [22,31) classical mask | 31 done
//   Q0:            x = lo^hi of the moves of rounds 0..7: round e in the nibble at bit
//                  (4(7-e)+2) mod 32, so that rotating Q0 right by four times the CODE of e
//                  (4(15-e) = 4(7-e) mod 32) lands 4x on bits 2..5.  The move of round 8 can only
//                  be the last one of a game: its x is the `last x` field of P1 (it is also XORed
//                  onto round 0's nibble, where it is harmless: the game is over; the cold
//                  kernels undo it).
//   Q1:            comps bits 0..31 (comps = 4 x 9-bit masks, slot k at bit 9k, list order, compact)
//   The autofill of board.py:22-25 is IMPLICIT: a board with exactly 8 classical squares stands
//   for the reference state in which the 9th square holds round 8 and moves ends with (idx,idx,8)
//   (the autofill round is always 8); the cold kernels materialise it.
//
// Files: qttt_state.h (layout, loads/stores, shared tables) -> qttt_step_core.h (the step) ->
// qttt_observation.h -> qttt_step_kernels.h; qttt_board_forms.h (unpacked views, winner, legal mask,
// tuple hash) -> qttt_search_core.h (the search rules several kernels share: counter draw, pair-action decode, expansion
// of a pair, the uniform playout) -> qttt_aux_kernels.h (the cold kernels, the reset fills), qttt_mcts_kernels.h,
// qttt_nn_kernels.h (the policy/value network) -> qttt_policy_rollout_kernels.h (network-guided playouts);
// qttt_tree_kernels.h (the batched search trees) -> qttt_selfplay_kernels.h (the self-play record) ->
// qttt_symmetry_kernels.h (the board's symmetries: images of states, the augmented self-play batch);
// qttt_nn_symmetric_kernels.h (the network averaged over a position's symmetries, on qttt_nn_kernels.h's trunk and head);
// qttt_tree_value_kernels.h (the value rollout: network evaluation of the leaves and backup in one launch);
// qttt_tree_leaves_kernels.h (leaf-parallel rounds: K descents per game under virtual loss, and their backup);
// qttt_tree_explore_kernels.h (root exploration: Dirichlet noise on the roots' priors, the sampled move);
// qttt_tree_gumbel_kernels.h (the Gumbel root: considered actions, sequential halving, the improved policy);
// qttt_tree_forced_kernels.h (forced playouts at the root and policy target pruning: the root rule, the pruned record's counts)
// with qttt_tree_forced_host.h (free of HIP: the root entry's argument check and one action's arithmetic);
// qttt_replay_kernels.h (the replay ring: the append's scan and move, the sampled minibatch, and reanalysis: the gathered
// window and the guarded update) with qttt_replay_host.h (host only and free of HIP: the ring's layout, the scan plan, the
// window and holder arithmetic, the argument checks);
// qttt_train_kernels.h (the training step: loss, gradients and AMSGrad on the packed f32 blob, on qttt_nn_kernels.h's layers)
// with qttt_train_host.h (host only and free of HIP: the workspace layout and the launch plan);
// qttt_replay_priority_kernels.h (prioritised replay: the priority table's sums, the guarded write-back, the proportional draw
// on the sample kernel's row functions) with qttt_replay_priority_host.h (host only and free of HIP: layout, guard, quantiser);
// qttt_selfplay_stream_kernels.h (continuous self-play: the harvest of finished games and their restart in place);
// qttt_solve_kernels.h (the exact endgame solver: the full expectimax tree of a late position, a workgroup per board; and what
// the kernels that call its recursion on many small boards share: table fill, root classification, the workgroup's list of
// boards and its item loop); qttt_tree_exact_kernels.h (exact leaves in the search trees: a lane per path record, on that list);
// qttt_selfplay_exact_kernels.h (exact targets for the late rows of a self-play batch: a lane per staging row, on that list,
// every action's value kept for the policy); qttt_tree_prove_kernels.h (proven interior nodes: a round's
// records walked upwards, a wave per game, integers only, and the roots' exact q);
// qttt_selfplay_value_kernels.h (search-value targets: the roots' searched value, a wave per game, and the value targets made
// of it, a lane per game) with qttt_selfplay_value_host.h (free of HIP: the argument checks and one game's row arithmetic);
// qttt_tree_subset_kernels.h (rounds and root noise for a listed subset of the games, a wave per listed game, on the full
// launches' own device functions) with qttt_tree_subset_host.h (free of HIP: the argument checks); qttt_selfplay_cap_kernels.h
// (the record and harvest of playout cap randomisation: the stream record's and the harvest's bodies);
// qttt_tree_resident_kernels.h (the resident search: every round of a move in one launch, a workgroup per tile of games, on the
// select's, the network's and the backup's own device functions) with qttt_tree_resident_host.h (free of HIP: the tile, the
// round plan, the argument check).  Host only: qttt_launch.h (launch shape, kernel selection,
// the one launch form), qttt_checks.h (free of HIP: what every argument check is made of), qttt_selfplay_record_host.h (free of
// HIP: the one check of the self-play records and the one of the leaf-parallel selects), qttt_mailbox.h (the host half of the
// single-record mailbox); this file: the step's launch logic + the C ABI.
#include <atomic>
#include <chrono>
#include <cmath>
#include "qttt_step_kernels.h"
#include "qttt_aux_kernels.h"
#include "qttt_mcts_kernels.h"
#include "qttt_nn_kernels.h"
#include "qttt_policy_rollout_kernels.h"
#include "qttt_tree_kernels.h"
#include "qttt_tree_explore_kernels.h"
#include "qttt_selfplay_kernels.h"
#include "qttt_symmetry_kernels.h"
#include "qttt_nn_symmetric_kernels.h"
#include "qttt_tree_value_kernels.h"
#include "qttt_tree_leaves_kernels.h"
#include "qttt_tree_gumbel_kernels.h"
#include "qttt_tree_forced_kernels.h"
#include "qttt_replay_kernels.h"
#include "qttt_train_kernels.h"
#include "qttt_replay_priority_kernels.h"
#include "qttt_selfplay_stream_kernels.h"
#include "qttt_solve_kernels.h"
#include "qttt_tree_exact_kernels.h"
#include "qttt_selfplay_exact_kernels.h"
#include "qttt_tree_prove_kernels.h"
#include "qttt_selfplay_value_kernels.h"
#include "qttt_tree_subset_kernels.h"
#include "qttt_selfplay_cap_kernels.h"
#include "qttt_tree_resident_kernels.h"
#include "qttt_launch.h"
#include "qttt_mailbox.h"

namespace {

// One step of the record's boards: qttt_env_step's modes STEP, STEP_OBSERVE (obs) and STEP_RANDOM (sample: the policy
// draws the actions, and writes them to `actions` when that is not null).
// quiet (internal, plain STEP only: qttt_step_many's steps whose outputs the next step overwrites): the same checks and
// the same launches, but of step_quiet_kernel, which stores the planes and neither reward nor terminated.
int launch_step(const qttt_env &e, uint8_t *actions, const uint8_t *bits, uint32_t step_idx, void *stream, bool sample,
                const ObsOut *obs, bool quiet = false) {
    const int64_t n = e.n, board_offset = e.board_offset;
    if (n < 0 || board_offset < 0) return QTTT_ERR_SIZE;
    if (n == 0) return 0;
    if (any_null(e.state, e.reward, e.terminated) || (!sample && !actions)) return QTTT_ERR_NULL;
    if (misaligned(actions, 2)) return QTTT_ERR_ACTION;    // actions are accessed as u16 pairs
    retire_mailbox_for(n);
    const Planes p = planes(e.state, n);
    const uint32_t *step_ctr = e.step_counter;
    // with a device-side step counter the kernel makes the key itself: it gets the offset and the id fold
    const u64 key = step_ctr ? ((u64)step_idx << 32) : launch_key(e.seed, step_idx);
    const u32 key_lo = (u32)key, key_hi = (u32)(key >> 32);
    uint16_t *a16 = reinterpret_cast<uint16_t *>(actions);
    u32 *rb = reinterpret_cast<u32 *>(e.reward);
    int bpl_max, blk_sel;
    resolve_shape(n, e.flags, obs != nullptr, bpl_max, blk_sel);
    // widest boards-per-lane the caller's pointers are aligned for (the planes always are)
    auto aligned = [&](int k) {
        return !misaligned(actions, 2u * k) && !misaligned(e.reward, 4u * k) && !misaligned(e.terminated, k) && !misaligned(bits, k);
    };
    while (bpl_max > 1 && !aligned(bpl_max)) bpl_max >>= 1;
    const ObsOut oo = obs ? *obs : ObsOut{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    // Device-side step counter (graph capture: small, launch-bound batches): one launch shape — one board per lane,
    // 256-thread workgroups — and the kernels that make the launch key themselves.  Explicit bits need no key: the
    // ordinary kernels take them.
    const bool devstep = step_ctr && !bits;
    const StepKeySource<true> sk = {step_ctr, (u64)e.seed};
    const bool ob = obs != nullptr, sm = sample && !ob, hb = bits && !sm;
    const bool qt = quiet && !sm && !ob && !devstep;
    // `groups` lane-groups of bpl boards from board i0, in blk-thread workgroups (four boards per lane come with
    // QTTT_BLOCK threads: resolve_shape)
    auto launch_groups = [&](int bpl, int blk, int64_t i0, int64_t groups, u32 key_fold, u32 id_base) {
        return with_bools([&](auto QT, auto DEV, auto HB, auto AR, auto SM, auto OB) {
            return with_int<4, 2, 1>(bpl, [&](auto BPL) {
                return with_int<QTTT_BLOCK, 1024, 256>(blk, [&](auto BLK) {
                    // the instances that exist: the policy draws its own bits and writes no observation, the
                    // observation tiles take at most two boards per lane, four boards per lane come with QTTT_BLOCK
                    // threads, the device-side counter has its one shape, and the quiet step is the plain step only
                    if constexpr (!(SM && (HB || OB)) && !(OB && BPL == 4) && (BPL != 4 || BLK == QTTT_BLOCK) &&
                                  (!DEV || (BLK == 256 && BPL == 1 && !HB)) && !(QT && (DEV || SM || OB))) {
                        const int64_t grid = ceil_div(groups, BLK);
                        const u32 last_groups = (u32)(groups - (grid - 1) * BLK);
                        if constexpr (QT) {
                            return launch(step_quiet_kernel<BLK, BPL, HB, AR>, grid, BLK, stream, p.P, p.Q, a16, bits, key_fold,
                                          id_base, i0, last_groups);
                        } else {
                            const auto key_source = [&] { if constexpr (DEV) return sk; else return StepKeySource<false>{}; };
                            return launch(step_kernel<BLK, BPL, HB, AR, SM, OB, DEV>, grid, BLK, stream, p.P, p.Q, a16, bits,
                                          key_fold, key_hi, id_base, rb, e.terminated, oo, i0, last_groups, key_source());
                        }
                    } else {
                        return 0;
                    }
                });
            });
        }, qt, devstep, hb, (e.flags & QTTT_FLAG_AUTO_RESET) != 0, sm, ob);
    };
    // The hash folds the global board id as lo32 ^ hi32*C (fold_id).  hi32 is uniform over a
    // range of boards unless the range crosses a multiple of 2^32; the batch is cut there (at most
    // once), so the kernel only ever adds a lane index to a 32-bit base.  Stops at the first launch that fails.
    for (int64_t seg_begin = 0, seg_n; seg_begin < n; seg_begin += seg_n) {
        const u64 first = (u64)board_offset + (u64)seg_begin;
        const u64 to_boundary = (((first >> 32) + 1u) << 32) - first;
        seg_n = (int64_t)((u64)(n - seg_begin) < to_boundary ? (u64)(n - seg_begin) : to_boundary);
        const u32 key_fold = key_lo ^ ((u32)(first >> 32) * 0x9E3779B9u);
        const u32 id_base = (u32)first;
        int bpl = devstep ? 1 : bpl_max;
        while (bpl > 1 && (seg_begin % bpl) != 0) bpl >>= 1;     // vector accesses need an aligned start
        const int blk = devstep ? 256 : blk_sel;
        const int64_t n_groups = seg_n / bpl, n_main = n_groups * bpl;
        if (n_groups > 0)
            if (const int rc = launch_groups(bpl, blk, seg_begin, n_groups, key_fold, id_base)) return rc;
        if (n_main < seg_n)                                      // ragged tail, one board per lane
            if (const int rc = launch_groups(1, blk, seg_begin + n_main, seg_n - n_main, key_fold, id_base + (u32)n_main)) return rc;
    }
    return 0;
}

int launch_sample(const qttt_env &e, uint8_t *actions, uint32_t step_idx, void *stream) {
    const int64_t n = e.n;
    if (n < 0 || e.board_offset < 0) return QTTT_ERR_SIZE;
    if (n == 0) return 0;
    if (any_null(e.state, actions)) return QTTT_ERR_NULL;
    if (misaligned(actions, 2)) return QTTT_ERR_ACTION;    // written as u16 pairs
    const Planes p = planes(e.state, n);
    const u64 key = e.step_counter ? ((u64)step_idx << 32) : launch_key(e.seed, step_idx);
    return launch(sample_actions_kernel, ceil_div((n + 1) / 2, QTTT_BLOCK), QTTT_BLOCK, stream, p.P, (u32)key,
                  (u32)(key >> 32), (u64)e.board_offset, (u32)((e.flags & QTTT_FLAG_AUTO_RESET) != 0),
                  reinterpret_cast<uint16_t *>(actions), n, e.step_counter, (u64)e.seed);
}

int launch_board_op(const void *records_in, void *records_out, int64_t n, void *stream, u32 stamp) {
    if (n < 0) return QTTT_ERR_SIZE;
    if (n == 0) return 0;
    if (any_null(records_in, records_out)) return QTTT_ERR_NULL;
    return launch(board_op_kernel, ceil_div(n, QTTT_COLD_BLOCK), QTTT_COLD_BLOCK, stream, (const uint8_t *)records_in,
                  (uint8_t *)records_out, n, stamp);
}

int stream_sync(void *stream) {
    const hipError_t e = hipStreamSynchronize((hipStream_t)stream);
    return e == hipSuccess ? 0 : (int)e;
}

// the per-child rows [n,2] of qttt_expand / qttt_expand_rollout are written as one vector per pair
bool expand_rows_misaligned(const int8_t *winner, const uint8_t *terminal, const uint64_t *legal, const int64_t *key,
                            const uint64_t *state_key) {
    return misaligned(winner, 2) || misaligned(terminal, 2) || misaligned(legal, 16) || misaligned(key, 16) ||
           misaligned(state_key, 16);
}

// THE SelfPlayOut of nine output pointers, typed by the C ABI entry that took them (the augment's inputs are const there)
SelfPlayOut selfplay_out(const void *states, const void *pi, const void *mask, const void *done, const void *v,
                         const void *action36, const void *length, const void *winner, const void *actions) {
    return {(u64 *)states, (double *)pi, (uint8_t *)mask, (uint8_t *)done, (float *)v, (uint8_t *)action36, (uint8_t *)length,
            (int8_t *)winner, (uint8_t *)actions};
}

// THE launch of the self-play record, after record_check (qttt_selfplay_record_host.h) let the arguments through; the stream
// kernels take the draw index (0 where the mode draws nothing) where the lockstep ones take the ply
template <int MODE, bool STREAM>
int record_launch(const RecordArgs &a, int64_t games, int64_t capacity, int ply_or_draw, uint32_t n_rollouts, double alpha,
                  double v_first, double v_second, const SelfPlaySampling<MODE> &sampling, void *stream) {
    const SelfPlayOut o = selfplay_out(a.states, a.pi, a.mask, a.done, a.v, a.action36, a.length, a.winner, a.actions);
    return launch(selfplay_record_kernel<MODE, STREAM>, ceil_div(games, TREE_GAMES_PER_BLOCK), TREE_BLOCK, stream, a.tree, games,
                  capacity, ply_or_draw, n_rollouts, alpha, (float)v_first, (float)v_second, o, sampling);
}

// THE check of the two harvests (include/qttt_selfplay_stream.h, qttt_selfplay_cap.h); `work`: there is something to launch
int harvest_check(const void *tree, int64_t games, int64_t capacity, double v_first, double v_second, const SelfPlayOut &o,
                  const SelfPlayHarvest &hv, bool &work) {
    work = false;
    if (tree_size_bad(games, capacity) || !is_finite(v_first) || !is_finite(v_second)) return QTTT_ERR_SIZE;
    if (games == 0) return 0;
    if (any_null(tree, o.states, o.pi, o.mask, o.done, o.v, o.action36, o.length, o.winner, o.actions) ||
        any_null(hv.harvest_len, hv.finished, hv.games_done, hv.tally))
        return QTTT_ERR_NULL;
    if (misaligned(tree, 16) || misaligned(o.states, 16) || misaligned(o.pi, 8) || misaligned(hv.games_done, 8) ||
        misaligned(hv.tally, 8) || misaligned(o.v, 4))
        return QTTT_ERR_ACTION;
    work = true;
    return 0;
}

// THE backup of a leaf-parallel round: qttt_tree_backup_batch, and with EXACT the one that honours solved nodes
template <bool EXACT>
int backup_batch(void *tree, int64_t games, int64_t capacity, int leaves, const void *paths, const float *leaf_value,
                 const float *leaf_probs, void *stream) {
    if (tree_size_bad(games, capacity) || tree_leaves_bad(games, leaves)) return QTTT_ERR_SIZE;
    if (games == 0) return 0;
    if (any_null(tree, paths, leaf_value, leaf_probs)) return QTTT_ERR_NULL;
    if (misaligned(tree, 16) || misaligned(paths, 16) || misaligned(leaf_value, 4) || misaligned(leaf_probs, 4))
        return QTTT_ERR_ACTION;
    return launch(tree_backup_batch_kernel<EXACT>, ceil_div(games, TREE_GAMES_PER_BLOCK), TREE_BLOCK, stream, tree, games, capacity,
                  (u32)leaves, static_cast<const TreePathRec *>(paths), leaf_value, leaf_probs);
}

}  // namespace

// ====================================================================== C ABI
extern "C" {

int qttt_abi_version(void) { return QTTT_ABI_VERSION; }

#ifdef QTTT_DEBUG_STAMPS
int qttt_debug_set_stamps(void *buf) {
    u64 *p = (u64 *)buf;
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_debug_stamps), &p, sizeof(p));
}
#endif

int64_t qttt_state_bytes(int64_t n) { return n < 0 ? (int64_t)QTTT_ERR_SIZE : plane_stride(n) * QTTT_STATE_BYTES; }

// reset_kernel rather than hipMemsetAsync: measured with bench.py, alternating on one box (profiles/r05/bench_reset_ab.txt)
int qttt_reset(void *state, int64_t n, void *stream) {
    if (n < 0) return QTTT_ERR_SIZE;
    if (n == 0) return 0;
    if (!state) return QTTT_ERR_NULL;
    const int64_t n16 = plane_stride(n) * QTTT_STATE_BYTES / 16;
    return launch(reset_kernel, ceil_div(n16, 256), 256, stream, static_cast<u32x4 *>(state), n16);
}

// state and the empty board's observation: seven byte fills in one launch (reset_observe_kernel)
int qttt_reset_observe(void *state, int8_t *classical, uint8_t *q_p1, uint8_t *q_p1_len, uint8_t *q_p2,
                       uint8_t *q_p2_len, uint8_t *turn, int64_t n, void *stream) {
    if (n < 0) return QTTT_ERR_SIZE;
    if (n == 0) return 0;
    if (!state || obs_missing({classical, q_p1, q_p1_len, q_p2, q_p2_len, turn})) return QTTT_ERR_NULL;
    FillSegs f = {{static_cast<uint8_t *>(state), reinterpret_cast<uint8_t *>(classical), q_p1, q_p1_len, q_p2, q_p2_len, turn},
                  {plane_stride(n) * QTTT_STATE_BYTES, 9 * n, 10 * n, n, 8 * n, n, n},
                  {0},
                  {0u, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0xFFFFFFFFu, 0u, 0u}};
    for (int k = 0; k < 7; ++k) f.first[k + 1] = f.first[k] + ((f.bytes[k] - fill_head(f.p[k], f.bytes[k])) >> 4);
    const int64_t grid = ceil_div(f.first[7], 256);
    return launch(reset_observe_kernel, grid ? grid : 1, 256, stream, f);
}

int qttt_step(void *state, const uint8_t *actions, const uint8_t *bits, uint64_t seed,
              uint32_t step_idx, int64_t board_offset, uint32_t flags, float *reward,
              uint8_t *terminated, int64_t n, void *stream) {
    const qttt_env e = {state, n, board_offset, seed, flags, 0u, reward, terminated};
    return qttt_env_step(&e, const_cast<uint8_t *>(actions), bits, step_idx, QTTT_ENV_STEP, stream);
}

int qttt_step_observe(void *state, const uint8_t *actions, const uint8_t *bits, uint64_t seed,
                      uint32_t step_idx, int64_t board_offset, uint32_t flags, float *reward,
                      uint8_t *terminated, int8_t *classical, uint8_t *q_p1, uint8_t *q_p1_len,
                      uint8_t *q_p2, uint8_t *q_p2_len, uint8_t *turn, int64_t n, void *stream) {
    const qttt_env e = {state, n, board_offset, seed, flags, 0u, reward, terminated, classical, q_p1, q_p1_len, q_p2,
                        q_p2_len, turn};
    return qttt_env_step(&e, const_cast<uint8_t *>(actions), bits, step_idx, QTTT_ENV_STEP_OBSERVE, stream);
}

int qttt_step_many(void *state, const uint8_t *actions, const uint8_t *bits, uint64_t seed,
                   uint32_t step_idx0, int64_t board_offset, uint32_t flags, float *reward,
                   uint8_t *terminated, int64_t out_stride, int64_t n, int32_t n_steps,
                   void *stream) {
    if (n_steps < 0 || out_stride < 0) return QTTT_ERR_SIZE;
    const u64 first = (u64)(board_offset < 0 ? 0 : board_offset);
    const bool one_hi = n > 0 && (first >> 32) == ((first + (u64)n - 1u) >> 32);
    // the boards in registers: asked for (QTTT_FLAG_FUSED), or the route of the one-round rows (resident_route, qttt_launch.h)
    const bool fused = (flags & QTTT_FLAG_FUSED) != 0 || resident_route(n, flags, out_stride, n_steps);
    if (fused && n > 0 && n_steps > 0 && one_hi) {
        if (board_offset < 0) return QTTT_ERR_SIZE;
        if (any_null(state, actions, reward, terminated)) return QTTT_ERR_NULL;
        if (misaligned(actions, 2)) return QTTT_ERR_ACTION;
        retire_mailbox_for(n);
        const Planes p = planes(state, n);
        const u32 hi_fold = (u32)(first >> 32) * 0x9E3779B9u;
        const uint16_t *a16 = reinterpret_cast<const uint16_t *>(actions);
        u32 *rb = reinterpret_cast<u32 *>(reward);
        const bool has_bits = bits != nullptr, auto_reset = (flags & QTTT_FLAG_AUTO_RESET) != 0;
        if (out_stride != 0)
            return fused_runs<FUSED_MAX_PLIES, FusedKeys>(seed, step_idx0, n_steps, [&](int64_t done, int32_t plies, const FusedKeys &keys) {
                return with_bools([&](auto HB, auto AR) {
                    return launch(step_fused_kernel<HB, AR, FUSED_OUT_EVERY>, ceil_div(n, QTTT_BLOCK), QTTT_BLOCK, stream, p.P, p.Q,
                                  a16 + done * n, bits ? bits + done * n : nullptr, keys, hi_fold, (u32)first,
                                  rb + done * out_stride, terminated + done * out_stride, out_stride, n, plies);
                }, has_bits, auto_reset);
            });
        // With out_stride == 0 only the run's last launch stores outputs (its last ply's, once, after the loop); the earlier
        // launches are handed no output pointers.  RESIDENT_MAX_PLIES per launch: nothing but the keys argument bounds it.
        typedef ResidentKeys<RESIDENT_MAX_PLIES> Keys;
        return fused_runs<RESIDENT_MAX_PLIES, Keys>(seed, step_idx0, n_steps, [&](int64_t done, int32_t plies, const Keys &keys) {
            return with_bools([&](auto HB, auto AR, auto LAST) {
                constexpr int OUT = LAST ? FUSED_OUT_LAST : FUSED_OUT_NONE;
                return launch(step_fused_kernel<HB, AR, OUT, RESIDENT_MAX_PLIES, RESIDENT_BLOCK>, ceil_div(n, RESIDENT_BLOCK),
                              RESIDENT_BLOCK, stream, p.P, p.Q, a16 + done * n, bits ? bits + done * n : nullptr, keys, hi_fold,
                              (u32)first, LAST ? rb : nullptr, LAST ? terminated : nullptr, n, plies);
            }, has_bits, auto_reset, done + plies == n_steps);
        });
    }
    // With out_stride == 0 every step writes the same n outputs and only the last step's can ever be read: the earlier
    // steps run without them (step_quiet_kernel: 34 instead of 39 bytes per board), after the same argument checks.
    for (int32_t t = 0; t < n_steps; ++t) {
        const qttt_env e = {state, n, board_offset, seed, flags, 0u, reward + (int64_t)t * out_stride,
                            terminated + (int64_t)t * out_stride};
        int rc = launch_step(e, const_cast<uint8_t *>(actions + (int64_t)t * 2 * n), bits ? bits + (int64_t)t * n : nullptr,
                             step_idx0 + (uint32_t)t, stream, false, nullptr, out_stride == 0 && t < n_steps - 1);
        if (rc != 0) return rc;
    }
    return 0;
}

int qttt_step_random_many(void *state, uint64_t seed, uint32_t step_idx0, int64_t board_offset, uint32_t flags,
                          uint8_t *actions_out, float *reward, uint8_t *terminated, int64_t out_stride,
                          float *returns, int64_t n, int32_t n_steps, void *stream) {
    if (n < 0 || board_offset < 0 || n_steps < 0 || out_stride < 0) return QTTT_ERR_SIZE;
    if (n == 0 || n_steps == 0) return 0;
    if (!state || (reward == nullptr) != (terminated == nullptr)) return QTTT_ERR_NULL;
    if (misaligned(actions_out, 2) || misaligned(reward, 4) || misaligned(returns, 4)) return QTTT_ERR_ACTION;
    retire_mailbox_for(n);
    const Planes p = planes(state, n);
    uint16_t *a16 = reinterpret_cast<uint16_t *>(actions_out);
    u32 *rb = reinterpret_cast<u32 *>(reward);
    // 256-thread workgroups: the finest spread of a small batch over the 256 CUs (4 096 boards = 16 CUs
    // with 512 threads, 16 with 256 — but 262 144 boards = 1 024 workgroups, four per CU, instead of two)
    // The boards go through HBM between the launches of a longer run (32 bytes per board and 64 plies).  With
    // out_stride == 0 only the LAST ply's outputs are kept, so the earlier launches of such a run write none.
    // The instantiation without the per-ply "what is kept" tests, where it pays: one or two waves per SIMD are bound by a
    // wave's own in-order stream (65 536 boards 0.59 -> 0.56 us per ply, 4 096: 0.58 -> 0.55), from four waves up the
    // test-free loop is no faster and at 1 M boards 2 % slower (profiles/r05/fused_keep_instantiation_ab.txt, same box,
    // alternating)
    const bool keep_all = out_stride != 0 && a16 && rb && n < 262144;
    return fused_runs<FUSED_MAX_PLIES, FusedKeys>(seed, step_idx0, n_steps, [&](int64_t done, int32_t plies, const FusedKeys &keys) {
        const bool writes = out_stride != 0 || done + plies == n_steps;
        uint16_t *a_c = (a16 && writes) ? a16 + done * out_stride : nullptr;
        u32 *r_c = (rb && writes) ? rb + done * out_stride : nullptr;
        uint8_t *t_c = (terminated && writes) ? terminated + done * out_stride : nullptr;
        return with_bools([&](auto AR, auto RT, auto KP) {
            return launch(step_random_fused_kernel<256, AR, RT, KP>, ceil_div(n, 256), 256, stream, p.P, p.Q, keys,
                          (u64)board_offset, a_c, r_c, t_c, out_stride, n, plies, returns);
        }, (flags & QTTT_FLAG_AUTO_RESET) != 0, returns != nullptr, keep_all);
    });
}

int qttt_observe(const void *state, int8_t *classical, uint8_t *q_p1, uint8_t *q_p1_len,
                 uint8_t *q_p2, uint8_t *q_p2_len, uint8_t *turn, int64_t n, void *stream) {
    if (n < 0) return QTTT_ERR_SIZE;
    if (n == 0) return 0;
    if (!state) return QTTT_ERR_NULL;
    const ObsOut o = {classical, q_p1, q_p1_len, q_p2, q_p2_len, turn};
    if (const int rc = obs_check(o, n)) return rc;
    const Planes p = planes(const_cast<void *>(state), n);
    // 256-thread workgroups: best or tied at every batch size for this write-heavy kernel (tools/rowbench, us per
    // launch, 256 / 512 / 1024 threads: 65 536 boards 3.7 / 4.1 / 5.2, 1 M: 8.7 / 8.7 / 8.6)
    const int blk_default = tuning_word().load(std::memory_order_relaxed) >> 8;
    return with_int<1024, 256, QTTT_BLOCK>(blk_default ? blk_default : 256, [&](auto BLK) {
        return launch(observe_kernel<BLK>, ceil_div(n, 2 * BLK), BLK, stream, p.P, p.Q, o, n);
    });
}

int qttt_check_win(const void *state, int8_t *p1_round, int8_t *p2_round, int64_t n, void *stream) {
    if (n < 0) return QTTT_ERR_SIZE;
    if (n == 0) return 0;
    if (any_null(state, p1_round, p2_round)) return QTTT_ERR_NULL;
    const Planes p = planes(const_cast<void *>(state), n);
    return launch(check_win_kernel, ceil_div((n + 1) / 2, QTTT_COLD_BLOCK), QTTT_COLD_BLOCK, stream, p.P, p.Q, p1_round,
                  p2_round, n);
}

int qttt_export(const void *state, uint8_t *moves, uint8_t *n_moves, int8_t *board,
                uint16_t *qmask, uint8_t *n_q, int64_t n, void *stream) {
    if (n < 0) return QTTT_ERR_SIZE;
    if (n == 0) return 0;
    if (!state) return QTTT_ERR_NULL;
    if (!moves && !n_moves && !board && !qmask && !n_q) return 0;            // nothing asked for
    if (misaligned(qmask, 2)) return QTTT_ERR_ACTION;
    const Planes p = planes(const_cast<void *>(state), n);
    const ExpOut o = {moves, n_moves, board, qmask, n_q};
    // tools/rowbench (profiles/r03/rowbench_*.txt), us per launch, boards per lane x workgroup size:
    //   1 M boards: 1 x 256 / 512 / 1024 = 13.7 / 14.1 / 12.7, 2 x 256 / 512 / 1024 = 9.2 / 9.4 / 9.4 (one occupancy round)
    //   64 K boards: 1 x 256 = 3.3, 2 x 256 = 3.8 (latency-bound: more waves in flight win)
    return with_int<2, 1>(n >= 384 * 1024 ? 2 : 1, [&](auto BPL) {
        return launch(export_kernel<QTTT_COLD_BLOCK, BPL>, ceil_div(ceil_div(n, BPL), QTTT_COLD_BLOCK), QTTT_COLD_BLOCK, stream,
                      p.P, p.Q, o, n);
    });
}

int qttt_import(void *state, const uint8_t *moves, const uint8_t *n_moves, const int8_t *board,
                const uint16_t *qmask, const uint8_t *n_q, int64_t n, void *stream) {
    if (n < 0) return QTTT_ERR_SIZE;
    if (n == 0) return 0;
    if (any_null(state, moves, n_moves, board, qmask, n_q)) return QTTT_ERR_NULL;
    const Planes p = planes(state, n);
    const ExpOut in = {const_cast<uint8_t *>(moves), const_cast<uint8_t *>(n_moves), const_cast<int8_t *>(board),
                       const_cast<uint16_t *>(qmask), const_cast<uint8_t *>(n_q)};
    return launch(import_kernel<QTTT_COLD_BLOCK>, ceil_div(n, QTTT_COLD_BLOCK), QTTT_COLD_BLOCK, stream, p.P, p.Q, in, n);
}

int qttt_board_op(const void *records_in, void *records_out, int64_t n, void *stream) {
    return launch_board_op(records_in, records_out, n, stream, 0u);
}

int qttt_board_op_sync(const void *records_in, void *records_out, int64_t n, void *stream) {
    if (const int rc = qttt_board_op(records_in, records_out, n, stream)) return rc;
    return stream_sync(stream);
}

// Records in HOST-accessible pinned memory: the host clears the stamp byte of every out record, launches, and polls the
// stamps — the kernel writes a record's stamp after the record itself is visible system-wide.  tools/sync_latency, one
// record: launch + hipStreamSynchronize 14.7 - 16.0 us per call, launch + poll 9.7.  A poll that has not ended after
// ~2 ms (or a batch too large to poll) falls back to synchronising the stream, so the call always returns.  A single
// record goes through the mailbox first (qttt_mailbox.h).
int qttt_board_op_host(const void *records_in, void *records_out, int64_t n, void *stream) {
    if (n < 0) return QTTT_ERR_SIZE;
    if (n == 0) return 0;
    if (any_null(records_in, records_out)) return QTTT_ERR_NULL;
    if (n == 1 && board_mailbox().call(records_in, records_out) == 0) return 0;
    constexpr int64_t POLL_MAX_RECORDS = 256;
    volatile uint8_t *out = static_cast<volatile uint8_t *>(records_out);
    const bool poll = n <= POLL_MAX_RECORDS;
    if (poll)
        for (int64_t i = 0; i < n; ++i) out[i * QTTT_BOARD_RECORD_BYTES + QTTT_BOARD_RECORD_BYTES - 1] = 0;
    std::atomic_thread_fence(std::memory_order_release);
    if (const int rc = launch_board_op(records_in, records_out, n, stream, poll ? 1u : 0u)) return rc;
    if (poll) {
        const auto give_up = std::chrono::steady_clock::now() + std::chrono::milliseconds(2);
        bool done = false;
        for (unsigned spin = 1; !done; ++spin) {
            done = true;
            for (int64_t i = n - 1; i >= 0 && done; --i) done = out[i * QTTT_BOARD_RECORD_BYTES + QTTT_BOARD_RECORD_BYTES - 1] != 0;
            if (!done && (spin & 1023u) == 0u && std::chrono::steady_clock::now() > give_up) break;
        }
        std::atomic_thread_fence(std::memory_order_acquire);
        if (done) return 0;
    }
    return stream_sync(stream);
}

int qttt_board_mailbox_retire(int wait) {
    if (!g_mailbox_resident.load(std::memory_order_relaxed) && !wait) return 0;
    return board_mailbox().retire(wait != 0);
}

int qttt_sample_actions(const void *state, uint64_t seed, uint32_t step_idx, int64_t board_offset,
                        uint32_t flags, uint8_t *actions, int64_t n, void *stream) {
    const qttt_env e = {const_cast<void *>(state), n, board_offset, seed, flags};
    return qttt_env_step(&e, actions, nullptr, step_idx, QTTT_ENV_SAMPLE, stream);
}

// ---------------------------------------------------------------- the next rows
int qttt_node_info(const void *state, int8_t *winner, uint8_t *terminal, uint64_t *legal,
                   int64_t *key, uint64_t *state_key, int64_t n, void *stream) {
    if (n < 0) return QTTT_ERR_SIZE;
    if (n == 0) return 0;
    if (!state) return QTTT_ERR_NULL;
    if (!winner && !terminal && !legal && !key && !state_key) return 0;      // nothing asked for
    const Planes p = planes(const_cast<void *>(state), n);
    // workgroup size by batch (tools/rowbench, us per launch, 256 / 512 / 1024 threads: 1 M boards 11.7 / 11.2 / 10.5 —
    // the 12 KB of tables are filled once per workgroup; 64 K boards 4.6 / 4.7 / 5.8 — latency-bound).  Measured and not
    // adopted: a 1 000-entry table of the accumulator after the first three board elements (three multiply steps
    // less per board): 10.2 us with 1024 threads, but every smaller shape and expand lose as much to the 8 KB fill.
    return with_int<1024, 256>(n >= 384 * 1024 ? 1024 : 256, [&](auto BLK) {
        return with_bools([&](auto PK) {
            return launch(node_info_kernel<BLK, PK>, ceil_div((n + 1) / 2, BLK), BLK, stream, p.P, p.Q, winner, terminal,
                          (u64 *)legal, key, (u64 *)state_key, n);
        }, key != nullptr);
    });
}

uint64_t qttt_state_key(uint64_t plane_p_word, uint64_t plane_q_word) { return state_key(plane_p_word, (u32)plane_q_word); }

int qttt_expand(const void *state, const uint8_t *action36, void *child0, void *child1,
                uint8_t *n_children, int8_t *winner, uint8_t *terminal, uint64_t *legal,
                int64_t *key, uint64_t *state_key, int64_t n, void *stream) {
    if (n < 0) return QTTT_ERR_SIZE;
    if (n == 0) return 0;
    if (any_null(state, action36, child0, child1)) return QTTT_ERR_NULL;
    if (expand_rows_misaligned(winner, terminal, legal, key, state_key)) return QTTT_ERR_ACTION;
    const Planes p = planes(const_cast<void *>(state), n), c0 = planes(child0, n), c1 = planes(child1, n);
    const ExpandOut o = {n_children, winner, terminal, (u64 *)legal, key, (u64 *)state_key};
    // workgroup size by batch (tools/rowbench, us per launch, 256 / 512 / 1024 threads: 1 M pairs with native keys 18.3 /
    // 18.2 / 17.5, with the CPython keys 28.3 / 26.8 / 25.0; 64 K pairs 4.5 / 4.4 / 4.7 and 5.8 / 6.1 / 7.7)
    return with_int<1024, 256>(n >= 384 * 1024 ? 1024 : 256, [&](auto BLK) {
        return with_bools([&](auto PK) {
            return launch(expand_kernel<BLK, PK>, ceil_div(n, BLK), BLK, stream, p.P, p.Q, action36, c0.P, c0.Q, c1.P, c1.Q, o, n);
        }, key != nullptr);
    });
}

int qttt_rollout(const void *state, uint64_t seed, uint32_t step_idx0, int64_t board_offset,
                 int8_t *result, uint8_t *plies, void *final_state, int64_t n, void *stream) {
    if (n < 0 || board_offset < 0) return QTTT_ERR_SIZE;
    if (n == 0) return 0;
    if (any_null(state, result, plies)) return QTTT_ERR_NULL;
    const Planes p = planes(const_cast<void *>(state), n);
    const Planes f = final_state ? planes(final_state, n) : Planes{nullptr, nullptr};
    return launch(rollout_kernel, ceil_div(n, QTTT_BLOCK), QTTT_BLOCK, stream, p.P, p.Q, (u64)seed, step_idx0,
                  (u64)board_offset, result, plies, f.P, f.Q, n);
}

int qttt_rollout_many(const void *state, uint64_t seed, uint32_t step_idx0, int64_t board_offset,
                      int32_t n_sims, int8_t *result, uint8_t *plies, int64_t n, void *stream) {
    if (n < 0 || board_offset < 0 || n_sims < 0) return QTTT_ERR_SIZE;
    if (n == 0 || n_sims == 0) return 0;
    if (any_null(state, result)) return QTTT_ERR_NULL;
    const Planes p = planes(const_cast<void *>(state), n);
    const int64_t lanes = n * (int64_t)n_sims;
    return launch(rollout_many_kernel, ceil_div(lanes, QTTT_BLOCK), QTTT_BLOCK, stream, p.P, p.Q, (u64)seed, step_idx0,
                  (u64)board_offset, (u32)n_sims, result, plies, lanes);
}

int qttt_expand_rollout(const void *state, const uint8_t *action36, void *child0, void *child1,
                        uint8_t *n_children, int8_t *winner, uint8_t *terminal, uint64_t *legal,
                        int64_t *key, uint64_t *state_key, uint64_t seed, uint32_t step_idx0,
                        int64_t board_offset, int32_t n_sims, int32_t *value_sum, int8_t *result,
                        int64_t n, void *stream) {
    constexpr int BLK = 256;
    if (n < 0 || board_offset < 0 || n_sims < 1 || n_sims > QTTT_EXPAND_ROLLOUT_MAX_SIMS) return QTTT_ERR_SIZE;
    if (n == 0) return 0;
    if (any_null(state, action36, value_sum)) return QTTT_ERR_NULL;
    if (expand_rows_misaligned(winner, terminal, legal, key, state_key) || misaligned(value_sum, 4)) return QTTT_ERR_ACTION;
    const Planes p = planes(const_cast<void *>(state), n), none = {nullptr, nullptr};
    const Planes c0 = child0 ? planes(child0, n) : none, c1 = child1 ? planes(child1, n) : none;
    const ExpandOut o = {n_children, winner, terminal, (u64 *)legal, key, (u64 *)state_key};
    // Two mappings with the same results (tools/rowbench): a lane per (pair, simulation, child) for the latency-bound
    // case — few playouts in all — and the job-list kernel, whose workgroups expand P pairs once and deal the playouts of
    // the children that exist to their lanes, wherever the playouts are the work.  P: as many pairs as lanes, but at
    // least ~1 000 workgroups so that a small batch still covers the chip.
    const bool jobs = n * (int64_t)n_sims >= 262144;
    // P pairs per workgroup of the job-list kernel: a power of two (the workgroups' rows of every output then start on
    // whole cache lines), at most one pair per lane, and few enough that ~1 000 workgroups exist.  tools/rowbench, us per
    // launch, 10 playouts per child: 65 536 pairs P = 32 / 48 / 58 / 64 / 128 / 256 -> 25.9 / 26.2 / 26.7 / 24.9 / 26.9 /
    // 37.7; 1 M pairs 64 / 128 / 251 / 256 -> 194 / 180 / 180 / 175 (one playout per child: 128 / 193 / 256 -> 46.7 / 39.9 /
    // 37.3).  Filling the workgroup's last round of lanes (P = 58: 708 jobs = 2.8 rounds instead of 3.05) does not
    // pay: the chip is bound by the total of wave-rounds, not by a workgroup's own span.
    u32 ppb = (u32)(BLK / (2 * n_sims));                          // the lane-per-playout kernel: whole pairs per workgroup
    if (jobs)
        for (ppb = 8; ppb * 2 <= XR_MAX_PAIRS && (int64_t)ppb * 2 * 1024 <= n;) ppb *= 2;
    return with_bools([&](auto JOBS, auto PK) {
        constexpr auto kernel = JOBS ? expand_rollout_jobs_kernel<BLK, PK> : expand_rollout_kernel<BLK, PK>;
        return launch(kernel, ceil_div(n, ppb), BLK, stream, p.P, p.Q, action36, c0.P, c0.Q, c1.P, c1.Q, o, (u64)seed, step_idx0,
                      (u64)board_offset, (u32)n_sims, ppb, value_sum, result, n);
    }, jobs, key != nullptr);
}

int qttt_encode(const void *state, float *vec, uint8_t *mask, int64_t n, void *stream) {
    if (n < 0) return QTTT_ERR_SIZE;
    if (n == 0) return 0;
    if (any_null(state, vec)) return QTTT_ERR_NULL;
    if (misaligned(vec, 16) || misaligned(mask, 4)) return QTTT_ERR_ACTION;   // vector stores
    const Planes p = planes(const_cast<void *>(state), n);
    return launch(encode_kernel, ceil_div(n, QTTT_ENC_BOARDS), QTTT_ENC_BLOCK, stream, p.P, p.Q, vec, mask, n);
}

// ---------------------------------------------------------------- the environment record; tuning
// The flat step entries are this call on a record of their arguments.
int qttt_env_step(const qttt_env *e, uint8_t *actions, const uint8_t *bits, uint32_t step_idx, int mode,
                  void *stream) {
    if (!e) return QTTT_ERR_NULL;
    switch (mode) {
    case QTTT_ENV_STEP:
        return launch_step(*e, actions, bits, step_idx, stream, false, nullptr);
    case QTTT_ENV_STEP_OBSERVE: {
        const ObsOut o = {e->classical, e->q_p1, e->q_p1_len, e->q_p2, e->q_p2_len, e->turn};
        if (const int rc = obs_check(o, e->n)) return rc;
        return launch_step(*e, actions, bits, step_idx, stream, false, &o);
    }
    case QTTT_ENV_STEP_RANDOM:
        return launch_step(*e, actions, nullptr, step_idx, stream, true, nullptr);
    case QTTT_ENV_SAMPLE:
        return launch_sample(*e, actions, step_idx, stream);
    default:
        return QTTT_ERR_SIZE;
    }
}

int qttt_counter_add(uint32_t *counter, uint32_t by, void *stream) {
    if (!counter) return QTTT_ERR_NULL;
    return launch(counter_add_kernel, 1, 1, stream, counter, by);
}

int qttt_set_tuning(int boards_per_lane, int workgroup_size) {
    if (!(boards_per_lane == 0 || boards_per_lane == 1 || boards_per_lane == 2 || boards_per_lane == 4)) return QTTT_ERR_SIZE;
    if (!(workgroup_size == 0 || workgroup_size == 256 || workgroup_size == 512 || workgroup_size == 1024)) return QTTT_ERR_SIZE;
    tuning_word().store(boards_per_lane | (workgroup_size << 8), std::memory_order_relaxed);
    return 0;
}

int qttt_step_launch_shape(int64_t n, uint32_t flags, int observe, int *boards_per_lane, int *workgroup_size) {
    if (n < 0) return QTTT_ERR_SIZE;
    if (any_null(boards_per_lane, workgroup_size)) return QTTT_ERR_NULL;
    resolve_shape(n, flags, observe != 0, *boards_per_lane, *workgroup_size);
    return 0;
}

int qttt_step_random(void *state, uint64_t seed, uint32_t step_idx, int64_t board_offset,
                     uint32_t flags, uint8_t *actions_out, float *reward, uint8_t *terminated,
                     int64_t n, void *stream) {
    const qttt_env e = {state, n, board_offset, seed, flags, 0u, reward, terminated};
    return qttt_env_step(&e, actions_out, nullptr, step_idx, QTTT_ENV_STEP_RANDOM, stream);
}

uint64_t qttt_hash(uint64_t seed, uint64_t board_id, uint32_t step_idx) {
    const Draw d = counter_draw(fold_id(board_id), launch_key(seed, step_idx));
    return ((u64)d.h2 << 32) | d.h1;
}

// ---------------------------------------------------------------- the network (include/qttt_nn.h, qttt_policy_rollout.h)
int64_t qttt_nn_weights_bytes(int precision) {
    if (precision == QTTT_NN_F32) return NNBlob<0>::BYTES;
    if (precision == QTTT_NN_BF16) return NNBlob<1>::BYTES;
    return -1;
}

int qttt_evaluate(const void *state, const void *weights, int precision, float *value, float *logits, float *probs,
                  int64_t n, void *stream) {
    if (n < 0 || (precision != QTTT_NN_F32 && precision != QTTT_NN_BF16)) return QTTT_ERR_SIZE;
    if (n == 0) return 0;
    if (any_null(state, weights) || (!value && !logits && !probs)) return QTTT_ERR_NULL;
    if (misaligned(weights, 16) || misaligned(value, 4) || misaligned(logits, 4) || misaligned(probs, 4))
        return QTTT_ERR_ACTION;                                  // 16-byte fragment loads / f32 stores
    const Planes p = planes(const_cast<void *>(state), n);
    return with_int<QTTT_NN_F32, QTTT_NN_BF16>(precision, [&](auto P) {
        return launch(evaluate_kernel<P>, ceil_div(n, NNCfg<P>::M), QTTT_NN_BLOCK, stream, p.P, p.Q, weights, value, logits,
                      probs, n);
    });
}

int qttt_rollout_policy(const void *state, const void *weights, int precision, uint64_t seed, uint32_t step_idx0,
                        int64_t board_offset, int n_sims, int8_t *result, uint8_t *plies, uint8_t *trace,
                        float *leaf_value, float *leaf_probs, int64_t n, void *stream) {
    if (n < 0 || board_offset < 0 || (precision != QTTT_NN_F32 && precision != QTTT_NN_BF16) || n_sims < 1 ||
        n_sims > QTTT_POLICY_ROLLOUT_MAX_SIMS)
        return QTTT_ERR_SIZE;
    if (n == 0) return 0;
    if (any_null(state, weights, result)) return QTTT_ERR_NULL;
    if (misaligned(weights, 16) || misaligned(leaf_value, 4) || misaligned(leaf_probs, 4))
        return QTTT_ERR_ACTION;                                  // 16-byte fragment loads / f32 stores
    const Planes p = planes(const_cast<void *>(state), n);
    const int64_t lanes = n * (int64_t)n_sims;
    return with_int<QTTT_NN_F32, QTTT_NN_BF16>(precision, [&](auto P) {
        return launch(rollout_policy_kernel<P>, ceil_div(lanes, NNCfg<P>::M), QTTT_NN_BLOCK, stream, p.P, p.Q, weights,
                      (u64)seed, step_idx0, (u64)board_offset, (u32)n_sims, result, plies, trace, leaf_value, leaf_probs, lanes);
    });
}

// ---------------------------------------------------------------- search trees (include/qttt_tree.h)
int64_t qttt_tree_bytes(int64_t games, int64_t capacity) {
    if (tree_size_bad(games, capacity)) return QTTT_ERR_SIZE;
    const int64_t per_game = QTTT_TREE_GAME_BYTES + capacity * (int64_t)(QTTT_TREE_NODE_BYTES + QTTT_TREE_PRIOR_BYTES);
    if (games > 0 && per_game > INT64_MAX / games) return QTTT_ERR_SIZE;
    return games * per_game;
}

int qttt_tree_reset(void *tree, int64_t games, int64_t capacity, const void *state, void *stream) {
    if (tree_size_bad(games, capacity)) return QTTT_ERR_SIZE;
    if (games == 0) return 0;
    if (any_null(tree, state)) return QTTT_ERR_NULL;
    if (misaligned(tree, 16)) return QTTT_ERR_ACTION;
    const Planes p = planes(const_cast<void *>(state), games);
    return launch(tree_reset_kernel, ceil_div(games, TREE_GAMES_PER_BLOCK), TREE_BLOCK, stream, tree, games, capacity, p.P, p.Q);
}

int qttt_tree_select(void *tree, int64_t games, int64_t capacity, uint64_t seed, uint32_t rollout_idx,
                     int64_t board_offset, double c_puct, void *leaf_state, void *stream) {
    if (tree_size_bad(games, capacity) || board_offset < 0 || rollout_idx >= QTTT_TREE_MAX_ROLLOUTS) return QTTT_ERR_SIZE;
    if (games == 0) return 0;
    if (any_null(tree, leaf_state)) return QTTT_ERR_NULL;
    if (misaligned(tree, 16)) return QTTT_ERR_ACTION;
    const Planes l = planes(leaf_state, games);
    return launch(tree_select_kernel, ceil_div(games, TREE_GAMES_PER_BLOCK), TREE_BLOCK, stream, tree, games, capacity, (u64)seed, rollout_idx,
                  (u64)board_offset, c_puct, l.P, l.Q);
}

int qttt_tree_backup(void *tree, int64_t games, int64_t capacity, const int8_t *result, int n_sims,
                     const float *leaf_probs, void *stream) {
    if (tree_size_bad(games, capacity) || n_sims < 1 || n_sims > QTTT_TREE_MAX_SIMS) return QTTT_ERR_SIZE;
    if (games == 0) return 0;
    if (any_null(tree, result)) return QTTT_ERR_NULL;
    if (misaligned(tree, 16) || misaligned(leaf_probs, 4)) return QTTT_ERR_ACTION;
    return launch(tree_backup_kernel, ceil_div(games, TREE_GAMES_PER_BLOCK), TREE_BLOCK, stream, tree, games, capacity, result, (u32)n_sims,
                  leaf_probs);
}

int qttt_tree_sync(void *tree, int64_t games, int64_t capacity, const void *state, void *stream) {
    if (tree_size_bad(games, capacity)) return QTTT_ERR_SIZE;
    if (games == 0) return 0;
    if (any_null(tree, state)) return QTTT_ERR_NULL;
    if (misaligned(tree, 16)) return QTTT_ERR_ACTION;
    const Planes p = planes(const_cast<void *>(state), games);
    return launch(tree_sync_kernel, ceil_div(games, TREE_GAMES_PER_BLOCK), TREE_BLOCK, stream, tree, games, capacity, p.P, p.Q);
}

int64_t qttt_tree_compact_bytes(int64_t games, int64_t capacity) {
    if (tree_size_bad(games, capacity)) return QTTT_ERR_SIZE;
    if (games > 0 && 4 * capacity > INT64_MAX / games) return QTTT_ERR_SIZE;
    return 4 * games * capacity;
}

int qttt_tree_compact(void *tree, int64_t games, int64_t capacity, void *scratch, void *stream) {
    if (tree_size_bad(games, capacity)) return QTTT_ERR_SIZE;
    if (games == 0) return 0;
    if (any_null(tree, scratch)) return QTTT_ERR_NULL;
    if (misaligned(tree, 16) || misaligned(scratch, 4)) return QTTT_ERR_ACTION;
    return launch(tree_compact_kernel, ceil_div(games, TREE_GAMES_PER_BLOCK), TREE_BLOCK, stream, tree, games, capacity,
                  (int32_t *)scratch);
}

int qttt_tree_root(const void *tree, int64_t games, int64_t capacity, int32_t *N, double *W, double *Q, double *P,
                   int32_t *Ntot, uint8_t *choose, int32_t *nodes_used, uint8_t *overflow, void *stream) {
    if (tree_size_bad(games, capacity)) return QTTT_ERR_SIZE;
    if (games == 0) return 0;
    if (!tree) return QTTT_ERR_NULL;
    if (misaligned(tree, 16) || misaligned(N, 4) || misaligned(Ntot, 4) || misaligned(nodes_used, 4) || misaligned(W, 8) ||
        misaligned(Q, 8) || misaligned(P, 8))
        return QTTT_ERR_ACTION;
    const TreeRootOut o = {N, W, Q, P, Ntot, choose, nodes_used, overflow};
    return launch(tree_root_kernel, ceil_div(games, TREE_GAMES_PER_BLOCK), TREE_BLOCK, stream, tree, games, capacity, o);
}

int qttt_tree_sqrt(uint32_t first, int64_t n, double *out, void *stream) {
    if (n < 0) return QTTT_ERR_SIZE;
    if (n == 0) return 0;
    if (!out) return QTTT_ERR_NULL;
    if (misaligned(out, 8)) return QTTT_ERR_ACTION;
    return launch(tree_sqrt_kernel, ceil_div(n, 256), 256, stream, first, n, out);
}

int qttt_tree_score(const double *W, const uint32_t *N, const double *prior, const uint32_t *Ntot, double c_puct,
                    int64_t n, double *out, void *stream) {
    if (n < 0) return QTTT_ERR_SIZE;
    if (n == 0) return 0;
    if (any_null(W, N, prior, Ntot, out)) return QTTT_ERR_NULL;
    if (misaligned(W, 8) || misaligned(prior, 8) || misaligned(out, 8) || misaligned(N, 4) || misaligned(Ntot, 4))
        return QTTT_ERR_ACTION;
    return launch(tree_score_kernel, ceil_div(n, 256), 256, stream, W, N, prior, Ntot, c_puct, n, out);
}

// ---------------------------------------------------------------- self-play (include/qttt_selfplay.h)
int qttt_selfplay_record(const void *tree, int64_t games, int64_t capacity, int ply, uint32_t n_rollouts, double alpha,
                         double v_first, double v_second, void *states, double *pi, uint8_t *mask, uint8_t *done,
                         float *v, uint8_t *action36, uint8_t *length, int8_t *winner, uint8_t *actions, void *stream) {
    const RecordArgs a = {tree, states, pi, mask, done, v, action36, length, winner, actions};
    bool work;
    if (const int rc = record_check(RECORD_PLAIN, false, a, games, capacity, ply, 0u, n_rollouts, alpha, v_first, v_second, {}, work);
        rc || !work)
        return rc;
    return record_launch<RECORD_PLAIN, false>(a, games, capacity, ply, n_rollouts, alpha, v_first, v_second, {}, stream);
}

// ---------------------------------------------------------------- symmetries (include/qttt_symmetry.h)
int qttt_symmetry_tables(uint8_t *cells, uint8_t *actions, uint8_t *inverse, uint8_t *compose) {
    for (u32 k = 0; k < (u32)QTTT_SYMMETRIES; ++k) {
        for (u32 v = 0; v < 9u && cells; ++v) cells[k * 9u + v] = (uint8_t)sym_cell(SYM_TABLES.cells[k], v);
        for (u32 i = 0, a = 0; i < 9u && actions; ++i)
            for (u32 j = i + 1u; j < 9u; ++j, ++a) actions[k * 36u + a] = (uint8_t)sym_action_of_pair(SYM_TABLES.cells[k], i | (j << 4));
        if (inverse) inverse[k] = SYM_TABLES.inverse[k];
        for (u32 b = 0; b < (u32)QTTT_SYMMETRIES && compose; ++b) compose[k * QTTT_SYMMETRIES + b] = SYM_TABLES.compose[k][b];
    }
    return 0;
}

int qttt_transform(const void *state_in, void *state_out, const uint8_t *sym, int k, int64_t n, void *stream) {
    if (n < 0 || k < 0 || k >= QTTT_SYMMETRIES) return QTTT_ERR_SIZE;
    if (n == 0) return 0;
    if (any_null(state_in, state_out)) return QTTT_ERR_NULL;
    if (misaligned(state_in, 16) || misaligned(state_out, 16)) return QTTT_ERR_ACTION;
    const Planes i = planes(const_cast<void *>(state_in), n), o = planes(state_out, n);
    return launch(transform_kernel, ceil_div(n, QTTT_COLD_BLOCK), QTTT_COLD_BLOCK, stream, i.P, i.Q, o.P, o.Q, sym, (u32)k, n);
}

int qttt_selfplay_augment(int64_t games, const uint8_t *symmetries, int n_sym, const void *states, const double *pi,
                          const uint8_t *mask, const uint8_t *done, const float *v, const uint8_t *action36,
                          const uint8_t *length, const int8_t *winner, const uint8_t *actions, void *states_out,
                          double *pi_out, uint8_t *mask_out, uint8_t *done_out, float *v_out, uint8_t *action36_out,
                          uint8_t *length_out, int8_t *winner_out, uint8_t *actions_out, void *stream) {
    if (games < 0 || n_sym < 1 || n_sym > QTTT_SYMMETRIES || games > INT64_MAX / (36 * QTTT_SELFPLAY_ROWS * QTTT_SYMMETRIES))
        return QTTT_ERR_SIZE;
    u32 syms = 0;
    for (int s = 0; s < n_sym && symmetries; ++s) {
        if (symmetries[s] >= QTTT_SYMMETRIES) return QTTT_ERR_SIZE;
        syms |= (u32)symmetries[s] << (4 * s);
    }
    if (games == 0) return 0;
    if (!symmetries || any_null(states, pi, mask, done, v, action36, length, winner, actions) ||
        any_null(states_out, pi_out, mask_out, done_out, v_out, action36_out, length_out, winner_out, actions_out))
        return QTTT_ERR_NULL;
    if (misaligned(states, 16) || misaligned(states_out, 16) || misaligned(pi, 8) || misaligned(pi_out, 8) ||
        misaligned(v, 4) || misaligned(v_out, 4))
        return QTTT_ERR_ACTION;
    const SelfPlayOut in = selfplay_out(states, pi, mask, done, v, action36, length, winner, actions);
    const SelfPlayOut out = selfplay_out(states_out, pi_out, mask_out, done_out, v_out, action36_out, length_out, winner_out,
                                         actions_out);
    return launch(selfplay_augment_kernel, ceil_div(games * n_sym, TREE_GAMES_PER_BLOCK), TREE_BLOCK, stream, games, (u32)n_sym,
                  syms, in, out);
}

// ---------------------------------------------------------------- the network over symmetries (include/qttt_nn_symmetric.h)
int qttt_evaluate_symmetric(const void *state, const void *weights, int precision, const uint8_t *symmetries, int n_sym,
                            const uint8_t *sym, float *value, float *logits, float *probs, int64_t n, void *stream) {
    if (n < 0 || n > INT64_MAX / QTTT_SYMMETRIES || (precision != QTTT_NN_F32 && precision != QTTT_NN_BF16) ||
        !(n_sym == 1 || n_sym == 2 || n_sym == 4 || n_sym == 8) || (sym && n_sym != 1))
        return QTTT_ERR_SIZE;
    u32 syms = 0, ls = 0;
    for (int s = 0; s < n_sym && !sym && symmetries; ++s) {
        if (symmetries[s] >= QTTT_SYMMETRIES) return QTTT_ERR_SIZE;
        syms |= (u32)symmetries[s] << (4 * s);
    }
    while ((1 << ls) < n_sym) ++ls;
    if (n == 0) return 0;
    if (any_null(state, weights) || (!sym && !symmetries) || (!value && !logits && !probs)) return QTTT_ERR_NULL;
    if (misaligned(weights, 16) || misaligned(value, 4) || misaligned(logits, 4) || misaligned(probs, 4))
        return QTTT_ERR_ACTION;                                  // 16-byte fragment loads / f32 stores
    const Planes p = planes(const_cast<void *>(state), n);
    return with_int<QTTT_NN_F32, QTTT_NN_BF16>(precision, [&](auto P) {
        return launch(evaluate_symmetric_kernel<P>, ceil_div(n, NNCfg<P>::M >> ls), QTTT_NN_BLOCK, stream, p.P, p.Q, weights,
                      sym, syms, ls, value, logits, probs, n);
    });
}

// ---------------------------------------------------------------- the value rollout (include/qttt_tree_value.h)
int qttt_tree_value_rollout(void *tree, int64_t games, int64_t capacity, const void *leaf_state, const void *weights,
                            int precision, float *leaf_value, float *leaf_probs, void *stream) {
    if (tree_size_bad(games, capacity) || (precision != QTTT_NN_F32 && precision != QTTT_NN_BF16)) return QTTT_ERR_SIZE;
    if (games == 0) return 0;
    if (any_null(tree, leaf_state, weights)) return QTTT_ERR_NULL;
    if (misaligned(tree, 16) || misaligned(weights, 16) || misaligned(leaf_value, 4) || misaligned(leaf_probs, 4))
        return QTTT_ERR_ACTION;                                  // 16-byte node vectors and fragment loads / f32 stores
    const Planes l = planes(const_cast<void *>(leaf_state), games);
    return with_int<QTTT_NN_F32, QTTT_NN_BF16>(precision, [&](auto P) {
        return launch(tree_value_rollout_kernel<P>, ceil_div(games, NNCfg<P>::M), QTTT_NN_BLOCK, stream, tree, games, capacity,
                      l.P, l.Q, weights, leaf_value, leaf_probs);
    });
}

// ---------------------------------------------------------------- leaf-parallel rounds (include/qttt_tree_leaves.h)
int64_t qttt_tree_paths_bytes(int64_t games, int leaves) {
    if (tree_leaves_bad(games, leaves)) return QTTT_ERR_SIZE;
    return games * leaves * (int64_t)QTTT_TREE_PATH_BYTES;
}

int qttt_tree_select_batch(void *tree, int64_t games, int64_t capacity, uint64_t seed, uint32_t rollout_idx0, int leaves,
                           int64_t board_offset, double c_puct, double virtual_loss, void *paths, void *leaf_state,
                           void *stream) {
    bool work;
    if (const int rc = select_batch_check(SELECT_PUCT, tree, games, capacity, rollout_idx0, leaves, board_offset, virtual_loss, paths,
                                      leaf_state, {}, work); rc || !work) return rc;
    const Planes l = planes(leaf_state, games * leaves);
    return launch(tree_select_batch_kernel, ceil_div(games, TREE_GAMES_PER_BLOCK), TREE_BLOCK, stream, tree, games, capacity,
                  (u64)seed, rollout_idx0, (u32)leaves, (u64)board_offset, c_puct, virtual_loss, static_cast<TreePathRec *>(paths),
                  l.P, l.Q);
}

int qttt_tree_backup_batch(void *tree, int64_t games, int64_t capacity, int leaves, const void *paths,
                           const float *leaf_value, const float *leaf_probs, void *stream) {
    return backup_batch<false>(tree, games, capacity, leaves, paths, leaf_value, leaf_probs, stream);
}

// ---------------------------------------------------------------- root exploration (include/qttt_tree_explore.h)
int qttt_tree_root_noise(void *tree, int64_t games, int64_t capacity, uint64_t seed, uint32_t noise_idx,
                         int64_t board_offset, double epsilon, double alpha, double *noise, uint8_t *applied,
                         void *stream) {
    if (tree_size_bad(games, capacity) || board_offset < 0 || noise_idx >= QTTT_TREE_MAX_NOISE || !(epsilon >= 0.0 && epsilon <= 1.0) ||
        !is_finite(alpha) || alpha <= 0.0)
        return QTTT_ERR_SIZE;
    if (games == 0) return 0;
    if (!tree) return QTTT_ERR_NULL;
    if (misaligned(tree, 16) || misaligned(noise, 8)) return QTTT_ERR_ACTION;
    return launch(tree_root_noise_kernel, ceil_div(games, TREE_GAMES_PER_BLOCK), TREE_BLOCK, stream, tree, games, capacity,
                  (u64)seed, noise_idx, (u64)board_offset, epsilon, alpha, noise, applied);
}

int qttt_selfplay_record_sampled(const void *tree, int64_t games, int64_t capacity, int ply, uint32_t n_rollouts,
                                 double alpha, double v_first, double v_second, void *states, double *pi, uint8_t *mask,
                                 uint8_t *done, float *v, uint8_t *action36, uint8_t *length, int8_t *winner,
                                 uint8_t *actions, uint64_t seed, int64_t board_offset, double temperature,
                                 int sample_plies, void *stream) {
    const RecordArgs a = {tree, states, pi, mask, done, v, action36, length, winner, actions};
    bool work;
    if (const int rc = record_check(RECORD_SAMPLED, false, a, games, capacity, ply, 0u, n_rollouts, alpha, v_first, v_second,
                                {board_offset, temperature, sample_plies}, work); rc || !work) return rc;
    const SelfPlaySampling<RECORD_SAMPLED> s = {(u64)seed, (u64)board_offset, temperature, sample_plies};
    return record_launch<RECORD_SAMPLED, false>(a, games, capacity, ply, n_rollouts, alpha, v_first, v_second, s, stream);
}

// ---------------------------------------------------------------- the Gumbel root (include/qttt_tree_gumbel.h)
int64_t qttt_tree_gumbel_bytes(int64_t games) {
    if (games < 0 || games > INT64_MAX / QTTT_TREE_GUMBEL_BYTES) return QTTT_ERR_SIZE;
    return games * (int64_t)QTTT_TREE_GUMBEL_BYTES;
}

int qttt_gumbel_visit_sequence(int m, int n_sims, int32_t *out) {
    if (m < 0 || m > 36 || n_sims < 1 || n_sims > QTTT_TREE_MAX_ROLLOUTS) return QTTT_ERR_SIZE;
    if (!out) return QTTT_ERR_NULL;
    const int n = n_sims;
    if (m <= 1) {
        for (int i = 0; i < n; ++i) out[i] = i;
        return 0;
    }
    int L = 0;
    while ((1 << L) < m) ++L;
    int32_t visits[36] = {0};
    int emitted = 0;
    for (int c = m; emitted < n; c = c / 2 > 2 ? c / 2 : 2) {
        const int e = n / (L * c) > 1 ? n / (L * c) : 1;
        for (int t = 0; t < e; ++t)
            for (int i = 0; i < c; ++i) {
                if (emitted < n) out[emitted++] = visits[i];
                ++visits[i];
            }
    }
    return 0;
}

int qttt_tree_root_states(const void *tree, int64_t games, int64_t capacity, void *state_out, void *stream) {
    if (tree_size_bad(games, capacity)) return QTTT_ERR_SIZE;
    if (games == 0) return 0;
    if (any_null(tree, state_out)) return QTTT_ERR_NULL;
    if (misaligned(tree, 16) || misaligned(state_out, 16)) return QTTT_ERR_ACTION;
    const Planes p = planes(state_out, games);
    return launch(tree_root_states_kernel, ceil_div(games, TREE_BLOCK), TREE_BLOCK, stream, tree, games, capacity, p.P, p.Q);
}

int qttt_tree_gumbel_begin(const void *tree, int64_t games, int64_t capacity, uint64_t seed, uint32_t move_idx,
                           int64_t board_offset, int max_considered, const float *root_value, const float *root_logits,
                           void *rec, void *stream) {
    if (tree_size_bad(games, capacity) || board_offset < 0 || max_considered < 1 || max_considered > 36 ||
        move_idx >= QTTT_TREE_MAX_GUMBEL || games > INT64_MAX / QTTT_TREE_GUMBEL_BYTES)
        return QTTT_ERR_SIZE;
    if (games == 0) return 0;
    if (any_null(tree, root_value, root_logits, rec)) return QTTT_ERR_NULL;
    if (misaligned(tree, 16) || misaligned(rec, 16) || misaligned(root_value, 4) || misaligned(root_logits, 4)) return QTTT_ERR_ACTION;
    return launch(tree_gumbel_begin_kernel, ceil_div(games, TREE_GAMES_PER_BLOCK), TREE_BLOCK, stream, tree, games, capacity,
                  (u64)seed, move_idx, (u64)board_offset, (u32)max_considered, root_value, root_logits, static_cast<GumbelRec *>(rec));
}

int qttt_tree_select_batch_gumbel(void *tree, int64_t games, int64_t capacity, uint64_t seed, uint32_t rollout_idx0,
                                  int leaves, int64_t board_offset, double c_puct, double virtual_loss, void *paths,
                                  void *leaf_state, const void *rec, const int32_t *visit_table, int n_sims, int sim_idx0,
                                  double c_visit, double c_scale, void *stream) {
    bool work;
    if (const int rc = select_batch_check(SELECT_GUMBEL, tree, games, capacity, rollout_idx0, leaves, board_offset, virtual_loss, paths,
                                      leaf_state, {0.0, rec, visit_table, n_sims, sim_idx0, c_visit, c_scale}, work);
        rc || !work)
        return rc;
    const Planes l = planes(leaf_state, games * leaves);
    return launch(tree_select_batch_gumbel_kernel, ceil_div(games, TREE_GAMES_PER_BLOCK), TREE_BLOCK, stream, tree, games, capacity,
                  (u64)seed, rollout_idx0, (u32)leaves, (u64)board_offset, c_puct, virtual_loss, static_cast<TreePathRec *>(paths),
                  l.P, l.Q, static_cast<const GumbelRec *>(rec), visit_table, (u32)n_sims, (u32)sim_idx0, c_visit, c_scale);
}

int qttt_tree_gumbel_root(const void *tree, const void *rec, int64_t games, int64_t capacity, double c_visit,
                          double c_scale, uint8_t *choose, double *pi, double *q_completed, void *stream) {
    if (tree_size_bad(games, capacity) || gumbel_scale_bad(c_visit, c_scale)) return QTTT_ERR_SIZE;
    if (games == 0) return 0;
    if (any_null(tree, rec)) return QTTT_ERR_NULL;
    if (misaligned(tree, 16) || misaligned(rec, 16) || misaligned(pi, 8) || misaligned(q_completed, 8)) return QTTT_ERR_ACTION;
    return launch(tree_gumbel_root_kernel, ceil_div(games, TREE_GAMES_PER_BLOCK), TREE_BLOCK, stream, tree,
                  static_cast<const GumbelRec *>(rec), games, capacity, c_visit, c_scale, choose, pi, q_completed);
}

int qttt_selfplay_record_gumbel(const void *tree, int64_t games, int64_t capacity, int ply, uint32_t n_rollouts,
                                double alpha, double v_first, double v_second, void *states, double *pi, uint8_t *mask,
                                uint8_t *done, float *v, uint8_t *action36, uint8_t *length, int8_t *winner,
                                uint8_t *actions, const void *rec, double c_visit, double c_scale, void *stream) {
    const RecordArgs a = {tree, states, pi, mask, done, v, action36, length, winner, actions};
    bool work;
    if (const int rc = record_check(RECORD_GUMBEL, false, a, games, capacity, ply, 0u, n_rollouts, alpha, v_first, v_second,
                                {0, 0.0, 0, 0.0, 0.0, rec, c_visit, c_scale}, work); rc || !work) return rc;
    const SelfPlaySampling<RECORD_GUMBEL> s = {static_cast<const GumbelRec *>(rec), c_visit, c_scale};
    return record_launch<RECORD_GUMBEL, false>(a, games, capacity, ply, n_rollouts, alpha, v_first, v_second, s, stream);
}

// ---------------------------------------------------------------- forced playouts and pruned targets (include/qttt_tree_forced.h)
int qttt_tree_select_batch_forced(void *tree, int64_t games, int64_t capacity, uint64_t seed, uint32_t rollout_idx0,
                                  int leaves, int64_t board_offset, double c_puct, double virtual_loss, void *paths,
                                  void *leaf_state, double forced_k, void *stream) {
    bool work;
    if (const int rc = select_batch_check(SELECT_FORCED, tree, games, capacity, rollout_idx0, leaves, board_offset, virtual_loss, paths,
                                      leaf_state, {forced_k}, work); rc || !work) return rc;
    const Planes l = planes(leaf_state, games * leaves);
    return launch(tree_select_batch_forced_kernel, ceil_div(games, TREE_GAMES_PER_BLOCK), TREE_BLOCK, stream, tree, games, capacity,
                  (u64)seed, rollout_idx0, (u32)leaves, (u64)board_offset, c_puct, virtual_loss, static_cast<TreePathRec *>(paths),
                  l.P, l.Q, forced_k);
}

int qttt_tree_root_forced(const void *tree, int64_t games, int64_t capacity, double forced_k, double c_puct,
                          uint8_t *forced, int32_t *n_pruned, void *stream) {
    bool work;
    const int rc = forced_root_check(tree, games, capacity, forced_k, c_puct, n_pruned, work);
    if (rc || !work) return rc;
    return launch(tree_root_forced_kernel, ceil_div(games, TREE_GAMES_PER_BLOCK), TREE_BLOCK, stream, tree, games, capacity,
                  forced_k, c_puct, forced, n_pruned);
}

int qttt_selfplay_record_pruned(const void *tree, int64_t games, int64_t capacity, int ply, uint32_t n_rollouts,
                                double alpha, double v_first, double v_second, void *states, double *pi, uint8_t *mask,
                                uint8_t *done, float *v, uint8_t *action36, uint8_t *length, int8_t *winner,
                                uint8_t *actions, uint64_t seed, int64_t board_offset, double temperature,
                                int sample_plies, double forced_k, double c_puct, void *stream) {
    const RecordArgs a = {tree, states, pi, mask, done, v, action36, length, winner, actions};
    bool work;
    if (const int rc = record_check(RECORD_PRUNED, false, a, games, capacity, ply, 0u, n_rollouts, alpha, v_first, v_second,
                                {board_offset, temperature, sample_plies, forced_k, c_puct}, work); rc || !work) return rc;
    const SelfPlaySampling<RECORD_PRUNED> s = {(u64)seed, (u64)board_offset, temperature, sample_plies, forced_k, c_puct};
    return record_launch<RECORD_PRUNED, false>(a, games, capacity, ply, n_rollouts, alpha, v_first, v_second, s, stream);
}

int qttt_selfplay_record_stream_pruned(const void *tree, int64_t games, int64_t capacity, uint32_t n_rollouts, double alpha,
                                       double v_first, double v_second, void *states, double *pi, uint8_t *mask,
                                       uint8_t *done, float *v, uint8_t *action36, uint8_t *length, int8_t *winner,
                                       uint8_t *actions, uint64_t seed, int64_t board_offset, double temperature,
                                       int sample_plies, uint32_t draw_index, double forced_k, double c_puct, void *stream) {
    const RecordArgs a = {tree, states, pi, mask, done, v, action36, length, winner, actions};
    bool work;
    if (const int rc = record_check(RECORD_PRUNED, true, a, games, capacity, 0, draw_index, n_rollouts, alpha, v_first, v_second,
                                {board_offset, temperature, sample_plies, forced_k, c_puct}, work); rc || !work) return rc;
    const SelfPlaySampling<RECORD_PRUNED> s = {(u64)seed, (u64)board_offset, temperature, sample_plies, forced_k, c_puct};
    return record_launch<RECORD_PRUNED, true>(a, games, capacity, (int)draw_index, n_rollouts, alpha, v_first, v_second, s, stream);
}

// ---------------------------------------------------------------- rounds and noise for a listed subset (include/qttt_tree_subset.h)
int qttt_tree_select_batch_subset(void *tree, int64_t games, int64_t capacity, uint64_t seed, uint32_t rollout_idx0,
                                  int leaves, int64_t board_offset, double c_puct, double virtual_loss, double forced_k,
                                  const int32_t *ids, int64_t n_ids, void *paths, void *leaf_state, void *stream) {
    bool work;
    if (const int rc = subset_select_check(tree, games, capacity, rollout_idx0, leaves, board_offset, virtual_loss, forced_k, ids,
                                           n_ids, paths, leaf_state, work); rc || !work) return rc;
    const Planes l = planes(leaf_state, n_ids * leaves);
    const auto go = [&](auto kernel) {
        return launch(kernel, ceil_div(n_ids, TREE_GAMES_PER_BLOCK), TREE_BLOCK, stream, tree, games, capacity, (u64)seed,
                      rollout_idx0, (u32)leaves, (u64)board_offset, c_puct, virtual_loss, forced_k, ids, n_ids,
                      static_cast<TreePathRec *>(paths), l.P, l.Q);
    };
    return forced_k >= 0.0 ? go(tree_select_batch_subset_kernel<true>) : go(tree_select_batch_subset_kernel<false>);
}

int qttt_tree_backup_batch_subset(void *tree, int64_t games, int64_t capacity, int leaves, const int32_t *ids,
                                  int64_t n_ids, const void *paths, const float *leaf_value, const float *leaf_probs,
                                  void *stream) {
    bool work;
    if (const int rc = subset_backup_check(tree, games, capacity, leaves, ids, n_ids, paths, leaf_value, leaf_probs, work);
        rc || !work)
        return rc;
    return launch(tree_backup_batch_subset_kernel, ceil_div(n_ids, TREE_GAMES_PER_BLOCK), TREE_BLOCK, stream, tree, games, capacity,
                  (u32)leaves, ids, n_ids, static_cast<const TreePathRec *>(paths), leaf_value, leaf_probs);
}

int qttt_tree_root_noise_subset(void *tree, int64_t games, int64_t capacity, uint64_t seed, uint32_t noise_idx,
                                int64_t board_offset, double epsilon, double alpha, const int32_t *ids, int64_t n_ids,
                                double *noise, uint8_t *applied, void *stream) {
    bool work;
    if (const int rc = subset_noise_check(tree, games, capacity, noise_idx, board_offset, epsilon, alpha, ids, n_ids, noise, work);
        rc || !work)
        return rc;
    return launch(tree_root_noise_subset_kernel, ceil_div(n_ids, TREE_GAMES_PER_BLOCK), TREE_BLOCK, stream, tree, games, capacity,
                  (u64)seed, noise_idx, (u64)board_offset, epsilon, alpha, ids, n_ids, noise, applied);
}

// ---------------------------------------------------------------- the capped record and harvest (include/qttt_selfplay_cap.h)
int qttt_selfplay_record_capped(const void *tree, int64_t games, int64_t capacity, uint32_t n_rollouts, double alpha,
                                double v_first, double v_second, void *states, double *pi, uint8_t *mask, uint8_t *done,
                                float *v, uint8_t *action36, uint8_t *length, int8_t *winner, uint8_t *actions,
                                uint64_t seed, int64_t board_offset, double temperature, int sample_plies,
                                uint32_t draw_index, double forced_k, double c_puct, const uint8_t *full, void *stream) {
    const RecordArgs a = {tree, states, pi, mask, done, v, action36, length, winner, actions};
    const bool pruned = forced_k >= 0.0;
    bool work;
    if (!is_finite(forced_k)) return QTTT_ERR_SIZE;
    if (const int rc = record_check(pruned ? RECORD_PRUNED : RECORD_SAMPLED, true, a, games, capacity, 0, draw_index, n_rollouts,
                                    alpha, v_first, v_second,
                                    {board_offset, temperature, sample_plies, forced_k, c_puct, nullptr, 0.0, 0.0, true, full}, work);
        rc || !work)
        return rc;
    const SelfPlayOut o = selfplay_out(a.states, a.pi, a.mask, a.done, a.v, a.action36, a.length, a.winner, a.actions);
    const int64_t grid = ceil_div(games, TREE_GAMES_PER_BLOCK);
    if (pruned) {
        const SelfPlaySampling<RECORD_PRUNED> s = {(u64)seed, (u64)board_offset, temperature, sample_plies, forced_k, c_puct};
        return launch(selfplay_record_capped_kernel<RECORD_PRUNED>, grid, TREE_BLOCK, stream, tree, games, capacity, (int)draw_index,
                      n_rollouts, alpha, (float)v_first, (float)v_second, o, s, full);
    }
    const SelfPlaySampling<RECORD_SAMPLED> s = {(u64)seed, (u64)board_offset, temperature, sample_plies};
    return launch(selfplay_record_capped_kernel<RECORD_SAMPLED>, grid, TREE_BLOCK, stream, tree, games, capacity, (int)draw_index,
                  n_rollouts, alpha, (float)v_first, (float)v_second, o, s, full);
}

int qttt_selfplay_harvest_capped(const void *tree, int64_t games, int64_t capacity, double v_first, double v_second,
                                 void *states, double *pi, uint8_t *mask, uint8_t *done, float *v, uint8_t *action36,
                                 uint8_t *length, int8_t *winner, uint8_t *actions, uint8_t *harvest_len, uint8_t *finished,
                                 int64_t *games_done, int64_t *tally, void *stream) {
    const SelfPlayOut o = selfplay_out(states, pi, mask, done, v, action36, length, winner, actions);
    const SelfPlayHarvest hv = {harvest_len, finished, games_done, tally};
    bool work;
    if (const int rc = harvest_check(tree, games, capacity, v_first, v_second, o, hv, work); rc || !work) return rc;
    return launch(selfplay_harvest_capped_kernel, ceil_div(games, TREE_GAMES_PER_BLOCK), TREE_BLOCK, stream, tree, games, capacity,
                  (float)v_first, (float)v_second, o, hv);
}

// ---------------------------------------------------------------- the resident search (include/qttt_tree_resident.h)
int qttt_tree_search_resident(void *tree, int64_t games, int64_t capacity, uint64_t seed, uint32_t rollout_idx0, int leaves,
                              uint32_t rollouts, int64_t board_offset, double c_puct, double virtual_loss, double forced_k,
                              const void *weights, int precision, void *stream) {
    bool work;
    if (const int rc = resident_search_check(tree, games, capacity, rollout_idx0, leaves, rollouts, board_offset, virtual_loss,
                                             forced_k, weights, precision, work); rc || !work) return rc;
    const int64_t grid = ceil_div(games, (int64_t)resident_games_per_group(leaves, precision));
    return with_int<QTTT_NN_F32, QTTT_NN_BF16>(precision, [&](auto P) {
        const auto go = [&](auto kernel) {
            return launch(kernel, grid, QTTT_NN_BLOCK, stream, tree, games, capacity, (u64)seed, rollout_idx0, (u32)leaves,
                          rollouts, (u64)board_offset, c_puct, virtual_loss, forced_k, weights);
        };
        return forced_k >= 0.0 ? go(tree_search_resident_kernel<P, true>) : go(tree_search_resident_kernel<P, false>);
    });
}

int qttt_tree_resident_games_per_group(int leaves, int precision) { return resident_games_per_group(leaves, precision); }

int qttt_tree_resident_plan(int leaves, uint32_t rollouts, int32_t *rounds_out, int cap) {
    return resident_plan(leaves, rollouts, rounds_out, cap);
}

// ---------------------------------------------------------------- the replay ring (include/qttt_replay.h)
int64_t qttt_replay_bytes(int64_t capacity) {
    return replay_capacity_bad(capacity) ? (int64_t)QTTT_ERR_SIZE : replay_layout(capacity).bytes;
}

int qttt_replay_layout(int64_t capacity, int64_t *offsets) {
    if (replay_capacity_bad(capacity)) return QTTT_ERR_SIZE;
    if (!offsets) return QTTT_ERR_NULL;
    const ReplayLayout l = replay_layout(capacity);
    for (int k = 0; k < 6; ++k) offsets[k] = l.off[k];
    return 0;
}

int64_t qttt_replay_append_scratch_bytes(int64_t games) {
    return replay_games_bad(games) ? (int64_t)QTTT_ERR_SIZE : replay_scan_plan(games).words * 8;
}

int qttt_replay_append(void *replay, int64_t capacity, int64_t games, const void *states, const double *pi,
                       const uint8_t *mask, const uint8_t *done, const float *v, const uint8_t *length, void *scratch,
                       void *stream) {
    bool work;
    if (const int rc = replay_append_check(replay, capacity, games, states, pi, mask, done, v, length, scratch, work)) return rc;
    if (!work) return 0;
    const ReplayRing ring = replay_ring(replay, capacity);
    const ReplayScanPlan plan = replay_scan_plan(games);
    u64 *words = static_cast<u64 *>(scratch);
    ReplayRanks rk = {};
    for (int k = 0; k < plan.levels; ++k) {
        const int64_t grid = plan.n[k + 1];                      // one workgroup per total of the next level
        u64 *arr = words + plan.off[k], *totals = words + plan.off[k + 1];
        const int rc = k == 0 ? launch(replay_scan_kernel<true>, grid, QTTT_REPLAY_SCAN_BLOCK, stream, length, arr, totals, plan.n[k],
                                       (const u64 *)ring.header, words)
                              : launch(replay_scan_kernel<false>, grid, QTTT_REPLAY_SCAN_BLOCK, stream, length, arr, totals, plan.n[k],
                                       (const u64 *)ring.header, words);
        if (rc) return rc;
        rk.excl[k] = arr;
    }
    rk.total = words + plan.off[plan.levels];
    rk.written0 = words;
    rk.levels = (u32)plan.levels;
    return launch(replay_append_kernel, ceil_div(games, REPLAY_APPEND_GAMES), REPLAY_APPEND_BLOCK, stream, ring, capacity, games,
                  static_cast<const u64 *>(states), reinterpret_cast<const u64 *>(pi), mask, done, reinterpret_cast<const u32 *>(v),
                  length, rk);
}

int qttt_replay_sample(const void *replay, int64_t capacity, int64_t n, uint64_t seed, uint32_t draw, const uint8_t *sym,
                       int random_symmetry, float *s_out, double *pi_out, uint8_t *mask_out, float *v_out,
                       uint8_t *done_out, int32_t *index_out, uint8_t *sym_out, void *stream) {
    bool work;
    if (const int rc = replay_sample_check(replay, capacity, n, draw, s_out, pi_out, mask_out, v_out, done_out, index_out, work))
        return rc;
    if (!work) return 0;
    const ReplayRing ring = replay_ring(const_cast<void *>(replay), capacity);
    const u64 key_slot = launch_key(seed, draw), key_sym = launch_key(seed, draw | 0x80000000u);
    return with_bools([&](auto SYM) {
        return launch(replay_sample_kernel<SYM>, ceil_div(n, REPLAY_TILE), REPLAY_SAMPLE_BLOCK, stream, ring, capacity, n, key_slot,
                      key_sym, sym, (u32)(random_symmetry != 0), s_out, reinterpret_cast<u64 *>(pi_out), mask_out,
                      reinterpret_cast<u32 *>(v_out), done_out, index_out, sym_out);
    }, sym != nullptr || random_symmetry != 0);
}

// ---------------------------------------------------------------- the training step (include/qttt_train.h)
int64_t qttt_train_workspace_bytes(int64_t n) { return train_samples_bad(n) ? -1 : train_plan(n).bytes; }

// qttt_train_gradients and qttt_train_gradients_weighted (include/qttt_train_weighted.h): one body, `weight` null for the first
static int train_gradients(const float *s, const double *pi, const uint8_t *mask, const float *v, const uint8_t *done,
                           const float *weight, int64_t n, const void *weights, void *grads, float *L, float *J, void *workspace,
                           void *stream) {
    const TrainPlan p = train_plan(n);
    char *ws = static_cast<char *>(workspace);
    const auto f32_at = [&](int64_t off) { return reinterpret_cast<float *>(ws + off); };
    float *h[3] = {f32_at(p.h[0]), f32_at(p.h[1]), f32_at(p.h[2])}, *dz[3] = {f32_at(p.dz[0]), f32_at(p.dz[1]), f32_at(p.dz[2])};
    float *dout = f32_at(p.dout), *partials = f32_at(p.partials);
    u32 *n_keep = reinterpret_cast<u32 *>(ws + p.count);
    const float *W = static_cast<const float *>(weights);
    if (const int rc = launch(train_count_kernel, 1, QTTT_NN_BLOCK, stream, done, n, n_keep)) return rc;
    if (const int rc = with_bools([&](auto WEIGHTED) {
            return launch(train_forward_kernel<WEIGHTED>, p.tiles, QTTT_NN_BLOCK, stream, s, pi, mask, v, done, n, W,
                          (const u32 *)n_keep, h[0], h[1], h[2], dout, L, J, weight);
        }, weight != nullptr))
        return rc;
    if (const int rc = launch(train_backward_kernel, p.tiles, QTTT_NN_BLOCK, stream, W, (const float *)dout, (const float *)h[0],
                              (const float *)h[1], (const float *)h[2], dz[0], dz[1], dz[2], n))
        return rc;
    const TrainWgradArgs a = {{s, h[0], h[1], h[2]}, {dz[0], dz[1], dz[2], dout}};
    if (const int rc = launch(train_wgrad_kernel, p.wgrad_groups, QTTT_NN_BLOCK, stream, a, n, partials)) return rc;
    return launch(train_reduce_kernel, p.reduce_groups, QTTT_NN_BLOCK, stream, (const float *)partials, p.chunks,
                  static_cast<float *>(grads));
}

int qttt_train_gradients(const float *s, const double *pi, const uint8_t *mask, const float *v, const uint8_t *done,
                         int64_t n, const void *weights, void *grads, float *L, float *J, void *workspace, void *stream) {
    if (train_samples_bad(n)) return QTTT_ERR_SIZE;
    if (any_null(s, pi, mask, v, done) || any_null(weights, grads, workspace)) return QTTT_ERR_NULL;
    if (misaligned(weights, 16) || misaligned(grads, 16) || misaligned(workspace, 256) || misaligned(pi, 8) ||
        misaligned(s, 4) || misaligned(v, 4) || misaligned(L, 4) || misaligned(J, 4))
        return QTTT_ERR_ACTION;
    return train_gradients(s, pi, mask, v, done, nullptr, n, weights, grads, L, J, workspace, stream);
}

int qttt_train_gradients_weighted(const float *s, const double *pi, const uint8_t *mask, const float *v, const uint8_t *done,
                                  const float *weight, int64_t n, const void *weights, void *grads, float *L, float *J,
                                  void *workspace, void *stream) {
    if (train_samples_bad(n)) return QTTT_ERR_SIZE;
    if (any_null(s, pi, mask, v, done) || any_null(weight, weights, grads, workspace)) return QTTT_ERR_NULL;
    if (misaligned(weights, 16) || misaligned(grads, 16) || misaligned(workspace, 256) || misaligned(pi, 8) ||
        misaligned(s, 4) || misaligned(v, 4) || misaligned(L, 4) || misaligned(J, 4) || misaligned(weight, 4))
        return QTTT_ERR_ACTION;
    return train_gradients(s, pi, mask, v, done, weight, n, weights, grads, L, J, workspace, stream);
}

int qttt_train_adam(void *weights, const void *grads, void *m, void *v2, void *vmax, int64_t step, float lr, float beta1,
                    float beta2, float eps, float weight_decay, void *weights_bf16, void *stream) {
    if (step < 1) return QTTT_ERR_SIZE;
    if (any_null(weights, grads, m, v2, vmax)) return QTTT_ERR_NULL;
    if (misaligned(weights, 16) || misaligned(grads, 16) || misaligned(m, 16) || misaligned(v2, 16) || misaligned(vmax, 16) ||
        misaligned(weights_bf16, 16))
        return QTTT_ERR_ACTION;
    const double bc1 = 1.0 - std::pow((double)beta1, (double)step), bc2 = 1.0 - std::pow((double)beta2, (double)step);
    const TrainAdam h = {beta1, beta2, eps, weight_decay, (float)((double)lr / bc1), (float)std::sqrt(bc2)};
    return launch(train_adam_kernel, ceil_div(TRAIN_BLOB_FLOATS, QTTT_NN_BLOCK), QTTT_NN_BLOCK, stream, static_cast<float *>(weights),
                  static_cast<const float *>(grads), static_cast<float *>(m), static_cast<float *>(v2),
                  static_cast<float *>(vmax), h, weights_bf16);
}

// ---------------------------------------------------------------- continuous self-play (include/qttt_selfplay_stream.h)
int qttt_selfplay_record_stream(const void *tree, int64_t games, int64_t capacity, uint32_t n_rollouts, double alpha,
                                double v_first, double v_second, void *states, double *pi, uint8_t *mask, uint8_t *done,
                                float *v, uint8_t *action36, uint8_t *length, int8_t *winner, uint8_t *actions,
                                void *stream) {
    const RecordArgs a = {tree, states, pi, mask, done, v, action36, length, winner, actions};
    bool work;
    if (const int rc = record_check(RECORD_PLAIN, true, a, games, capacity, 0, 0u, n_rollouts, alpha, v_first, v_second, {}, work);
        rc || !work)
        return rc;
    return record_launch<RECORD_PLAIN, true>(a, games, capacity, 0, n_rollouts, alpha, v_first, v_second, {}, stream);
}

int qttt_selfplay_record_stream_sampled(const void *tree, int64_t games, int64_t capacity, uint32_t n_rollouts, double alpha,
                                        double v_first, double v_second, void *states, double *pi, uint8_t *mask,
                                        uint8_t *done, float *v, uint8_t *action36, uint8_t *length, int8_t *winner,
                                        uint8_t *actions, uint64_t seed, int64_t board_offset, double temperature,
                                        int sample_plies, uint32_t draw_index, void *stream) {
    const RecordArgs a = {tree, states, pi, mask, done, v, action36, length, winner, actions};
    bool work;
    if (const int rc = record_check(RECORD_SAMPLED, true, a, games, capacity, 0, draw_index, n_rollouts, alpha, v_first, v_second,
                                {board_offset, temperature, sample_plies}, work); rc || !work) return rc;
    const SelfPlaySampling<RECORD_SAMPLED> s = {(u64)seed, (u64)board_offset, temperature, sample_plies};
    return record_launch<RECORD_SAMPLED, true>(a, games, capacity, (int)draw_index, n_rollouts, alpha, v_first, v_second, s, stream);
}

int qttt_selfplay_record_stream_gumbel(const void *tree, int64_t games, int64_t capacity, uint32_t n_rollouts, double alpha,
                                       double v_first, double v_second, void *states, double *pi, uint8_t *mask,
                                       uint8_t *done, float *v, uint8_t *action36, uint8_t *length, int8_t *winner,
                                       uint8_t *actions, const void *rec, double c_visit, double c_scale, void *stream) {
    const RecordArgs a = {tree, states, pi, mask, done, v, action36, length, winner, actions};
    bool work;
    if (const int rc = record_check(RECORD_GUMBEL, true, a, games, capacity, 0, 0u, n_rollouts, alpha, v_first, v_second,
                                {0, 0.0, 0, 0.0, 0.0, rec, c_visit, c_scale}, work); rc || !work) return rc;
    const SelfPlaySampling<RECORD_GUMBEL> s = {static_cast<const GumbelRec *>(rec), c_visit, c_scale};
    return record_launch<RECORD_GUMBEL, true>(a, games, capacity, 0, n_rollouts, alpha, v_first, v_second, s, stream);
}

int qttt_selfplay_harvest(const void *tree, int64_t games, int64_t capacity, double v_first, double v_second, void *states,
                          double *pi, uint8_t *mask, uint8_t *done, float *v, uint8_t *action36, uint8_t *length,
                          int8_t *winner, uint8_t *actions, uint8_t *harvest_len, uint8_t *finished, int64_t *games_done,
                          int64_t *tally, void *stream) {
    const SelfPlayOut o = selfplay_out(states, pi, mask, done, v, action36, length, winner, actions);
    const SelfPlayHarvest hv = {harvest_len, finished, games_done, tally};
    bool work;
    if (const int rc = harvest_check(tree, games, capacity, v_first, v_second, o, hv, work); rc || !work) return rc;
    return launch(selfplay_harvest_kernel, ceil_div(games, TREE_GAMES_PER_BLOCK), TREE_BLOCK, stream, tree, games, capacity,
                  (float)v_first, (float)v_second, o, hv);
}

int qttt_selfplay_restart(void *tree, int64_t games, int64_t capacity, void *state, const uint8_t *finished, void *states,
                          double *pi, uint8_t *mask, uint8_t *done, float *v, uint8_t *action36, uint8_t *length,
                          void *stream) {
    if (tree_size_bad(games, capacity)) return QTTT_ERR_SIZE;
    if (games == 0) return 0;
    if (any_null(tree, state, finished, states, pi, mask, done, v, action36, length)) return QTTT_ERR_NULL;
    if (misaligned(tree, 16) || misaligned(state, 16) || misaligned(states, 16) || misaligned(pi, 8) || misaligned(v, 4))
        return QTTT_ERR_ACTION;
    const Planes p = planes(state, games);
    const SelfPlayOut o = selfplay_out(states, pi, mask, done, v, action36, length, nullptr, nullptr);
    return launch(selfplay_restart_kernel, ceil_div(games, TREE_GAMES_PER_BLOCK), TREE_BLOCK, stream, tree, games, capacity, p.P, p.Q,
                  finished, o);
}

// ---------------------------------------------------------------- the exact endgame solver (include/qttt_solve.h)
int qttt_solve(const void *state, int64_t n, int min_ply, float *value, float *q, uint8_t *best, int64_t *nodes,
               uint8_t *status, void *stream) {
    if (n < 0 || min_ply < QTTT_SOLVE_MIN_PLY || min_ply > QTTT_SOLVE_MAX_PLY) return QTTT_ERR_SIZE;
    if (n == 0) return 0;
    if (!state) return QTTT_ERR_NULL;
    if (misaligned(state, 16) || misaligned(value, 4) || misaligned(q, 4) || misaligned(nodes, 8)) return QTTT_ERR_ACTION;
    if (!value && !q && !best && !nodes && !status) return 0;                // nothing asked for
    const Planes p = planes(const_cast<void *>(state), n);
    const SolveOut o = {value, q, best, nodes, status};
    return chunked_launch(n, [&](int64_t i0, int64_t grid) {           // a workgroup per board
        return launch(solve_kernel, grid, SOLVE_BLOCK, stream, (const u64 *)p.P, (const u64 *)p.Q, i0, min_ply, o);
    });
}

// ---------------------------------------------------------------- exact leaves in the search trees (include/qttt_tree_exact.h)
int qttt_tree_solve_leaves(void *tree, int64_t games, int64_t capacity, int leaves, const void *paths,
                           const void *leaf_state, int min_ply, float *leaf_value, uint8_t *leaf_exact, void *stream) {
    if (tree_size_bad(games, capacity) || tree_leaves_bad(games, leaves) || min_ply < QTTT_TREE_EXACT_MIN_PLY ||
        min_ply > QTTT_SOLVE_MAX_PLY)
        return QTTT_ERR_SIZE;
    if (games == 0) return 0;
    if (any_null(tree, paths, leaf_state)) return QTTT_ERR_NULL;
    if (misaligned(tree, 16) || misaligned(paths, 16) || misaligned(leaf_state, 16) || misaligned(leaf_value, 4))
        return QTTT_ERR_ACTION;
    const int64_t rows = games * leaves;
    const Planes l = planes(const_cast<void *>(leaf_state), rows);
    return chunked_launch(ceil_div(rows, SOLVE_LIST_RECORDS), [&](int64_t b0, int64_t grid) {     // a lane per record
        return launch(tree_solve_leaves_kernel, grid, SOLVE_BLOCK, stream, tree, games, capacity, (u32)leaves,
                      static_cast<const TreePathRec *>(paths), (const u64 *)l.P, (const u64 *)l.Q, b0 * SOLVE_LIST_RECORDS, rows,
                      min_ply, leaf_value, leaf_exact);
    });
}

int qttt_tree_backup_batch_exact(void *tree, int64_t games, int64_t capacity, int leaves, const void *paths,
                                 const float *leaf_value, const float *leaf_probs, void *stream) {
    return backup_batch<true>(tree, games, capacity, leaves, paths, leaf_value, leaf_probs, stream);
}

// ---------------------------------------------------------------- proven interior nodes (include/qttt_tree_prove.h)
int qttt_tree_prove(void *tree, int64_t games, int64_t capacity, int leaves, const void *paths, int32_t *proved,
                    void *stream) {
    if (tree_size_bad(games, capacity) || tree_leaves_bad(games, leaves)) return QTTT_ERR_SIZE;
    if (games == 0) return 0;
    if (any_null(tree, paths)) return QTTT_ERR_NULL;
    if (misaligned(tree, 16) || misaligned(paths, 16) || misaligned(proved, 4)) return QTTT_ERR_ACTION;
    return launch(tree_prove_kernel, ceil_div(games, TREE_GAMES_PER_BLOCK), TREE_BLOCK, stream, tree, games, capacity, (u32)leaves,
                  static_cast<const TreePathRec *>(paths), proved);
}

int qttt_tree_root_exact(const void *tree, int64_t games, int64_t capacity, float *q, uint8_t *proven, float *value,
                         uint8_t *solved, void *stream) {
    if (tree_size_bad(games, capacity)) return QTTT_ERR_SIZE;
    if (games == 0) return 0;
    if (!tree) return QTTT_ERR_NULL;
    if (misaligned(tree, 16) || misaligned(q, 4) || misaligned(value, 4)) return QTTT_ERR_ACTION;
    return launch(tree_root_exact_kernel, ceil_div(games, TREE_GAMES_PER_BLOCK), TREE_BLOCK, stream, tree, games, capacity, q,
                  proven, value, solved);
}

// ---------------------------------------------------------------- exact targets of a self-play batch (include/qttt_selfplay_exact.h)
int qttt_selfplay_exact_targets(const void *states, int64_t games, int min_ply, int policy, const uint8_t *rows,
                                const uint8_t *length, const uint8_t *done, const uint8_t *mask, double *pi, float *v,
                                uint8_t *exact, void *stream) {
    if (games < 0 || min_ply < QTTT_SELFPLAY_EXACT_MIN_PLY || min_ply > QTTT_SELFPLAY_EXACT_MAX_PLY || policy < 0 || policy > 1)
        return QTTT_ERR_SIZE;
    if (games == 0) return 0;
    if (any_null(states, length, done, mask) || any_null(pi, v)) return QTTT_ERR_NULL;
    if (misaligned(states, 16) || misaligned(pi, 8) || misaligned(v, 4)) return QTTT_ERR_ACTION;
    const ExactTargets o = {static_cast<const u64 *>(states), rows, length, done, pi, v, exact};
    const int64_t blocks = ceil_div((int64_t)QTTT_SELFPLAY_ROWS * games, SOLVE_LIST_RECORDS);
    return chunked_launch(blocks, [&](int64_t b0, int64_t grid) {                                 // a lane per record
        return launch(selfplay_exact_targets_kernel, grid, SOLVE_BLOCK, stream, o, games, b0 * SOLVE_LIST_RECORDS, min_ply, policy);
    });
}

// ---------------------------------------------------------------- reanalysis of the replay ring (include/qttt_replay_reanalyse.h)
int qttt_replay_gather(const void *replay, int64_t capacity, int64_t n, uint64_t seed, uint32_t draw, int64_t start,
                       void *state_out, int32_t *slot_out, int64_t *number_out, float *v_out, uint8_t *done_out,
                       void *stream) {
    bool work;
    if (const int rc = replay_gather_check(replay, capacity, n, draw, state_out, slot_out, number_out, v_out, work)) return rc;
    if (!work) return 0;
    const ReplayRing ring = replay_ring(const_cast<void *>(replay), capacity);
    return launch(replay_gather_kernel, ceil_div(plane_stride(n), REPLAY_GATHER_BLOCK), REPLAY_GATHER_BLOCK, stream, ring, capacity,
                  n, qttt_hash(seed, QTTT_REPLAY_WINDOW_ID, draw), start, static_cast<u64 *>(state_out), slot_out, number_out,
                  reinterpret_cast<u32 *>(v_out), done_out);
}

int qttt_replay_update(void *replay, int64_t capacity, int64_t n, const int32_t *slot, const int64_t *number,
                       const double *pi, const float *v, uint8_t *updated_out, void *stream) {
    bool work;
    if (const int rc = replay_update_check(replay, capacity, n, slot, number, pi, v, work)) return rc;
    if (!work) return 0;
    return launch(replay_update_kernel, ceil_div(n, REPLAY_UPDATE_SAMPLES), REPLAY_UPDATE_BLOCK, stream, replay_ring(replay, capacity),
                  capacity, n, slot, number, reinterpret_cast<const u64 *>(pi), reinterpret_cast<const u32 *>(v), updated_out);
}

// ---------------------------------------------------------------- prioritised replay (include/qttt_replay_priority.h)
int64_t qttt_replay_priority_bytes(int64_t capacity) {
    return replay_capacity_bad(capacity) ? (int64_t)QTTT_ERR_SIZE : priority_layout(capacity).bytes;
}

int qttt_replay_priority_layout(int64_t capacity, int64_t *offsets) {
    if (replay_capacity_bad(capacity)) return QTTT_ERR_SIZE;
    if (!offsets) return QTTT_ERR_NULL;
    const PriorityLayout l = priority_layout(capacity);
    for (int k = 0; k <= QTTT_PRIORITY_MAX_LEVELS; ++k) offsets[k] = k <= l.levels ? l.off[k] : 0;
    return l.levels;
}

// every sum level from the level below; ASSIGN and `seen`: the sync's first and last launch
static int priority_rebuild(bool assign, const u64 *ring_header, const PriorityTable &tab, int64_t capacity, void *stream) {
    u64 *seen = assign ? tab.header + PRIORITY_SEEN_WORD : nullptr;
    if (const int rc = with_bools([&](auto ASSIGN) {
            return launch(priority_sum0_kernel<ASSIGN>, tab.n[1], QTTT_REPLAY_SCAN_BLOCK, stream, ring_header, (const u64 *)tab.header,
                          tab.q, tab.sum[0], capacity, tab.levels == 1u ? seen : (u64 *)nullptr);
        }, assign))
        return rc;
    for (u32 k = 1; k < tab.levels; ++k)
        if (const int rc = launch(priority_sum_kernel, tab.n[k + 1], QTTT_REPLAY_SCAN_BLOCK, stream, ring_header,
                                  (const u64 *)tab.sum[k - 1], tab.sum[k], tab.n[k], k + 1u == tab.levels ? seen : (u64 *)nullptr))
            return rc;
    return 0;
}

int qttt_replay_priority_sync(const void *replay, void *prio, int64_t capacity, void *stream) {
    if (const int rc = priority_sync_check(replay, prio, capacity)) return rc;
    return priority_rebuild(true, static_cast<const u64 *>(replay), priority_table(prio, capacity), capacity, stream);
}

int qttt_replay_priority_update(const void *replay, void *prio, int64_t capacity, int64_t n, const int32_t *slot,
                                const int64_t *number, const float *priority, uint8_t *updated_out, void *stream) {
    bool work;
    if (const int rc = priority_update_check(replay, prio, capacity, n, slot, number, priority, work)) return rc;
    if (!work) return 0;
    const u64 *ring_header = static_cast<const u64 *>(replay);
    const PriorityTable tab = priority_table(prio, capacity);
    const int64_t groups = ceil_div(n, PRIORITY_UPDATE_BLOCK);
    if (const int rc = launch(priority_update_kernel<false>, groups, PRIORITY_UPDATE_BLOCK, stream, ring_header, tab, capacity, n, slot,
                              number, priority, updated_out))
        return rc;
    if (const int rc = launch(priority_update_kernel<true>, groups, PRIORITY_UPDATE_BLOCK, stream, ring_header, tab, capacity, n, slot,
                              number, priority, updated_out))
        return rc;
    return priority_rebuild(false, ring_header, tab, capacity, stream);
}

int qttt_replay_sample_prioritized(const void *replay, const void *prio, int64_t capacity, int64_t n, uint64_t seed,
                                   uint32_t draw, const uint8_t *sym, int random_symmetry, float *s_out, double *pi_out,
                                   uint8_t *mask_out, float *v_out, uint8_t *done_out, int32_t *index_out, uint8_t *sym_out,
                                   int64_t *number_out, uint32_t *q_out, uint64_t *total_out, void *stream) {
    bool work;
    if (const int rc = priority_sample_check(replay, prio, capacity, n, draw, s_out, pi_out, mask_out, v_out, done_out, index_out,
                                             number_out, q_out, total_out, work))
        return rc;
    if (!work) return 0;
    const ReplayRing ring = replay_ring(const_cast<void *>(replay), capacity);
    const PriorityTable tab = priority_table(const_cast<void *>(prio), capacity);
    const u64 key_slot = launch_key(seed, draw), key_sym = launch_key(seed, draw | 0x80000000u);
    return with_bools([&](auto SYM) {
        return launch(replay_sample_prioritized_kernel<SYM>, ceil_div(n, REPLAY_TILE), REPLAY_SAMPLE_BLOCK, stream, ring, tab, capacity,
                      n, key_slot, key_sym, sym, (u32)(random_symmetry != 0), s_out, reinterpret_cast<u64 *>(pi_out), mask_out,
                      reinterpret_cast<u32 *>(v_out), done_out, index_out, sym_out, number_out, q_out, reinterpret_cast<u64 *>(total_out));
    }, sym != nullptr || random_symmetry != 0);
}

// ---------------------------------------------------------------- search-value targets for self-play (include/qttt_selfplay_value.h)
int qttt_selfplay_record_value(const void *tree, int64_t games, int64_t capacity, int ply, const uint8_t *length, float *q,
                               const float *v, void *stream) {
    bool work;
    if (const int rc = value_record_check(tree, games, capacity, ply, length, q, v, work)) return rc;
    if (!work) return 0;
    return launch(selfplay_record_value_kernel, ceil_div(games, TREE_GAMES_PER_BLOCK), TREE_BLOCK, stream, tree, games, capacity,
                  ply, length, q, v);
}

int qttt_selfplay_value_targets(int64_t games, int mode, double lambda, const uint8_t *rows, const uint8_t *length,
                                const uint8_t *done, const uint8_t *exact, const float *q, float *v, void *stream) {
    bool work;
    if (const int rc = value_targets_check(games, mode, lambda, length, done, q, v, work)) return rc;
    if (!work) return 0;
    return launch(selfplay_value_targets_kernel, ceil_div(games, VALUE_TARGETS_BLOCK), VALUE_TARGETS_BLOCK, stream, games, mode,
                  lambda, rows, length, done, exact, q, v);
}

}  // extern "C"
