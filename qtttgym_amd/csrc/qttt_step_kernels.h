// qttt_step_kernels.h — the step kernels: lane per board, one launch per step (the metric's form), and the
// T-steps-in-registers forms (recorded actions / in-kernel policy).  The wave-per-board mapping study
// lives in tools/qttt_study.hip, outside the product library.
#ifndef QTTT_STEP_KERNELS_H
#define QTTT_STEP_KERNELS_H
#include "qttt_step_core.h"
#include "qttt_observation.h"

namespace {

// ====================================================================== the step kernels
// BPL boards per lane: lane j owns boards [j*BPL, (j+1)*BPL), so every plane is read and written
// with 16-byte vector accesses that are contiguous across the wave.  Addresses are a block-uniform
// 64-bit base (scalar unit) plus a 32-bit lane offset.
// SAMPLE: the action is not read but drawn in the kernel from the uniform-legal policy (and written to
// `actions` when that is not null) — qttt_sample_actions + qttt_step in one launch.
// OBS: Env.step returns the observation too (env.py:46,53): it is written from the registers the
// step already holds, through the LDS tiles above — qttt_step + qttt_observe in one launch.
// BLOCK, BPL: workgroup size and boards per lane, chosen by the host per launch from the batch size
// (auto_tuning() in qttt_kernels.hip holds the measured table: one board per lane in 256-thread
// workgroups below ~450 K boards, 1024-thread workgroups where they fill the chip exactly once,
// two boards per lane in 256-thread workgroups above 1 536 K boards).
// DEVSTEP: the step index lives on the DEVICE (qttt_env.step_counter, for launches captured in a hipGraph: the
// host cannot bake a step index into a node that is replayed).  key_hi then carries the node's offset, key_fold
// the fold of the ids' high word, and the launch key is made in the kernel (scalar unit, ~30 SALU instructions).
// A separate instantiation, so that the kernels of the ordinary path carry neither the two extra arguments nor
// the branch (measured: 2-3 % on a 1 M-board launch when they did).
//@isa lane
template <bool DEVSTEP> struct StepKeySource {};
template <> struct StepKeySource<true> {
    const u32 *ctr;
    u64 seed;
};

// OUT: reward and terminated are formed and stored.  Without it (step_quiet_kernel, below) the step moves the two planes
// only: 34 bytes per board instead of 39.
template <int BLOCK, int BPL, bool HAS_BITS, bool AUTO_RESET, bool SAMPLE, bool OBS, bool DEVSTEP, bool OUT>
__device__ __forceinline__ void step_body(
    u64 *__restrict__ pP, u64 *__restrict__ pQ, uint16_t *__restrict__ actions,
    const uint8_t *__restrict__ bits, u32 key_fold, u32 key_hi, u32 id_base,
    u32 *__restrict__ reward_bits, uint8_t *__restrict__ terminated, ObsOut obs, int64_t i_begin,
    u32 last_groups, StepKeySource<DEVSTEP> sk) {
    constexpr u32 TILE_BOARDS = BLOCK * BPL;
    __shared__ __attribute__((aligned(16))) uint8_t lut[LINE_LUT_BYTES];
    // the policy's tables: from 512 threads up qttt_state.h's PolicyRows (one word per empty-square mask + the
    // pre-scaled pair table, 692 words), in 256-thread workgroups — where that would be three table words per thread —
    // the two-level PolicyLut (146 words).  tools/stepbench STEPBENCH_RANDOM=1, interleaved, us per launch, round 3's
    // kernel / trusted step + two-level table / trusted step + rows: 1 M boards (2 x 1024) 8.06 / 7.79 / 7.66,
    // 768 K (2 x 512) 6.69 / 6.43 / 6.45, 2 M (2 x 256) 15.03 / 14.80 / 15.16, 256 K (1 x 256) 4.13 / 3.75 / 3.88.
    constexpr bool ROWS = SAMPLE && BLOCK >= 512;
    constexpr u32 PT_WORDS = ROWS ? POLICY_ROWS_WORDS : POLICY_LUT_WORDS;
    constexpr int PRW = SAMPLE ? (int)((PT_WORDS + BLOCK - 1) / BLOCK) : 1;
    __shared__ __attribute__((aligned(16))) u32 prows[SAMPLE ? PT_WORDS : 1];
    __shared__ __attribute__((aligned(16))) uint8_t otile[OBS ? obs_lds_bytes(TILE_BOARDS) : 16];
    __shared__ __attribute__((aligned(16))) u32 olut[OBS ? OBS_LUT_BYTES / 4 : 4];
#ifdef QTTT_DEBUG_STAMPS
    const u64 st0 = __builtin_amdgcn_s_memrealtime();
#endif
    typedef Vec<u64, BPL> V64;
    typedef Vec<u32, BPL> V32;
    typedef Vec<uint16_t, BPL> V16;
    typedef Vec<uint8_t, BPL> V8;
    if constexpr (DEVSTEP) {
        const u64 key = launch_key(sk.seed, key_hi + *sk.ctr);
        key_fold ^= (u32)key;
        key_hi = (u32)(key >> 32);
    }
    const int64_t jb = (int64_t)blockIdx.x * BLOCK;                // first lane-group of the block
    const int64_t ib = i_begin + jb * BPL;                              // first board of the block
    // lane-groups of this block: every block is full except possibly the last one of the grid
    const u32 ng = blockIdx.x + 1u == gridDim.x ? last_groups : (u32)BLOCK;
    const bool active = threadIdx.x < ng;
    const u32 g = active ? threadIdx.x : 0u;                            // idle lanes re-read group 0
    // The small tables that are LOADED (policy, observation) are requested first and stored after
    // the streaming loads have been issued: vector loads return in order, so the wait in front of
    // the table's LDS store then covers the table word only, not this wave's state.  The line table
    // is computed.  Either way the workgroup barrier is passed while the state is still in flight.
    u32 olw = 0;
    if (OBS && threadIdx.x < OBS_LUT_BYTES / 4) olw = (&g_obs_lut.sel[0][0])[threadIdx.x];
    u32 prw[PRW];
    if (SAMPLE) {
#pragma unroll
        for (int k = 0; k < PRW; ++k) {
            const u32 w = threadIdx.x + (u32)k * BLOCK;
            const u32 *src = ROWS ? reinterpret_cast<const u32 *>(&g_policy_rows) : reinterpret_cast<const u32 *>(&g_policy_lut);
            prw[k] = w < PT_WORDS ? src[w] : 0u;
        }
    }
    V64 p = load_stream(&reinterpret_cast<const V64 *>(pP + ib)[g]);
    V64 q = load_stream(&reinterpret_cast<const V64 *>(pQ + ib)[g]);
    V16 act;
    V8 bt;
    if (!SAMPLE) act = load_stream(&reinterpret_cast<const V16 *>(actions + ib)[g]);
    if (HAS_BITS) bt = load_stream(&reinterpret_cast<const V8 *>(bits + ib)[g]);
    fill_line_lut_nosync<BLOCK>(lut);
    if (OBS && threadIdx.x < OBS_LUT_BYTES / 4) olut[threadIdx.x] = olw;
    if (SAMPLE) {
#pragma unroll
        for (int k = 0; k < PRW; ++k) {
            const u32 w = threadIdx.x + (u32)k * BLOCK;
            if (w < PT_WORDS) prows[w] = prw[k];
        }
    }
    ObsTiles T;
    if (OBS) T = obs_tiles<TILE_BOARDS>(otile, obs, ib);
//@isa hash
    // The counter hash (collapse bit; with SAMPLE the policy's word too) depends on the board id and the launch key
    // only: it is computed HERE, while the state loads are in flight and the SIMD has nothing else to issue, and
    // pinned in registers (the empty asm) so that the compiler does not sink it back behind the loads' wait — 8
    // (SAMPLE: 16) VALU instructions per board off the critical path between "data landed" and "stores issued".
    const u32 id0 = id_base + ((u32)jb + g) * BPL;                      // low 32 bits of the global board id
    u32 hbit[BPL], hpol[BPL];
#pragma unroll
    for (int k = 0; k < BPL; ++k) {
        hbit[k] = hpol[k] = 0u;
        if (SAMPLE) {
            const u32 h1 = lowbias32((id0 + (u32)k) ^ key_fold);
            hpol[k] = lowbias32(h1 ^ key_hi);
            hbit[k] = h1 >> 31;
            asm volatile("" : "+v"(hbit[k]), "+v"(hpol[k]));
        } else if (!HAS_BITS) {
            hbit[k] = collapse_bit_of((id0 + (u32)k) ^ key_fold);
            asm volatile("" : "+v"(hbit[k]));
        }
    }
//@isa pack
    __syncthreads();
#ifdef QTTT_DEBUG_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const u64 st1 = __builtin_amdgcn_s_memrealtime();
#endif
    if (active) {
        V32 rw;
        V8 tm;
#pragma unroll
        for (int k = 0; k < BPL; ++k) {
            u32 P0 = (u32)p.v[k], P1 = (u32)(p.v[k] >> 32);
            u32 Q0 = (u32)q.v[k], Q1 = (u32)(q.v[k] >> 32);
            u32 bit, av, win;
            if (SAMPLE) {
                const u32 h2 = hpol[k];
                bit = hbit[k];
                if (AUTO_RESET) {
                    // a finished board restarts first (empty = all zero); a board that is not done has >= 2 empty
                    // squares (8 classical squares set the done bit), so the policy always finds a legal pair,
                    // lo < hi by construction: the step runs TRUSTED (no validation, no sorting), as in
                    // step_random_fused_kernel
                    step_auto_reset(P0, P1, Q0, Q1);
                    const u32 empty = ~(P1 >> P1_CL_SHIFT) & 0x1FFu;
                    av = ROWS ? policy_action_rows(prows, empty, h2) : policy_action(reinterpret_cast<const uint8_t *>(prows), empty, h2);
                    win = step_core<false, true>(P0, P1, Q0, Q1, av, bit, lut);
                } else {
                    // post-terminal legal moves are accepted; no legal pair -> (0,0), a noop
                    const u32 empty = ~(P1 >> P1_CL_SHIFT) & 0x1FFu;
                    av = !(empty & (empty - 1u)) ? 0u : ROWS ? policy_action_rows(prows, empty, h2)
                                                             : policy_action(reinterpret_cast<const uint8_t *>(prows), empty, h2);
                    win = step_core<false>(P0, P1, Q0, Q1, av, bit, lut);
                }
                act.v[k] = (uint16_t)av;
            } else {
                av = act.v[k];
                if (HAS_BITS) bit = bt.v[k] & 1u;
                else bit = hbit[k];
                win = step_core<AUTO_RESET>(P0, P1, Q0, Q1, av, bit, lut);
            }
            p.v[k] = (u64)P0 | ((u64)P1 << 32);
            q.v[k] = (u64)Q0 | ((u64)Q1 << 32);
            if (OUT) {
                rw.v[k] = 0x80000000u | (win << 23);                     // env.py:49: -1.0f / -0.0f
                tm.v[k] = (uint8_t)(P1 >> 31);
            }
            if (OBS) obs_board(P0, P1, Q0, T, g * BPL + (u32)k, olut);
        }
        store_stream_sbase(pP + ib, g * (u32)sizeof(V64), p);          // block-uniform base + 32-bit lane offset, like the loads
        store_stream_sbase(pQ + ib, g * (u32)sizeof(V64), q);
        if (SAMPLE && actions) store_stream(&reinterpret_cast<V16 *>(actions + ib)[g], act);
        if (OUT) {
            store_stream(&reinterpret_cast<V32 *>(reward_bits + ib)[g], rw);
            store_stream(&reinterpret_cast<V8 *>(terminated + ib)[g], tm);
        }
    }
    if (OBS) {
        // a wave's boards [64w * BPL, 64(w+1) * BPL) start on a multiple of 4 bytes in every tile
        const u32 ph = obs_all_phases(obs, ib, 15u);                 // block-uniform
        if ((ph & 3u) == 0u) {
            const u32 w0 = (threadIdx.x & ~63u) * BPL;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // rows written by other lanes of this wave
            __builtin_amdgcn_wave_barrier();
            if (w0 < ng * BPL) {
                if (ph == 0u) obs_wave_copy_out<TILE_BOARDS, true>(otile, obs, ib, w0, min(w0 + 64u * BPL, ng * BPL));
                else obs_wave_copy_out<TILE_BOARDS, false>(otile, obs, ib, w0, min(w0 + 64u * BPL, ng * BPL));
            }
        } else {
            __syncthreads();
            obs_copy_out<BLOCK, TILE_BOARDS>(otile, obs, ib, ng * BPL);
        }
    }
#ifdef QTTT_DEBUG_STAMPS
    const u64 st2 = __builtin_amdgcn_s_memrealtime();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const u64 st3 = __builtin_amdgcn_s_memrealtime();
    if (g_debug_stamps && (threadIdx.x & 63) == 0) {
        u64 *o = g_debug_stamps + ((int64_t)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6)) * 4;
        o[0] = st0; o[1] = st1; o[2] = st2; o[3] = st3;
    }
#endif
}

template <int BLOCK, int BPL, bool HAS_BITS, bool AUTO_RESET, bool SAMPLE = false, bool OBS = false, bool DEVSTEP = false>
__global__ __launch_bounds__(BLOCK) void step_kernel(
    u64 *__restrict__ pP, u64 *__restrict__ pQ, uint16_t *__restrict__ actions,
    const uint8_t *__restrict__ bits, u32 key_fold, u32 key_hi, u32 id_base,
    u32 *__restrict__ reward_bits, uint8_t *__restrict__ terminated, ObsOut obs, int64_t i_begin,
    u32 last_groups, StepKeySource<DEVSTEP> sk) {
    step_body<BLOCK, BPL, HAS_BITS, AUTO_RESET, SAMPLE, OBS, DEVSTEP, true>(
        pP, pQ, actions, bits, key_fold, key_hi, id_base, reward_bits, terminated, obs, i_begin, last_groups, sk);
}

// The plain step (recorded actions; no policy, no observation, host-side step index) WITHOUT its outputs: the launches
// of qttt_step_many whose reward / terminated the next launch overwrites (out_stride == 0, every step but the last).
// A kernel of its own rather than a null-pointer test in step_kernel (see DEVSTEP above on what extra arguments and a
// branch cost the ordinary kernel).  The launch key's high word is not needed: only the policy and DEVSTEP read it.
template <int BLOCK, int BPL, bool HAS_BITS, bool AUTO_RESET>
__global__ __launch_bounds__(BLOCK) void step_quiet_kernel(
    u64 *__restrict__ pP, u64 *__restrict__ pQ, const uint16_t *__restrict__ actions,
    const uint8_t *__restrict__ bits, u32 key_fold, u32 id_base, int64_t i_begin, u32 last_groups) {
    step_body<BLOCK, BPL, HAS_BITS, AUTO_RESET, false, false, false, false>(
        pP, pQ, const_cast<uint16_t *>(actions), bits, key_fold, 0u, id_base, nullptr, nullptr,
        ObsOut{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}, i_begin, last_groups, StepKeySource<false>{});
}

//@isa lane
// T consecutive steps in ONE launch (qttt_step_many with QTTT_FLAG_FUSED): the boards stay in
// registers, only the per-step streams move (2 B action in, 5 B reward/terminated out per step), so
// the loop is VALU-bound and pays one launch instead of T.  Same results as T launches of
// step_kernel; meant for replay / evaluation where the actions are known up front (a policy that
// looks at the state between steps needs the one-launch-per-step form).
// The launch keys of the plies come from the host as a kernel argument (FusedKeys, at most FUSED_MAX_PLIES per launch; the
// library splits longer runs): splitmix64 per ply on the scalar unit was 25 of the loop's 86 scalar instructions — measured:
// 3.57 -> 3.44 us per ply at 1 M boards, 1.19 -> 1.10 at 262 144 (profiles/r05/fused_kernarg_keys_check.txt).
constexpr int FUSED_MAX_PLIES = 64;
struct FusedKeys { u64 k[FUSED_MAX_PLIES]; };
// OUT — which plies' reward / terminated a launch stores:
//   FUSED_OUT_EVERY  every ply's (out_stride != 0), from inside the loop: the kernel below, FUSED_MAX_PLIES per launch;
//   FUSED_OUT_LAST   its last ply's only (out_stride == 0, the last launch of a run): formed from `win` and P1 AFTER the
//                    loop and stored once, beside the two planes;
//   FUSED_OUT_NONE   none (out_stride == 0, the earlier launches of a run longer than one launch: the run's last
//                    launch overwrites whatever they would store; they are handed no output pointers).
// LAST and NONE are the output-free kernel further down (the overload with a ply cap and a workgroup size of its own).
constexpr int FUSED_OUT_NONE = 0, FUSED_OUT_LAST = 1, FUSED_OUT_EVERY = 2;
template <bool HAS_BITS, bool AUTO_RESET, int OUT>
__global__ __launch_bounds__(QTTT_BLOCK) void step_fused_kernel(
    u64 *__restrict__ pP, u64 *__restrict__ pQ, const uint16_t *__restrict__ actions,
    const uint8_t *__restrict__ bits, FusedKeys keys, u32 id_hi_fold, u32 id_base,
    u32 *__restrict__ reward_bits, uint8_t *__restrict__ terminated, int64_t out_stride, int64_t n,
    int32_t n_steps) {
    static_assert(OUT == FUSED_OUT_EVERY, "the output-free forms are the overload below");
    __shared__ __attribute__((aligned(16))) uint8_t lut[LINE_LUT_BYTES];
    const int64_t ib = (int64_t)blockIdx.x * QTTT_BLOCK;            // first board of the workgroup (block-uniform)
    const int64_t i = ib + threadIdx.x;
    const int64_t il = i < n ? i : 0;                               // idle lanes re-read board 0, store nothing
    const u64 P = load_stream(&pP[il]), Q = load_stream(&pQ[il]);   // requested before the table fills
    fill_line_lut<QTTT_BLOCK>(lut);
    if (i >= n) return;
    u32 P0 = (u32)P, P1 = (u32)(P >> 32), Q0 = (u32)Q, Q1 = (u32)(Q >> 32);
    const u32 id = (id_base + (u32)i) ^ id_hi_fold;
    // per-ply streams: a block-uniform 64-bit base (scalar unit, advanced by the stride every ply) plus the lane's offset
    const uint16_t *a_blk = actions + ib;
    const uint8_t *b_blk = HAS_BITS ? bits + ib : nullptr;
    const u32 lane = threadIdx.x;
    u32 win = 0;
    u64 key = keys.k[0];
    u32 *r_blk = reward_bits + ib;
    uint8_t *t_blk = terminated + ib;
    u32 act = load_stream(&a_blk[lane]), bit_in = HAS_BITS ? (u32)load_stream(&b_blk[lane]) : 0u;
    for (int32_t t = 0; t < n_steps; ++t) {
        const u64 key_next = keys.k[(t + 1) & (FUSED_MAX_PLIES - 1)];   // one scalar load, requested a ply ahead
        // the next ply's action (and bit) are requested before this ply's step: their latency hides behind it
        const bool more = t + 1 < n_steps;
        a_blk += more ? n : 0;
        if (HAS_BITS) b_blk += more ? n : 0;
        const u32 act_next = load_stream(&a_blk[lane]), bit_next = HAS_BITS ? (u32)load_stream(&b_blk[lane]) : 0u;
        const u32 bit = HAS_BITS ? (bit_in & 1u) : collapse_bit_of(id ^ (u32)key);
        win = step_core<AUTO_RESET>(P0, P1, Q0, Q1, act, bit, lut);
        if (out_stride != 0 || t == n_steps - 1) {
            // (the compiler's own stores here: it counts them when it waits for the action requested a ply ahead)
            store_stream(&r_blk[lane], 0x80000000u | (win << 23));
            store_stream(&t_blk[lane], (uint8_t)(P1 >> 31));
        }
        r_blk += out_stride;
        t_blk += out_stride;
        key = key_next;
        act = act_next;
        bit_in = bit_next;
    }
    store_stream(&pP[i], (u64)P0 | ((u64)P1 << 32));
    store_stream(&pQ[i], (u64)Q0 | ((u64)Q1 << 32));
}

// The output-free forms (FUSED_OUT_LAST / FUSED_OUT_NONE: qttt_step_many with out_stride == 0, asked for or by the route of
// the one-round rows).  Without per-ply outputs the loop holds no store, no output pointer and no test of what to keep, and
// nothing couples the action stream to a store queue: the actions are requested FUSED_PREFETCH plies ahead instead of one
// (the stream of a long replay comes from HBM, not from the Infinity Cache), and the state is consumed in front of the loop
// (as in step_random_fused_kernel below) so that the wait for its loads does not land inside.
// (tools/stepbench, interleaved, 1 M boards, us per step with 1 / 2 / 4 plies ahead: 3.29 / 3.27 / 3.29 at K = 200,
// 3.46 / 3.43 / 3.47 at K = 20 — within the spread of the repeats; profiles/resident/stepbench_1M_k*.txt)
constexpr int FUSED_PREFETCH = 2;
// CAP — the plies one launch takes, the size of its keys argument (ResidentKeys<CAP>, 8 B per ply; the kernel arguments
// stay within 4 KB).  A launch costs the kernel boundary, the wave ramp, the table fill behind the workgroup's barrier, the
// state's round trip and the drain of the second occupancy round, and nothing in the result needs any of it; with no
// per-ply outputs only the keys argument bounds a launch.  RESIDENT_MAX_PLIES is the product's CAP: the smallest within
// the spread of the best.  tools/stepbench 1048576 K 15 parent.so this.so resident:CAP:512 ..., interleaved, us per step,
// median (min) (profiles/resident_long/stepbench_cap_and_block.txt):
//   plies per launch      64            128           256           448
//   K = 1000              3.14 (3.09)   3.07 (3.06)   3.04 (3.03)   3.05 (3.04)     a launch costs (3.14 - 3.04) x 1000 / 12 = 8 us
//   K = 200               3.26 (3.22)   3.20 (3.13)   3.18 (3.11)   3.18 (3.14)
//   K = 20                3.47 (3.42)   -             3.48 (3.41)   -               one launch either way
// BLOCK — threads per workgroup (RESIDENT_BLOCK in the product).  The same tool, K = 200, CAP = 256, median (min):
//   boards        256           512           1024
//   458 816       1.68 (1.66)   1.74 (1.70)   1.72 (1.70)
//   786 432       2.47 (2.43)   2.48 (2.43)   2.47 (2.45)
//   1 048 576     3.18 (3.15)   3.20 (3.14)   3.20 (3.14)
//   1 572 864     4.67 (4.62)   4.67 (4.60)   4.68 (4.60)
// 512 stays: from 786 432 boards on the three are within the spread of the repeats (0.03 - 0.07 between a variant's min and
// median); 256 threads are 0.04 - 0.06 ahead at the window's first size only, one spread, and a second instantiation for
// that edge was not taken.
// The ply — ResidentBoard (qttt_step_core.h): the loop runs on a form of the board of its own, unpacked in front of it and
// packed behind it.  tools/isa_budget.py '<this kernel>' 1 --loop: 118.8 -> 113.8 VALU, 164.2 -> 157.6 ns of issue per
// wave-ply; SQ_INSTS_VALU per board-ply 121.7 -> 116.8.  tools/stepbench 1048576 K 15, every variant its own library,
// interleaved, us per step, median (min), the parent 3.06 (3.04) at K = 1000 and 3.46 (3.37) at K = 20
// (profiles/resident_diet/stepbench_candidates.txt):
//   kept     "done" as a lane mask, the lookups kept apart, the reward formed behind the loop: alone 3.06 (3.04) / 3.48 (3.38)
//   kept     SDWA byte selects in the decode, one compare for "lo != hi and neither is classical": alone 3.05 (3.01) / 3.43 (3.34)
//   kept     comps' high nibble and the classical mask in registers of their own, `last x` by one v_bitop3: alone 3.02 (2.99) / 3.46 (3.38)
//            the three together 2.89 (2.88) / 3.32 (3.23): more than their sum (the body without any of them: 3.04 / 3.49)
//   dropped  SLOT_LSB, the `last x` mask and the classical mask's bit pinned in VGPRs (their v_bitop3 fast-class, -0.7 ns in the
//            model): alone 3.06 (3.04) / 3.47 (3.43), on top of the three 2.92 (2.91) / 3.34 (3.24): not faster
//   dropped  the action as a 16-bit operand (no v_and 0xffff): the compiler packs two plies' actions into one register and
//            pays a v_alignbit to rotate them; by the model +0.7 ns, not run
//   dropped  the slots / qstructs / lookups as pieces shared with step_core: the other kernels' instruction streams reorder
//   not tried: the walk's cost per node, the classical mask "times four" (the one compare above needs it above x16)
// The decode — the action table (qttt_step_core.h, action_lut_entry): lo, hi, x16 and the two-square mask of ply t + 1 come
// from ONE ds_read_b128, requested by ply t behind its line test's two lookups (they are waited for before it is issued: their
// wait is what it was) and looked at first in ply t + 1's decode.  What is left per ply: the index (v_lshl_or, v_and), z (one
// v_bitop3 that meets the action's high nibbles as well), the one compare, pm's shift.  isa_budget, the loop: decode 9.0 -> 5.0
// VALU = 14.3 -> 6.6 ns, in all 113.8 -> 108.8 VALU = 157.6 -> 148.9 ns per wave-ply (the v_and 0xffff of the action's zero
// extension went too); SQ_INSTS_VALU per board-ply 116.76 -> 111.80; LDS 2 -> 6 KB, still 8 waves per SIMD.  Predicted
// 8.7 ns x 16 waves = 0.14 us per step.  Measured (profiles/resident_decode/), bench.py, parent / this tree alternately, five runs
// each, two sessions: K = 1000 medians 2.886 -> 2.787 and 2.911 -> 2.815 us, every run of this tree below every run of the
// parent in both; the gain, 0.100 and 0.096, is 2.4 x and 3.4 x the parent's max - min of its session (0.042, 0.029): the margin
// of three spreads is met in the second session and missed in the first, whose parent runs scatter further than in any session
// before (0.013 - 0.026).  K = 20: 3.776 -> 3.720 and 3.776 -> 3.730 (the parent's max - min 0.12, 0.14).  tools/stepbench interleaved,
// median (min): 2.95 (2.92) -> 2.88 (2.83) at K = 1000, 3.31 (3.24) -> 3.22 (3.14) at K = 20.  0.020 us per VALU taken out,
// the low end of the model's 0.016 - 0.028: the wait for the entry at the top of the ply is a wait for the key's scalar load
// too (scalar loads answer out of order, so the count is 0), seven instructions behind its request where it had a whole ply.
//   kept     the entry's four words as they are consumed: lo and hi clean (the rooting rule multiplies them by four), hi as the
//            validity mark (0 in an entry that is not two distinct squares below 9), pmS | 0xF0F0 as one or-and operand
//   dropped  the entry requested at the top of ply t (a whole ply ahead): it is live beside ply t's own, two v_mov_b64 per ply
//            hand it over (by the model + 3.5 ns), and left to itself the compiler merges the two requests into one read at
//            the top of the ply that consumes it; not run
//   dropped  the index as one v_bitop3 with the mask 0xFF0: the mask travels in an SGPR (slow class), + 0.7 ns; not run
//   dropped  the key's scalar load requested behind the ply: its destination is a register the loop's head writes, so the wait
//            moves to the loop's first instruction, in front of the action's load; not run
//   LDS      the pipe serves 3 instead of 2 reads per wave-ply; the read's latency and its bank conflicts (64 lanes, 72 live
//            entries of 16 bytes) were not counted on their own: what shows is the whole, 740 - 744 -> 727 - 728 us per dispatch
//            of 256 plies under the profiler, two thirds of the model's gain
constexpr int RESIDENT_MAX_PLIES = 256;
constexpr int RESIDENT_BLOCK = QTTT_BLOCK;
template <int CAP>
struct ResidentKeys { u64 k[CAP]; };
template <bool HAS_BITS, bool AUTO_RESET, int OUT, int CAP, int BLOCK>
__global__ __launch_bounds__(BLOCK) void step_fused_kernel(
    u64 *__restrict__ pP, u64 *__restrict__ pQ, const uint16_t *__restrict__ actions,
    const uint8_t *__restrict__ bits, ResidentKeys<CAP> keys, u32 id_hi_fold, u32 id_base,
    u32 *__restrict__ reward_bits, uint8_t *__restrict__ terminated, int64_t n, int32_t n_steps) {
    static_assert(OUT == FUSED_OUT_LAST || OUT == FUSED_OUT_NONE, "every ply's outputs: the kernel above");
    static_assert(sizeof(ResidentKeys<CAP>) + 64 + 256 <= 4096, "4 KB of kernel arguments, the hidden ones included");
    static_assert(FUSED_PREFETCH >= 2, "the entry of ply t + 1 is requested from act[1] while ply t runs");
    __shared__ __attribute__((aligned(16))) uint8_t lut[LINE_LUT_BYTES];
    __shared__ __attribute__((aligned(16))) uint8_t atab[ACTION_LUT_BYTES];
    const int64_t ib = (int64_t)blockIdx.x * BLOCK;                 // first board of the workgroup (block-uniform)
    const int64_t i = ib + threadIdx.x;
    const int64_t il = i < n ? i : 0;                               // idle lanes re-read board 0, store nothing
    const u64 P = load_stream(&pP[il]), Q = load_stream(&pQ[il]);   // requested before the tables fill
    fill_action_lut_nosync<BLOCK>(atab);
    fill_line_lut<BLOCK>(lut);                                      // ends with the workgroup barrier
    if (i >= n) return;
    u32 P0 = (u32)P, P1 = (u32)(P >> 32), Q0 = (u32)Q, Q1 = (u32)(Q >> 32);
    const u32 id = (id_base + (u32)i) ^ id_hi_fold;
    // per-ply streams: a block-uniform 64-bit base (scalar unit, advanced by the stride every ply) plus the lane's offset
    const uint16_t *a_blk = actions + ib;
    const uint8_t *b_blk = HAS_BITS ? bits + ib : nullptr;
    const u32 lane = threadIdx.x;
    u32 win = 0;
    u64 key = keys.k[0];
    // the actions (and bits) of plies 0 .. FUSED_PREFETCH - 1 are in flight before the first step; a ply past the
    // launch's last re-reads the last one's (the base stops advancing), so every address stays inside the run — and so
    // does every action an entry of the action table is requested for
    u32 act[FUSED_PREFETCH], bit_in[FUSED_PREFETCH];
#pragma unroll
    for (int k = 0; k < FUSED_PREFETCH; ++k) {
        if (k > 0) {
            const bool more = k < n_steps;
            a_blk += more ? n : 0;
            if (HAS_BITS) b_blk += more ? n : 0;
        }
        act[k] = load_stream(&a_blk[lane]);
        bit_in[k] = HAS_BITS ? (u32)load_stream(&b_blk[lane]) : 0u;
    }
    ResidentBoard<AUTO_RESET> board;
    board.unpack(P0, P1, Q0, Q1);                                   // (consumes the state in front of the loop)
    // the decoded action travels a ply ahead of the board: ply 0's entry is requested here, ply t + 1's while ply t runs
    u32x4 entry = action_lut_read(atab, act[0]);
    for (int32_t t = 0; t < n_steps; ++t) {
        // one scalar load, requested a ply ahead; the index wraps at CAP (a mask where CAP is a power of two)
        const u64 key_next = keys.k[(CAP & (CAP - 1)) == 0 ? (t + 1) & (CAP - 1) : t + 1 < CAP ? t + 1 : 0];
        const bool more = t + FUSED_PREFETCH < n_steps;
        a_blk += more ? n : 0;
        if (HAS_BITS) b_blk += more ? n : 0;
        const u32 act_far = load_stream(&a_blk[lane]), bit_far = HAS_BITS ? (u32)load_stream(&b_blk[lane]) : 0u;
        const u32 bit = HAS_BITS ? (bit_in[0] & 1u) : collapse_bit_of(id ^ (u32)key);
        board.ply(entry, act[0], act[1], bit, lut, atab);
        key = key_next;
#pragma unroll
        for (int k = 0; k + 1 < FUSED_PREFETCH; ++k) {
            act[k] = act[k + 1];
            bit_in[k] = bit_in[k + 1];
        }
        act[FUSED_PREFETCH - 1] = act_far;
        bit_in[FUSED_PREFETCH - 1] = bit_far;
    }
    board.pack(P0, P1, Q0, Q1, win);
    if constexpr (OUT == FUSED_OUT_LAST) {
        store_stream(&reward_bits[i], 0x80000000u | (win << 23));   // env.py:49: -1.0f / -0.0f
        store_stream(&terminated[i], (uint8_t)(P1 >> 31));          // env.py:51
    }
    store_stream(&pP[i], (u64)P0 | ((u64)P1 << 32));
    store_stream(&pQ[i], (u64)Q0 | ((u64)Q1 << 32));
}

// The same with the uniform-legal policy IN the kernel (qttt_step_random_many): T consecutive
// qttt_step_random steps — policy -> collapse bit -> step, ply t keyed by the counter hash of
// (seed, global board id, step_idx0 + t) exactly as the launch-by-launch form — with the boards in
// registers.  This is MCTS._simulate's loop (mcts.py:185-198: policy -> step until terminal) turned
// into the env's throughput mode: with AUTO_RESET a finished board restarts on its next ply, so every
// ply of every lane is a live transition.  Per ply it moves only what the caller keeps (nothing, or
// action 2 B + reward 4 B + terminated 1 B per board), so it is VALU-bound and pays one launch per T
// steps: this is what takes batches of <= 512 K boards (BASELINE configs 2-4: one partial occupancy
// round per launch) out of the launch-bound regime.
//   nth9 / policy_action_nth9: qttt_state.h (the full 4.5 KB "r-th empty square" table, computed by the workgroup).
// With AUTO_RESET the policy always has a legal pair (a board that is not done has >= 2 empty squares:
// 8 classical squares set the done bit), so the step runs TRUSTED (no validation, no sorting).
// KEEP: every ply's action, reward and terminated are kept (out_stride != 0, no null output) — the loop then carries no
// test of what to store.
template <int BLOCK, bool AUTO_RESET, bool RETURNS = false, bool KEEP = false>
__global__ __launch_bounds__(BLOCK) void step_random_fused_kernel(
    u64 *__restrict__ pP, u64 *__restrict__ pQ, FusedKeys keys, u64 board_offset,
    uint16_t *__restrict__ actions_out, u32 *__restrict__ reward_bits, uint8_t *__restrict__ terminated,
    int64_t out_stride, int64_t n, int32_t n_steps, float *__restrict__ returns) {
    __shared__ __attribute__((aligned(16))) uint8_t lut[LINE_LUT_BYTES];
    __shared__ __attribute__((aligned(16))) uint8_t plut[POLICY_LUT_WORDS * 4];
    __shared__ uint8_t nth9[NTH9_BYTES];
    const int64_t ib = (int64_t)blockIdx.x * BLOCK;                 // first board of the workgroup (block-uniform)
    const int64_t i = ib + threadIdx.x;
    const bool active = i < n;
    const int64_t il = active ? i : 0;                              // idle lanes re-read board 0, store nothing
    const u64 P = load_stream(&pP[il]), Q = load_stream(&pQ[il]);   // requested before the table fills
    fill_policy_lut<BLOCK>(plut);
    fill_nth9<BLOCK>(nth9);
    fill_line_lut<BLOCK>(lut);                                      // ends with the workgroup barrier
    if (!active) return;
    u32 P0 = (u32)P, P1 = (u32)(P >> 32), Q0 = (u32)Q, Q1 = (u32)(Q >> 32);
    const u32 id = fold_id(board_offset + (u64)i);
    // per-ply outputs: a block-uniform 64-bit base (scalar unit, advanced by the stride every ply) plus the
    // lane's 32-bit offset — no 64-bit vector address arithmetic in the loop
    uint16_t *a_blk = actions_out ? actions_out + ib : nullptr;
    u32 *r_blk = reward_bits ? reward_bits + ib : nullptr;
    uint8_t *t_blk = terminated ? terminated + ib : nullptr;
    const int64_t a_step = actions_out ? out_stride : 0, r_step = reward_bits ? out_stride : 0;   // a null output stays null
    const u32 lane = threadIdx.x;
    u32 lines = 0;                                                  // plies whose reward was -1.0 (env.py:49): -(the return)
    u64 key = keys.k[0];
    // The state is consumed HERE, in front of the loop: the per-ply stores below are written out (store_stream_sbase_word),
    // so the compiler sees no memory operation in the loop and would leave its wait for the state loads inside it — where
    // a vmcnt wait also waits for the previous ply's stores (+9 % per ply with one wave per SIMD).
    asm volatile("" : "+v"(P0), "+v"(P1), "+v"(Q0), "+v"(Q1));
    for (int32_t t = 0; t < n_steps; ++t) {
        const u64 key_next = keys.k[(t + 1) & (FUSED_MAX_PLIES - 1)];   // one scalar load, requested a ply ahead
        const u32 h1 = lowbias32(id ^ (u32)key);
        const u32 h2 = lowbias32(h1 ^ (u32)(key >> 32));
        u32 act, win;
        if (AUTO_RESET) {
            step_auto_reset(P0, P1, Q0, Q1);                        // a finished board restarts: empty = all zero
            const u32 empty = ~(P1 >> P1_CL_SHIFT) & 0x1FFu;        // >= 2 squares: the board is not done
            act = policy_action_nth9(plut, nth9, empty, h2);
            win = step_core<false, true>(P0, P1, Q0, Q1, act, h1 >> 31, lut);
        } else {
            // post-terminal legal moves are accepted; no legal pair -> (0,0), a noop
            const u32 empty = ~(P1 >> P1_CL_SHIFT) & 0x1FFu;
            act = (empty & (empty - 1u)) ? policy_action_nth9(plut, nth9, empty, h2) : 0u;
            win = step_core<false, false>(P0, P1, Q0, Q1, act, h1 >> 31, lut);
        }
        if (KEEP || out_stride != 0 || t == n_steps - 1) {
            if (KEEP || a_blk) store_stream_sbase_word<2>(a_blk, lane * 2u, act);
            if (KEEP || r_blk) {
                store_stream_sbase_word<4>(r_blk, lane * 4u, 0x80000000u | (win << 23));   // env.py:49: -1.0f / -0.0f
                store_stream_sbase_word<1>(t_blk, lane, P1 >> 31);                          // env.py:51
            }
        }
        if (RETURNS) lines += win & 1u;                             // (its own instantiation: the ordinary ply carries nothing extra)
        a_blk += a_step;
        r_blk += r_step;
        t_blk += r_step;
        key = key_next;
    }
    if (RETURNS) returns[i] -= (float)lines;                        // the sum of the rewards of these plies, accumulated
    store_stream(&pP[i], (u64)P0 | ((u64)P1 << 32));
    store_stream(&pQ[i], (u64)Q0 | ((u64)Q1 << 32));
}

}  // namespace

#endif  // QTTT_STEP_KERNELS_H
