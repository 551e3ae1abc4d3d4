// qttt_replay_priority_kernels.h — prioritised replay on the device (include/qttt_replay_priority.h): the
// sum launches that sync and update share, the two launches of the guarded write-back, and the one launch of the
// prioritised draw: a wavefront descends the sum levels for a sample (64 lanes x 4 children, a wave-wide inclusive scan in
// u64 by __shfl_up, a ballot for the first lane past t), four samples of a wave in lock step so that their loads overlap;
// then the workgroup builds and streams the rows with qttt_replay_kernels.h's own row functions.  Every sum is an integer:
// no result depends on the order of anything.  The only atomics are atomicMax on u32.
#ifndef QTTT_REPLAY_PRIORITY_KERNELS_H
#define QTTT_REPLAY_PRIORITY_KERNELS_H
#include "qttt_replay_kernels.h"
#include "qttt_replay_priority_host.h"

namespace {

// the table's arrays (qttt_replay_priority_layout), as the kernels take them
struct PriorityTable {
    u64 *header;                                                 // word 0: seen; u32 word 2: pmax
    u32 *q;
    u64 *sum[QTTT_PRIORITY_MAX_LEVELS];                          // sum[k - 1] = level k
    int64_t n[QTTT_PRIORITY_MAX_LEVELS + 1];
    u32 levels;
};
inline PriorityTable priority_table(void *prio, int64_t capacity) {
    const PriorityLayout l = priority_layout(capacity);
    uint8_t *b = static_cast<uint8_t *>(prio);
    PriorityTable t = {};
    t.header = reinterpret_cast<u64 *>(b);
    t.q = reinterpret_cast<u32 *>(b + l.off[0]);
    for (int k = 1; k <= l.levels; ++k) t.sum[k - 1] = reinterpret_cast<u64 *>(b + l.off[k]);
    for (int k = 0; k <= l.levels; ++k) t.n[k] = l.n[k];
    t.levels = (u32)l.levels;
    return t;
}

// the sum of x over the workgroup's SCAN_BLOCK lanes, in every lane (wave butterflies, then the four wave totals)
__device__ __forceinline__ u64 priority_block_sum(u64 x, u64 *wave_tot) {
#pragma unroll
    for (u32 d = 32u; d > 0u; d >>= 1) x += __shfl_xor(x, (int)d, 64);
    if ((threadIdx.x & 63u) == 0u) wave_tot[threadIdx.x >> 6] = x;
    __syncthreads();
    u64 all = 0;
#pragma unroll
    for (u32 w = 0; w < (u32)(QTTT_REPLAY_SCAN_BLOCK / 64); ++w) all += wave_tot[w];
    return all;
}

// Level 0 -> level 1: a workgroup sums SCAN_BLOCK priorities.  ASSIGN (sync): a slot whose sample has no priority yet gets
// pmax first.  seen_out (nullable; given to the launch that makes the top total, which is a single workgroup): seen =
// written, stored after the workgroup's barrier, so after every lane of the launch has read `seen`.
template <bool ASSIGN>
__global__ __launch_bounds__(QTTT_REPLAY_SCAN_BLOCK) void priority_sum0_kernel(const u64 *ring_header, const u64 *tab_header, u32 *q,
                                                                               u64 *sums, int64_t capacity, u64 *seen_out) {
    __shared__ u64 wave_tot[QTTT_REPLAY_SCAN_BLOCK / 64];
    const int64_t i = priority_child((int64_t)blockIdx.x, threadIdx.x);
    const u64 written = ring_header[0];
    u64 x = 0;
    if (i < capacity) {
        x = q[i];
        if constexpr (ASSIGN) {
            const u64 seen = tab_header[PRIORITY_SEEN_WORD];
            if (priority_slot_is_new((u64)i, seen, written, (u64)capacity)) {
                const u32 p = priority_pmax(reinterpret_cast<const u32 *>(tab_header)[PRIORITY_PMAX_WORD]);
                q[i] = p;
                x = p;
            }
        }
    }
    const u64 all = priority_block_sum(x, wave_tot);
    if (threadIdx.x == 0u) {
        sums[blockIdx.x] = all;
        if (seen_out) *seen_out = written;
    }
}

// Level k -> level k + 1, k >= 1.
__global__ __launch_bounds__(QTTT_REPLAY_SCAN_BLOCK) void priority_sum_kernel(const u64 *ring_header, const u64 *in, u64 *sums, int64_t n,
                                                                              u64 *seen_out) {
    __shared__ u64 wave_tot[QTTT_REPLAY_SCAN_BLOCK / 64];
    const int64_t i = priority_child((int64_t)blockIdx.x, threadIdx.x);
    const u64 all = priority_block_sum(i < n ? in[i] : 0ull, wave_tot);
    if (threadIdx.x == 0u) {
        sums[blockIdx.x] = all;
        if (seen_out) *seen_out = ring_header[0];
    }
}

// The write-back, a lane per entry.  First launch (RAISE = false): every passing entry clears its slot (all store the same
// 0).  Second launch: every passing entry raises its slot to its Q with atomicMax, so the slot ends at the largest of them;
// a wave's largest stored value goes to pmax, never below QTTT_PRIORITY_ONE (what 0 reads as).
constexpr int PRIORITY_UPDATE_BLOCK = 256;
template <bool RAISE>
__global__ __launch_bounds__(PRIORITY_UPDATE_BLOCK) void priority_update_kernel(const u64 *ring_header, PriorityTable tab, int64_t capacity,
                                                                                int64_t n, const int32_t *slot, const int64_t *number,
                                                                                const float *priority, uint8_t *updated_out) {
    const int64_t i = (int64_t)blockIdx.x * PRIORITY_UPDATE_BLOCK + threadIdx.x;
    u32 stored = 0;
    if (i < n) {
        const int32_t s = slot[i];
        const bool pass = priority_entry_passes(s, number[i], tab.header[PRIORITY_SEEN_WORD], ring_header[0], (u64)capacity);
        if constexpr (RAISE) {
            if (pass) {
                stored = priority_quantise(priority[i]);
                atomicMax(&tab.q[s], stored);
            }
            if (updated_out) updated_out[i] = pass ? 1 : 0;
        } else {
            if (pass) tab.q[s] = 0u;
        }
    }
    if constexpr (RAISE) {
#pragma unroll
        for (u32 d = 32u; d > 0u; d >>= 1) stored = max(stored, (u32)__shfl_xor((int)stored, (int)d, 64));
        if ((threadIdx.x & 63u) == 0u && stored != 0u)
            atomicMax(reinterpret_cast<u32 *>(tab.header) + PRIORITY_PMAX_WORD, max(stored, (u32)QTTT_PRIORITY_ONE));
    }
}

// ---- the descent.  A wave holds up to PRIORITY_WAVE_SAMPLES samples; for each, `idx` is the entry of the current level
// it stands on and `t` what is left of its draw inside that entry (t < the entry's sum, in a table that is in sync).  One
// step: lane l takes the children 4 l .. 4 l + 3 of the entry's block (those past the level's end count 0), the wave scans
// the lanes' sums, the ballot finds the first lane whose running sum passes t, and that lane's own four children finish
// the step.  The new index is clamped to the level, so a table out of sync draws a wrong slot, never an address outside.
constexpr u32 PRIORITY_WAVE_SAMPLES = REPLAY_TILE / (REPLAY_SAMPLE_BLOCK / 64);
static_assert(QTTT_REPLAY_SCAN_BLOCK == 4 * 64, "a wave takes a block of children four per lane");

__device__ __forceinline__ u64 priority_read_lane(u64 x, u32 lane_uniform) {
    const u32 lo = (u32)__builtin_amdgcn_readlane((int)(u32)x, (int)lane_uniform);
    const u32 hi = (u32)__builtin_amdgcn_readlane((int)(u32)(x >> 32), (int)lane_uniform);
    return ((u64)hi << 32) | lo;
}

template <typename E>
__device__ __forceinline__ void priority_descend_step(const E *__restrict__ arr, int64_t n, u32 lane, u64 &idx, u64 &t) {
    const u64 c0 = idx * (u64)QTTT_REPLAY_SCAN_BLOCK + 4u * lane;
    u64 x[4];
#pragma unroll
    for (u32 m = 0; m < 4u; ++m) x[m] = c0 + m < (u64)n ? (u64)arr[c0 + m] : 0ull;
    const u64 mine = x[0] + x[1] + x[2] + x[3];
    u64 incl = mine;
#pragma unroll
    for (u32 d = 1; d < 64u; d <<= 1) {
        const u64 up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    const u64 past = __ballot(incl > t);
    const u32 f = past ? (u32)__builtin_ctzll(past) : 63u;       // wave-uniform
    const u64 rem = t - (incl - mine);                           // meaningful in lane f
    u32 m = 3u;
    u64 before = x[0] + x[1] + x[2];
    if (x[0] + x[1] + x[2] > rem) { m = 2u; before = x[0] + x[1]; }
    if (x[0] + x[1] > rem) { m = 1u; before = x[0]; }
    if (x[0] > rem) { m = 0u; before = 0ull; }
    const u32 fu = (u32)__builtin_amdgcn_readfirstlane((int)f);
    const u32 child = (u32)__builtin_amdgcn_readlane((int)(4u * lane + m), (int)fu);
    t = priority_read_lane(rem - before, fu);
    const u64 to = idx * (u64)QTTT_REPLAY_SCAN_BLOCK + child;
    idx = to < (u64)n ? to : (u64)n - 1u;
}

template <bool SYM>
__global__ __launch_bounds__(REPLAY_SAMPLE_BLOCK) void replay_sample_prioritized_kernel(
    ReplayRing ring, PriorityTable tab, int64_t capacity, int64_t n, u64 key_slot, u64 key_sym, const uint8_t *sym,
    u32 random_symmetry, float *s_out, u64 *pi_out, uint8_t *mask_out, u32 *v_out, uint8_t *done_out, int32_t *index_out,
    uint8_t *sym_out, int64_t *number_out, u32 *q_out, u64 *total_out) {
    __shared__ __attribute__((aligned(16))) float tile[REPLAY_TILE * 180];
    __shared__ __attribute__((aligned(16))) u64 ptile[REPLAY_TILE * 36];
    __shared__ __attribute__((aligned(16))) uint8_t mtile[REPLAY_TILE * 36];
    __shared__ u64 drawn[REPLAY_TILE];
    const ReplayTiles tiles = {tile, ptile, mtile};
    const ReplaySampleOut out = {s_out, pi_out, mask_out, v_out, done_out, index_out, sym_out};
    const int64_t base = (int64_t)blockIdx.x * REPLAY_TILE;
    const u32 valid = (u32)min((int64_t)REPLAY_TILE, n - base);
    const u32 wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const u64 total = tab.sum[tab.levels - 1u][0];
    if (blockIdx.x == 0 && threadIdx.x == 0u && total_out) *total_out = total;

    if (total != 0ull) {                                         // workgroup-uniform
        u64 idx[PRIORITY_WAVE_SAMPLES], t[PRIORITY_WAVE_SAMPLES];
#pragma unroll
        for (u32 r = 0; r < PRIORITY_WAVE_SAMPLES; ++r) {
            const int64_t i = base + wave * PRIORITY_WAVE_SAMPLES + r;          // past n: drawn and dropped, never stored
            const Draw d = counter_draw(fold_id((u64)i), key_slot);
            idx[r] = 0ull;
            t[r] = __umul64hi(((u64)d.h2 << 32) | d.h1, total);  // < total
        }
        for (u32 lv = tab.levels - 1u; lv >= 1u; --lv) {         // from the top total down to level 1
#pragma unroll
            for (u32 r = 0; r < PRIORITY_WAVE_SAMPLES; ++r) priority_descend_step(tab.sum[lv - 1u], tab.n[lv], lane, idx[r], t[r]);
        }
#pragma unroll
        for (u32 r = 0; r < PRIORITY_WAVE_SAMPLES; ++r) {
            priority_descend_step(tab.q, tab.n[0], lane, idx[r], t[r]);
            if (lane == 0u) drawn[wave * PRIORITY_WAVE_SAMPLES + r] = idx[r];   // < capacity
        }
    }
    __syncthreads();

    const u32 b = threadIdx.x >> 4, j = threadIdx.x & 15u;
    const int64_t i = base + b;
    if (b < valid) {
        if (total == 0ull) {                                     // nothing has a priority: as the empty ring
            replay_sample_empty_rows(tiles, out, i, b, j);
            if (j == 14u) {
                if (number_out) number_out[i] = -1;
                if (q_out) q_out[i] = 0u;
            }
        } else {
            const u64 slot = drawn[b];
            const u32 k = replay_sample_symmetry<SYM>(i, fold_id((u64)i), key_sym, sym, random_symmetry);
            replay_sample_rows<SYM>(ring, tiles, out, i, b, j, slot, k);
            if (j == 14u) {
                if (number_out) number_out[i] = (int64_t)replay_holder(slot, ring.header[0], (u64)capacity);
                if (q_out) q_out[i] = tab.q[slot];
            }
        }
    }
    __syncthreads();
    replay_sample_stream(tiles, out, base, valid);
}

}  // namespace

#endif  // QTTT_REPLAY_PRIORITY_KERNELS_H
