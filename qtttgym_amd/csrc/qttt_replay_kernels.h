// qttt_replay_kernels.h — the replay ring on the device (include/qttt_replay.h): the scan levels and the
// move of qttt_replay_append, and the one launch of qttt_replay_sample, which gathers whole rows from random slots,
// builds the (permuted) to_vector encoding and the permuted pi / mask rows of a tile of samples in LDS — encode_kernel's
// plan — and streams them out as coalesced 16-byte stores (its row functions serve the prioritised draw of
// qttt_replay_priority_kernels.h as well).  Behind them the two launches of reanalysis
// (include/qttt_replay_reanalyse.h): a window of the ring as a state buffer, and the guarded write-back.
#ifndef QTTT_REPLAY_KERNELS_H
#define QTTT_REPLAY_KERNELS_H
#include "qttt_mcts_kernels.h"
#include "qttt_symmetry_kernels.h"
#include "qttt_replay_host.h"
#include "qttt_replay.h"
#include "qttt_replay_reanalyse.h"

namespace {

// the ring's arrays (qttt_replay_layout), as the kernels take them
struct ReplayRing {
    u64 *header, *P, *Q, *pi, *mask;
    u32 *v;
    uint8_t *done;
};
inline ReplayRing replay_ring(void *replay, int64_t capacity) {
    const ReplayLayout l = replay_layout(capacity);
    uint8_t *b = static_cast<uint8_t *>(replay);
    return {reinterpret_cast<u64 *>(b), reinterpret_cast<u64 *>(b + l.off[0]), reinterpret_cast<u64 *>(b + l.off[1]),
            reinterpret_cast<u64 *>(b + l.off[2]), reinterpret_cast<u64 *>(b + l.off[3]), reinterpret_cast<u32 *>(b + l.off[4]),
            b + l.off[5]};
}

// what the move reads of the scan: level k's exclusive prefixes, the grand total, `written` as the first launch found it
struct ReplayRanks {
    const u64 *excl[REPLAY_MAX_LEVELS];
    const u64 *total, *written0;
    u32 levels;
};

// One level of the scan: a workgroup turns QTTT_REPLAY_SCAN_BLOCK entries of `arr` into their exclusive prefix and writes
// their total to totals[blockIdx.x] (wave scan + wave totals; no other workgroup is looked at).  FIRST: the entries are the
// games' clamped lengths, and lane 0 of the launch copies the header's `written` for the later launches.
template <bool FIRST>
__global__ __launch_bounds__(QTTT_REPLAY_SCAN_BLOCK) void replay_scan_kernel(const uint8_t *length, u64 *arr, u64 *totals, int64_t n,
                                                                             const u64 *header, u64 *written0) {
    __shared__ u64 wave_tot[QTTT_REPLAY_SCAN_BLOCK / 64];
    const u32 t = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * QTTT_REPLAY_SCAN_BLOCK + t;
    u64 x = 0;
    if (i < n) x = FIRST ? (u64)min((u32)length[i], (u32)QTTT_SELFPLAY_ROWS) : arr[i];
    u64 incl = x;
#pragma unroll
    for (u32 d = 1; d < 64u; d <<= 1) {
        const u64 up = __shfl_up(incl, d, 64);
        if ((t & 63u) >= d) incl += up;
    }
    if ((t & 63u) == 63u) wave_tot[t >> 6] = incl;
    __syncthreads();
    u64 before = 0, all = 0;
#pragma unroll
    for (u32 w = 0; w < (u32)(QTTT_REPLAY_SCAN_BLOCK / 64); ++w) {
        const u64 y = wave_tot[w];
        before += w < (t >> 6) ? y : 0ull;
        all += y;
    }
    if (i < n) arr[i] = before + incl - x;
    if (t == 0u) totals[blockIdx.x] = all;
    if (FIRST && i == 0) *written0 = header[0];
}

// The move: one wavefront per game (the augment kernel's mapping).  Lane a < 36 moves pi entry a of every row and gives
// its mask bit to the ballot; lane 0 moves the rest of the row.  Sample r of the batch's n goes to slot (written + r) %
// capacity, the first n - capacity of them nowhere; a wave stores only to its own samples' slots.  Lane 0 of the launch
// writes the header: nothing in this launch reads it.
constexpr int REPLAY_APPEND_BLOCK = 256, REPLAY_APPEND_GAMES = REPLAY_APPEND_BLOCK / 64;
__global__ __launch_bounds__(REPLAY_APPEND_BLOCK) void replay_append_kernel(ReplayRing ring, int64_t capacity, int64_t games,
                                                                            const u64 *states, const u64 *pi, const uint8_t *mask,
                                                                            const uint8_t *done, const u32 *v, const uint8_t *length,
                                                                            ReplayRanks rk) {
    const int64_t g = (int64_t)blockIdx.x * REPLAY_APPEND_GAMES + threadIdx.x / 64;
    const u32 lane = threadIdx.x & 63u;
    const u64 n = *rk.total, w0 = *rk.written0, cap = (u64)capacity;
    if (blockIdx.x == 0 && threadIdx.x == 0) ring.header[0] = w0 + n;
    if (g >= games) return;
    const u32 rows = min((u32)length[g], (u32)QTTT_SELFPLAY_ROWS);
    u64 rank = 0;
    for (u32 k = 0; k < rk.levels; ++k) rank += rk.excl[k][g >> (8u * k)];
    const u64 skip = n > cap ? n - cap : 0ull;
    const int64_t stride = plane_stride(games);
    for (u32 t = 0; t < rows; ++t) {                             // wave-uniform: every lane of the wave takes the same path
        const u64 r = rank + t;
        if (r < skip) continue;
        const u64 slot = (w0 + r) % cap;
        const int64_t row = (int64_t)t * games + g;
        bool bit = false;
        if (lane < 36u) {
            ring.pi[slot * 36u + lane] = pi[row * 36 + lane];
            bit = mask[row * 36 + lane] != 0;
        }
        const u64 bits = __ballot(bit);
        if (lane == 0u) {
            const u64 *plane = states + (int64_t)t * 2 * stride;
            ring.P[slot] = plane[g];
            ring.Q[slot] = plane[stride + g];
            ring.mask[slot] = bits;
            ring.v[slot] = v[row];
            ring.done[slot] = done[row];
        }
    }
}

// The sample: a 256-thread workgroup owns a tile of REPLAY_TILE = 16 samples, thread (sample b, part j) with j = 0..15.
// Every part computes its sample's slot and symmetry itself (two hashes, no exchange).  Part j < 9 builds the rows of
// square j (to_vector's rows j and 9 + j, as encode_kernel) at the place of sigma(j); every part moves the pi entries and
// mask bits of actions j, j + 16, j + 32 to the place of tau; part 15 writes the sample's scalars.  Then all four waves
// stream the three LDS tiles out.  16 samples: 16.3 KB of LDS, so eight workgroups fit a CU and the 32-wave cap, not LDS,
// bounds the occupancy; and a minibatch of 4 096 is 256 workgroups, one per CU.
constexpr int REPLAY_TILE = 16, REPLAY_SAMPLE_BLOCK = 256;
// The three LDS tiles of a workgroup's samples.  The row functions below are what qttt_replay_sample and
// qttt_replay_sample_prioritized (qttt_replay_priority_kernels.h) share: the two differ in how a sample's slot is drawn.
struct ReplayTiles {
    float *tile;                                                 // [REPLAY_TILE * 180]
    u64 *ptile;                                                  // [REPLAY_TILE * 36]
    uint8_t *mtile;                                              // [REPLAY_TILE * 36]
};
struct ReplaySampleOut {
    float *s_out;
    u64 *pi_out;
    uint8_t *mask_out;
    u32 *v_out;
    uint8_t *done_out;
    int32_t *index_out;
    uint8_t *sym_out;
};

// sample i's symmetry: sym[i] when given (a value past 7: the identity), else the hash's top three bits, else 0
template <bool SYM>
__device__ __forceinline__ u32 replay_sample_symmetry(int64_t i, u32 id, u64 key_sym, const uint8_t *sym, u32 random_symmetry) {
    u32 k = 0;
    if constexpr (SYM) {
        if (sym) k = sym[i] < (u32)QTTT_SYMMETRIES ? sym[i] : 0u;
        else if (random_symmetry) k = counter_draw(id, key_sym).h2 >> 29;
    }
    return k;
}

// part j of sample b of the tile when there is nothing to draw from: zero rows, index -1
__device__ __forceinline__ void replay_sample_empty_rows(const ReplayTiles &t, const ReplaySampleOut &out, int64_t i, u32 b, u32 j) {
    float *o = t.tile + b * 180u;
    for (u32 c = j; c < 180u; c += 16u) o[c] = 0.0f;
    for (u32 a = j; a < 36u; a += 16u) {
        t.ptile[b * 36u + a] = 0ull;
        t.mtile[b * 36u + a] = 0;
    }
    if (j == 15u) {
        out.v_out[i] = 0u;
        out.done_out[i] = 0;
        if (out.index_out) out.index_out[i] = -1;
        if (out.sym_out) out.sym_out[i] = 0;
    }
}

// part j of sample b of the tile: the rows of slot `slot` under symmetry k into the LDS tiles, the scalars straight out
template <bool SYM>
__device__ __forceinline__ void replay_sample_rows(const ReplayRing &ring, const ReplayTiles &t, const ReplaySampleOut &out,
                                                   int64_t i, u32 b, u32 j, u64 slot, u32 k) {
    float *o = t.tile + b * 180u;
    const u64 cells = g_sym_tables.cells[k];
    if (j < 9u) {                                        // encode_kernel's rows, spelled out: one square per thread
        Cold s;                                          // here, and that kernel's own stream (a leg of bench.py) stays
        cold_unpack(ring.P[slot], ring.Q[slot], s);
        const u32 v = j, w = SYM ? sym_cell(cells, v) : v;
        const u32 qsets = s.comp(0) | s.comp(1) | s.comp(2) | s.comp(3);
        const u32 col = (s.cl >> v & 1u) ? s.sqv(v) : 9u;   // board -1 indexes column 9
        u32 touched = 0;                                    // rounds whose move touches v
        for (u32 r = 0; r < s.n; ++r)
            if ((s.mv(r) & 0xFu) == v || (s.mv(r) >> 4) == v) touched |= 1u << r;
        for (u32 c = 0; c < 10u; ++c) {
            o[w * 10u + c] = c == col ? 1.0f : 0.0f;
            float q = (touched >> c & 1u) ? (1.0f / 3.0f) : 0.0f;   // 1/math.sqrt(9)
            if (c == 9u && !(qsets >> v & 1u)) q = 1.0f;    // square in no qstruct
            o[90u + w * 10u + c] = q;
        }
    }
    const u64 mbits = ring.mask[slot];
    for (u32 a = j; a < 36u; a += 16u) {
        const u32 to = SYM ? sym_action_of_pair(cells, g_pair_lut.b[a]) : a;
        t.ptile[b * 36u + to] = ring.pi[slot * 36u + a];
        t.mtile[b * 36u + to] = (uint8_t)(mbits >> a & 1ull);
    }
    if (j == 15u) {
        out.v_out[i] = ring.v[slot];
        out.done_out[i] = ring.done[slot] != 0 ? 1 : 0;
        if (out.index_out) out.index_out[i] = (int32_t)slot;
        if (out.sym_out) out.sym_out[i] = (uint8_t)k;
    }
}

// all four waves stream the three LDS tiles of the tile's `valid` samples out (after a __syncthreads)
__device__ __forceinline__ void replay_sample_stream(const ReplayTiles &t, const ReplaySampleOut &out, int64_t base, u32 valid) {
    {
        const u32 n4 = valid * 45u;                                // 16-byte pieces of the encoding in this tile
        const u32x4 *src = reinterpret_cast<const u32x4 *>(t.tile);
        u32x4 *dst = reinterpret_cast<u32x4 *>(out.s_out + base * 180);
        for (u32 q = threadIdx.x; q < n4; q += REPLAY_SAMPLE_BLOCK) __builtin_nontemporal_store(src[q], &dst[q]);
    }
    {
        const u32 n4 = valid * 18u;                                // 16-byte pieces of pi (36 x 8 bytes = 18 x 16)
        const u32x4 *src = reinterpret_cast<const u32x4 *>(t.ptile);
        u32x4 *dst = reinterpret_cast<u32x4 *>(out.pi_out + base * 36);
        for (u32 q = threadIdx.x; q < n4; q += REPLAY_SAMPLE_BLOCK) __builtin_nontemporal_store(src[q], &dst[q]);
    }
    {
        const u32 n4 = valid * 9u;                                 // 4-byte pieces of the mask (36 = 9 x 4)
        const u32 *src = reinterpret_cast<const u32 *>(t.mtile);
        u32 *dst = reinterpret_cast<u32 *>(out.mask_out + base * 36);
        for (u32 q = threadIdx.x; q < n4; q += REPLAY_SAMPLE_BLOCK) dst[q] = src[q];
    }
}

template <bool SYM>
__global__ __launch_bounds__(REPLAY_SAMPLE_BLOCK) void replay_sample_kernel(ReplayRing ring, int64_t capacity, int64_t n, u64 key_slot,
                                                                            u64 key_sym, const uint8_t *sym, u32 random_symmetry,
                                                                            float *s_out, u64 *pi_out, uint8_t *mask_out, u32 *v_out,
                                                                            uint8_t *done_out, int32_t *index_out, uint8_t *sym_out) {
    __shared__ __attribute__((aligned(16))) float tile[REPLAY_TILE * 180];
    __shared__ __attribute__((aligned(16))) u64 ptile[REPLAY_TILE * 36];
    __shared__ __attribute__((aligned(16))) uint8_t mtile[REPLAY_TILE * 36];
    const ReplayTiles tiles = {tile, ptile, mtile};
    const ReplaySampleOut out = {s_out, pi_out, mask_out, v_out, done_out, index_out, sym_out};
    const int64_t base = (int64_t)blockIdx.x * REPLAY_TILE;
    const u32 b = threadIdx.x >> 4, j = threadIdx.x & 15u;
    const int64_t i = base + b;
    const u32 valid = (u32)min((int64_t)REPLAY_TILE, n - base);
    const u64 written = ring.header[0];
    const u64 filled = written < (u64)capacity ? written : (u64)capacity;
    if (b < valid) {
        if (filled == 0ull) {                                    // an empty ring: zero rows, index -1
            replay_sample_empty_rows(tiles, out, i, b, j);
        } else {
            const u32 id = fold_id((u64)i);
            const Draw d = counter_draw(id, key_slot);
            const u64 slot = __umul64hi(((u64)d.h2 << 32) | d.h1, filled);   // < filled <= capacity
            replay_sample_rows<SYM>(ring, tiles, out, i, b, j, slot, replay_sample_symmetry<SYM>(i, id, key_sym, sym, random_symmetry));
        }
    }
    __syncthreads();
    replay_sample_stream(tiles, out, base, valid);
}

// ---- reanalysis (include/qttt_replay_reanalyse.h)
// The gather: a lane per board of the state buffer, the padding behind board n - 1 included (it gets the empty board, as
// qttt_reset gives it).  The window is consecutive slots, so consecutive lanes load and store consecutive addresses in
// every array; the one break is where the window wraps.  `hash` is the window's draw, taken on the host.
constexpr int REPLAY_GATHER_BLOCK = 256;
__global__ __launch_bounds__(REPLAY_GATHER_BLOCK) void replay_gather_kernel(ReplayRing ring, int64_t capacity, int64_t n, u64 hash,
                                                                            int64_t start, u64 *state_out, int32_t *slot_out,
                                                                            int64_t *number_out, u32 *v_out, uint8_t *done_out) {
    const int64_t i = (int64_t)blockIdx.x * REPLAY_GATHER_BLOCK + threadIdx.x;
    const int64_t stride = plane_stride(n);
    if (i >= stride) return;
    u64 P = 0ull, Q = 0ull;                                      // the empty board is the all-zero state
    if (i < n) {
        const u64 written = ring.header[0];
        const u64 filled = written < (u64)capacity ? written : (u64)capacity;
        int64_t slot = -1, number = -1;
        u32 v = 0u;
        uint8_t done = 0;
        if ((u64)i < filled) {
            const u64 s = replay_window_slot(replay_window_start(start, hash, filled), (u64)i, filled);   // < filled <= capacity
            slot = (int64_t)s;
            number = (int64_t)replay_holder(s, written, (u64)capacity);
            P = ring.P[s];
            Q = ring.Q[s];
            if (v_out) v = ring.v[s];
            if (done_out) done = ring.done[s];
        }
        slot_out[i] = (int32_t)slot;
        number_out[i] = number;
        if (v_out) v_out[i] = v;
        if (done_out) done_out[i] = done;
    }
    state_out[i] = P;
    state_out[stride + i] = Q;
}

// The update: sixteen lanes per sample (the sample kernel's group), part j moving the pi words j, j + 16, j + 32 of the
// row, so a group's stores are consecutive addresses.  Part 0 evaluates the guard once — the slot is held, still by the
// sample it was gathered for, and not a terminal row — writes v and the flag, and broadcasts the slot (or -1) to its group.
// Distinct slots (the header's condition): no two groups store to one slot.  No lane leaves before the broadcast.
constexpr int REPLAY_UPDATE_BLOCK = 256, REPLAY_UPDATE_LANES = 16, REPLAY_UPDATE_SAMPLES = REPLAY_UPDATE_BLOCK / REPLAY_UPDATE_LANES;
__global__ __launch_bounds__(REPLAY_UPDATE_BLOCK) void replay_update_kernel(ReplayRing ring, int64_t capacity, int64_t n,
                                                                            const int32_t *slot, const int64_t *number, const u64 *pi,
                                                                            const u32 *v, uint8_t *updated_out) {
    const u32 j = threadIdx.x & (u32)(REPLAY_UPDATE_LANES - 1);
    const int64_t i = (int64_t)blockIdx.x * REPLAY_UPDATE_SAMPLES + threadIdx.x / REPLAY_UPDATE_LANES;
    int32_t to = -1;
    if (j == 0u && i < n) {
        const u64 written = ring.header[0];
        const u64 filled = written < (u64)capacity ? written : (u64)capacity;
        const int32_t s = slot[i];
        if (s >= 0 && (u64)s < filled && replay_holder((u64)s, written, (u64)capacity) == (u64)number[i] && ring.done[s] == 0) to = s;
        if (to >= 0 && v) ring.v[to] = v[i];
        if (updated_out) updated_out[i] = to >= 0 ? 1 : 0;
    }
    to = __shfl(to, (int)((threadIdx.x & 63u) & ~(u32)(REPLAY_UPDATE_LANES - 1)), 64);
    if (to < 0 || !pi) return;
    for (u32 a = j; a < 36u; a += (u32)REPLAY_UPDATE_LANES) ring.pi[(u64)to * 36u + a] = pi[i * 36 + a];
}

}  // namespace

#endif  // QTTT_REPLAY_KERNELS_H
