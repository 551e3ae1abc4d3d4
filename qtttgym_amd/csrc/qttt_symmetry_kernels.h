// qttt_symmetry_kernels.h — the board's eight symmetries (include/qttt_symmetry.h): the image of a
// packed state, for a batch of boards (transform_kernel) and for every row of a self-play batch (selfplay_augment_kernel).
//
// The image is built from the state alone, in packed words (no per-thread arrays): the generic unpacked form
// (cold_unpack) gives Board.board / Board.moves, sigma maps them into the words qttt_import's lane reads from its LDS
// tiles, the qstructs list comes from replaying the un-collapsed moves, and import_board — the importer's own code —
// builds the rooted forest, the x nibbles and the done bit.  So the image of a state IS an imported position, and an
// imported position is bit for bit the state stepping reaches (import_board's contract).
#ifndef QTTT_SYMMETRY_KERNELS_H
#define QTTT_SYMMETRY_KERNELS_H
#include "qttt_aux_kernels.h"
#include "qttt_tree_kernels.h"
#include "qttt_selfplay_kernels.h"
#include "qttt_symmetry.h"

namespace {

// sigma_k as nine nibbles of one word (square v at bits [4v, 4v + 4)); inverse and composition for the host table entry
struct SymTables {
    u64 cells[QTTT_SYMMETRIES];
    uint8_t inverse[QTTT_SYMMETRIES];
    uint8_t compose[QTTT_SYMMETRIES][QTTT_SYMMETRIES];
    static constexpr u32 sigma(u32 k, u32 v) {
        u32 r = v / 3u, c = v % 3u;
        if (k & 4u) c = 2u - c;                                  // mirror first
        for (u32 q = 0; q < (k & 3u); ++q) {                     // then quarter turns clockwise
            const u32 nr = c, nc = 2u - r;
            r = nr;
            c = nc;
        }
        return 3u * r + c;
    }
    constexpr SymTables() : cells(), inverse(), compose() {
        for (u32 k = 0; k < QTTT_SYMMETRIES; ++k)
            for (u32 v = 0; v < 9u; ++v) cells[k] |= (u64)sigma(k, v) << (4u * v);
        for (u32 a = 0; a < QTTT_SYMMETRIES; ++a)
            for (u32 b = 0; b < QTTT_SYMMETRIES; ++b)
                for (u32 k = 0; k < QTTT_SYMMETRIES; ++k) {
                    bool same = true;
                    for (u32 v = 0; v < 9u; ++v) same = same && sigma(k, v) == sigma(b, sigma(a, v));
                    if (same) {
                        compose[a][b] = (uint8_t)k;
                        if (k == 0u) inverse[a] = (uint8_t)b;
                    }
                }
    }
};
constexpr SymTables SYM_TABLES = SymTables();
__constant__ SymTables g_sym_tables = SymTables();

// sigma(v) from the packed word; a square past 8 (255: none, or garbage) reads 0 from the empty nibbles
__host__ __device__ __forceinline__ u32 sym_cell(u64 cells, u32 v) { return (u32)(cells >> (4u * (v & 15u))) & 0xFu; }
// move2ind (mcts.py:345-350) of a sorted pair: row i of the lexicographic order starts at i (17 - i) / 2
__host__ __device__ __forceinline__ u32 sym_move2ind(u32 lo, u32 hi) { return ((lo * (17u - lo)) >> 1) + (hi - lo - 1u); }
// tau(a) of an action index below 36; pr = its pair as lo | hi << 4
__host__ __device__ __forceinline__ u32 sym_action_of_pair(u64 cells, u32 pr) {
    const u32 a = sym_cell(cells, pr & 0xFu), b = sym_cell(cells, pr >> 4);
    return sym_move2ind(min(a, b), max(a, b));
}

// update_qstructs (board.py:27-69) of a move that closes no cycle, on the packed list (4 x 9-bit masks, list order,
// compact): append a new set, add to the set of the end that has one, or merge hi's set into lo's and pop it
__device__ __forceinline__ u64 sym_replay_move(u64 comps, u32 lo, u32 hi) {
    const u32 mlo = (u32)(comps >> lo) & SLOT_LSB, mhi = (u32)(comps >> hi) & SLOT_LSB;
    const u64 pm = (u64)((1u << lo) | (1u << hi));
    if (mlo != 0u && mhi != 0u) {
        const u32 sl = (u32)__builtin_ctz(mlo), sh = (u32)__builtin_ctz(mhi);     // 0, 9, 18 or 27
        if (sl == sh) return comps;                              // (a cycle: no reachable state's live move closes one)
        comps |= ((comps >> sh) & 0x1FFull) << sl;
        return (comps & ((1ull << sh) - 1ull)) | ((comps >> (sh + 9u)) << sh);
    }
    if ((mlo | mhi) != 0u) return comps | (pm << (u32)__builtin_ctz(mlo | mhi));
    const u32 c32 = (u32)comps;                                  // the first empty slot (the slots are compact)
    const u32 used = (c32 & 0x1FFu ? 1u : 0u) + ((c32 >> 9) & 0x1FFu ? 1u : 0u) + ((c32 >> 18) & 0x1FFu ? 1u : 0u) +
                     ((comps >> 27) ? 1u : 0u);
    return used < 4u ? comps | (pm << (9u * used)) : comps;
}

// The image of one state under the symmetry whose packed sigma is `cells`.  lut: the workgroup's line table.
__device__ __forceinline__ void sym_image(u64 Pin, u64 Qin, u64 cells, const uint8_t *lut, u64 &Pout, u64 &Qout) {
    Cold s;
    cold_unpack(Pin, Qin, s, false);                             // the implicit autofill stays implicit
    const u32 n = min(s.n, 9u);
    // Board.board of the image as qttt_import's words (-1 = not classical), and the rounds that stand on a square
    u64 b07 = ~0ull;
    u32 b8 = 0xFFu, on_board = 0u;
#pragma unroll
    for (u32 v = 0; v < 9u; ++v) {
        if (s.cl >> v & 1u) {
            const u32 w = sym_cell(cells, v), r = s.sqv(v);
            on_board |= 1u << r;
            if (w < 8u) b07 = (b07 & ~(0xFFull << (8u * w))) | ((u64)r << (8u * w));
            else b8 = r;
        }
    }
    // Board.moves of the image, every pair re-sorted (255, 255 where not played), and the qstructs list: the moves that
    // are still un-collapsed (their round stands on no square) replayed in round order.  (Round 8 always closes a cycle.)
    const u32 live = ~on_board & ((1u << n) - 1u) & 0xFFu;
    u64 m03 = ~0ull, m47 = ~0ull, comps = 0ull;
    u32 m8 = 0xFFFFu;
#pragma unroll
    for (u32 t = 0; t < 9u; ++t) {
        if (t < n) {
            const u32 m = s.mv(t);
            const u32 a = sym_cell(cells, m & 0xFu), b = sym_cell(cells, m >> 4);
            const u32 lo = min(a, b), hi = max(a, b);
            const u64 pr = (u64)(lo | (hi << 8));
            if (t < 4u) m03 = (m03 & ~(0xFFFFull << (16u * t))) | (pr << (16u * t));
            else if (t < 8u) m47 = (m47 & ~(0xFFFFull << (16u * (t - 4u)))) | (pr << (16u * (t - 4u)));
            else m8 = (u32)pr;
            if (live >> t & 1u) comps = sym_replay_move(comps, lo, hi);
        }
    }
    const u32 c32 = (u32)comps;
    const u64 qm = (u64)(c32 & 0x1FFu) | ((u64)((c32 >> 9) & 0x1FFu) << 16) | ((u64)((c32 >> 18) & 0x1FFu) << 32) |
                   ((comps >> 27) << 48);
    import_board(m03, m47, m8, n, b07, b8, qm, 4u, lut, Pout, Qout);
}

// sym (nullable): one symmetry per board; else every board's is k.  One lane per board, as the cold kernels.
__global__ __launch_bounds__(QTTT_COLD_BLOCK) void transform_kernel(const u64 *inP, const u64 *inQ, u64 *outP, u64 *outQ,
                                                                    const uint8_t *sym, u32 k, int64_t n) {
    __shared__ __attribute__((aligned(16))) uint8_t lut[LINE_LUT_BYTES];
    const int64_t i = (int64_t)blockIdx.x * QTTT_COLD_BLOCK + threadIdx.x;
    u64 P = 0ull, Q = 0ull;
    u32 ks = k;
    if (i < n) {                                                 // requested before the table fill
        P = load_stream(&inP[i]);
        Q = load_stream(&inQ[i]);
        if (sym) ks = sym[i];
    }
    fill_line_lut<QTTT_COLD_BLOCK>(lut);                         // ends with the workgroup barrier
    if (i >= n) return;
    if (ks < (u32)QTTT_SYMMETRIES) sym_image(P, Q, g_sym_tables.cells[ks], lut, P, Q);
    store_stream(&outP[i], P);
    store_stream(&outQ[i], Q);
}

// One wavefront per OUTPUT game j = s * games + g (the record kernel's mapping): lane a < 36 moves the
// pi and mask entries of action a of every row, lane t < length the rest of row t, its state's image included, lane 63
// the per-game values.  A wave writes only its own game's columns: no atomics.  syms: symmetries[s] in nibble s.
__global__ __launch_bounds__(TREE_BLOCK) void selfplay_augment_kernel(int64_t games, u32 n_sym, u32 syms, SelfPlayOut in,
                                                                      SelfPlayOut out) {
    __shared__ __attribute__((aligned(16))) uint8_t lut[LINE_LUT_BYTES];
    fill_line_lut<TREE_BLOCK>(lut);                              // ends with the workgroup barrier
    const int64_t total = games * (int64_t)n_sym;
    const int64_t j = (int64_t)blockIdx.x * TREE_GAMES_PER_BLOCK + threadIdx.x / 64;
    const u32 lane = threadIdx.x & 63u;
    if (j >= total) return;
    const int64_t g = j % games;
    const u32 s = (u32)(j / games);
    const u64 cells = g_sym_tables.cells[(syms >> (4u * s)) & 7u];
    const u32 rows = min((u32)in.length[g], (u32)QTTT_SELFPLAY_ROWS);
    if (lane < 36u) {
        const u32 to = sym_action_of_pair(cells, g_pair_lut.b[lane]);
        const u64 *pi_in = reinterpret_cast<const u64 *>(in.pi);        // the eight bytes, whatever they hold (a NaN row)
        u64 *pi_out = reinterpret_cast<u64 *>(out.pi);
        for (u32 t = 0; t < rows; ++t) {
            const int64_t ri = ((int64_t)t * games + g) * 36, ro = ((int64_t)t * total + j) * 36;
            pi_out[ro + to] = pi_in[ri + lane];
            out.mask[ro + to] = in.mask[ri + lane];
        }
    }
    if (lane < rows) {
        const int64_t si = plane_stride(games), so = plane_stride(total);
        const int64_t ri = (int64_t)lane * games + g, ro = (int64_t)lane * total + j;
        const u64 *pin = in.states + (int64_t)lane * 2 * si;
        u64 *pout = out.states + (int64_t)lane * 2 * so;
        u64 P, Q;
        sym_image(pin[g], pin[si + g], cells, lut, P, Q);
        pout[j] = P;
        pout[so + j] = Q;
        out.done[ro] = in.done[ri];
        reinterpret_cast<u32 *>(out.v)[ro] = reinterpret_cast<const u32 *>(in.v)[ri];
        const u32 a = in.action36[ri];
        out.action36[ro] = (uint8_t)(a < 36u ? sym_action_of_pair(cells, g_pair_lut.b[a]) : a);
    }
    if (lane == 63u) {
        out.length[j] = in.length[g];
        out.winner[j] = in.winner[g];
        const u32 a0 = in.actions[2 * g], a1 = in.actions[2 * g + 1];
        out.actions[2 * j] = (uint8_t)(a0 < 9u ? sym_cell(cells, a0) : a0);
        out.actions[2 * j + 1] = (uint8_t)(a1 < 9u ? sym_cell(cells, a1) : a1);
    }
}

}  // namespace

#endif  // QTTT_SYMMETRY_KERNELS_H
