// qttt_nn_symmetric_kernels.h — the policy/value network averaged over a position's symmetries in ONE kernel
// (include/qttt_nn_symmetric.h): evaluate_kernel's trunk and head (qttt_nn_kernels.h) on a tile whose rows
// are the IMAGES of the boards, and an epilogue that maps every image's outputs back and takes the mean per board.
//
// Rows.  A workgroup's M rows (64 f32 / 128 bf16) are M / n_sym boards x n_sym images: row r is board r / n_sym under the
// symmetry at list position r % n_sym (per-board form: n_sym = 1, row r under sym[board]).  Rows past n * n_sym are zero
// rows and store nothing.
// Encoding.  nn_encode_row reads Board.board, the moves and the set of squares in a qstruct, nothing else; under sigma
// the board value, the rounds touching a square and its membership of a qstruct all travel with the square.  So the
// image's row is the board's row with the block of square v written at sigma(v), both halves, and its legal mask is the
// mask of sigma(classical): the replay of the mirrored game (sym_image) is not needed.
// Epilogue.  Masked logits, softmax statistics and probabilities per image row exactly as evaluate_kernel computes them;
// then thread (board b, action a) gathers the n_sym values at column tau_j[a] of the board's n_sym adjacent rows and sums
// them as the header's balanced tree.  LDS reads of the gather: with a fastest over the lanes, the 32 lanes of a
// ds_read_b32 group read distinct columns of one row (tau is a permutation), or of two rows where a board ends inside
// the group; the head tile's odd row stride (QTTT_NN_OUT_LD = 49 dwords) keeps rows apart, and what is left is the wrap of
// columns 32..35 onto banks 0..3 — two-way on at most four banks, as in evaluate_kernel's own epilogue.  (The other
// assignment, a board per lane, would put 32 rows n_sym * 49 dwords apart on 4 banks.)  legal / rmax / rsum / rowk are
// read at one address per board: broadcasts.
// No atomics; every loop is bounded by a compile-time count or by n; no scratch; LDS as evaluate_kernel's plus M bytes.
#ifndef QTTT_NN_SYMMETRIC_KERNELS_H
#define QTTT_NN_SYMMETRIC_KERNELS_H
#include "qttt_nn_kernels.h"
#include "qttt_symmetry_kernels.h"

namespace {

// nn_encode_row of the image of board (P, Q) under the symmetry whose packed sigma is `cells`: the quarter `part` of row
// x, and legal[row].  A row that is not `live` gets zeros and an empty mask.
template <int PREC>
__device__ __forceinline__ void nn_encode_image_row(typename NNCfg<PREC>::T *x, u64 *legal, u32 row, bool live, u64 P, u64 Q,
                                                    u64 cells, u32 part) {
    typedef NNCfg<PREC> C;
    typedef typename C::T T;
    if (live) {
        Cold s;
        cold_unpack(P, Q, s);
        const u32 qsets = s.comp(0) | s.comp(1) | s.comp(2) | s.comp(3);
        for (u32 v = part; v < 9u; v += 4u) {
            const u32 w = sym_cell(cells, v);                        // where square v's block goes
            const u32 col = (s.cl >> v & 1u) ? s.sqv(v) : 9u;
            u32 touched = 0;
            for (u32 t = 0; t < s.n; ++t)
                if ((s.mv(t) & 0xFu) == v || (s.mv(t) >> 4) == v) touched |= 1u << t;
            for (u32 c = 0; c < 10u; ++c) {
                x[w * 10u + c] = (T)(c == col ? 1.0f : 0.0f);
                float q = (touched >> c & 1u) ? (1.0f / 3.0f) : 0.0f;
                if (c == 9u && !(qsets >> v & 1u)) q = 1.0f;
                x[90u + w * 10u + c] = (T)q;
            }
        }
        if (part == 3u) {
            u32 cl = 0;
#pragma unroll
            for (u32 v = 0; v < 9u; ++v) cl |= (s.cl >> v & 1u) << sym_cell(cells, v);
            legal[row] = fast_legal_mask(cl);
        }
    } else {
        for (u32 k = part; k < 180u; k += 4u) x[k] = (T)0.0f;
        if (part == 3u) legal[row] = 0;
    }
    for (u32 k = 180u + part; k < (u32)C::K1; k += 4u) x[k] = (T)0.0f;  // K padding (bf16)
}

// one image's mapped-back masked logit and probability of an action
struct NNSymTerm {
    float l, p;
    __device__ __forceinline__ NNSymTerm operator+(const NNSymTerm &o) const { return NNSymTerm{l + o.l, p + o.p}; }
};

// The mean of x(0) .. x(n_sym - 1), n_sym in {1, 2, 4, 8} (wave-uniform), as include/qttt_nn_symmetric.h defines it: the
// balanced tree level by level in f32, then the exact scale.  Constant indices after unrolling: registers.
template <typename X, typename F>
__device__ __forceinline__ X nn_sym_tree(u32 n_sym, X zero, F &&x) {
    X t[QTTT_SYMMETRIES];
#pragma unroll
    for (u32 j = 0; j < (u32)QTTT_SYMMETRIES; ++j) t[j] = j < n_sym ? x(j) : zero;
#pragma unroll
    for (u32 half = QTTT_SYMMETRIES / 2; half >= 1u; half >>= 1)     // 4 sums (n_sym >= 2), then 2 (>= 4), then 1 (8)
        if (n_sym * half >= (u32)QTTT_SYMMETRIES)
#pragma unroll
            for (u32 j = 0; j < half; ++j) t[j] = t[2u * j] + t[2u * j + 1u];
    return t[0];
}

// sym (nullable): one symmetry per board (n_sym = 1; an entry past 7 is the identity); else list position j's symmetry
// is nibble j of `syms`.  n_sym = 1 << ls.
template <int PREC>
__global__ __launch_bounds__(QTTT_NN_BLOCK) void evaluate_symmetric_kernel(const u64 *pP, const u64 *pQ, const void *weights,
                                                                           const uint8_t *sym, u32 syms, u32 ls, float *value,
                                                                           float *logits, float *probs, int64_t n) {
    typedef NNCfg<PREC> C;
    typedef typename C::T T;
    typedef NNBlob<PREC> L;
    static_assert(C::M * QTTT_NN_OUT_LD * 4 <= C::M * C::LD * (int)sizeof(T), "head tile must fit over the activations");
    __shared__ __attribute__((aligned(16))) T H[C::M * C::LD];
    __shared__ u64 legal[C::M];
    __shared__ float rmax[C::M], rsum[C::M];
    __shared__ uint8_t rowk[C::M];                               // the symmetry of every row
    const u32 tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const u32 n_sym = 1u << ls, tile_boards = (u32)C::M >> ls;
    const int64_t base = (int64_t)blockIdx.x * tile_boards;      // the tile's first board
    const u32 valid = (u32)min((int64_t)tile_boards, n - base);  // boards of the tile
    const T *W = reinterpret_cast<const T *>(weights);
    const float *bias = reinterpret_cast<const float *>(W + L::END);

    // ---- the encoding of the tile's images: four threads per row
    for (u32 r = tid >> 2; r < (u32)C::M; r += QTTT_NN_BLOCK / 4) {
        const u32 part = tid & 3u, b = r >> ls;
        const bool live = b < valid;
        u64 P = 0ull, Q = 0ull;
        u32 k = (syms >> (4u * (r & (n_sym - 1u)))) & 7u;
        if (live) {
            P = pP[base + b];
            Q = pQ[base + b];
            if (sym) {
                k = sym[base + b];
                k = k < (u32)QTTT_SYMMETRIES ? k : 0u;
            }
        }
        nn_encode_image_row<PREC>(H + r * C::LD, legal, r, live, P, Q, g_sym_tables.cells[k], part);
        if (part == 3u) rowk[r] = (uint8_t)k;
    }
    __syncthreads();

    // ---- the trunk and the head on the matrix cores, as evaluate_kernel
    nn_hidden<PREC>(W + L::W1, bias, C::K1 / C::KS, H, wave, lane);
    nn_hidden<PREC>(W + L::W2, bias + QTTT_NN_HIDDEN, QTTT_NN_HIDDEN / C::KS, H, wave, lane);
    nn_hidden<PREC>(W + L::W3, bias + 2 * QTTT_NN_HIDDEN, QTTT_NN_HIDDEN / C::KS, H, wave, lane);
    float *O = reinterpret_cast<float *>(H);
    nn_head<PREC>(W + L::WH, bias + 3 * QTTT_NN_HIDDEN, H, O, wave, lane);

    // ---- every image row's softmax statistics (nn_softmax_stats), then the mean per board through tau
    if (probs && tid < (valid << ls)) {
        nn_softmax_stats(O + tid * QTTT_NN_OUT_LD, legal[tid], rmax[tid], rsum[tid]);
    }
    __syncthreads();
    const float scale = 1.0f / (float)n_sym;
    if (value)
        for (u32 b = tid; b < valid; b += QTTT_NN_BLOCK) {
            const float s = nn_sym_tree(n_sym, 0.f, [&](u32 j) { return O[((b << ls) + j) * QTTT_NN_OUT_LD + 36u]; });
            value[base + b] = ls ? s * scale : s;
        }
    if (logits || probs) {                                       // the tile's boards are contiguous: coalesced stores
        const u32 cnt = valid * 36u;
        for (u32 k = tid; k < cnt; k += QTTT_NN_BLOCK) {
            const u32 b = k / 36u, a = k - b * 36u;
            const u32 pr = g_pair_lut.b[a];
            const NNSymTerm s = nn_sym_tree(n_sym, NNSymTerm{0.f, 0.f}, [&](u32 j) {
                const u32 r = (b << ls) + j;
                const u32 ta = sym_action_of_pair(g_sym_tables.cells[rowk[r]], pr);
                const u64 lm = legal[r];
                const bool ok = lm >> ta & 1ull;
                const float lg = O[r * QTTT_NN_OUT_LD + ta];
                return NNSymTerm{ok ? lg : -INFINITY, probs ? nn_prob(lg, ok, lm, rmax[r], rsum[r]) : 0.f};
            });
            if (logits) logits[base * 36 + k] = ls ? s.l * scale : s.l;
            if (probs) probs[base * 36 + k] = ls ? s.p * scale : s.p;
        }
    }
}

}  // namespace

#endif  // QTTT_NN_SYMMETRIC_KERNELS_H
