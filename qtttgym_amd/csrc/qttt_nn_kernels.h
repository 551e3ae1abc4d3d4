// qttt_nn_kernels.h — the reference's policy/value network (nn.py:7-72: 180 -> 256 -> 256 -> 256 ReLU trunk, value head
// -> 1, policy head -> 36, illegal actions masked to -inf) evaluated for a batch of packed boards in ONE kernel, on the
// matrix cores.  Two instantiations of one template: exact-f32 MFMA (v_mfma_f32_16x16x4_f32, the reference's numerics)
// and bf16 MFMA (v_mfma_f32_16x16x32_bf16: bf16 weights and activations, f32 accumulation and biases).
//
// Mapping: a 256-thread workgroup owns a tile of M boards (64 f32 / 128 bf16).  The tile's activations
// live in LDS as [M][LD] rows (board-major; padded rows, no bank conflicts on the A-fragment reads) and are overwritten
// layer by layer; the weights stream from L2 straight into B fragments, pre-arranged by the packer (include/qttt_nn.h
// "packed weight blob") so that a wave's fragment is one contiguous 256 B / 1 KB load.  Hidden layers: wave w owns the
// 64 output columns [64w, 64w + 64) for all M boards, i.e. 4 x M/16 accumulator tiles of 16 x 16; the 256 -> 37 head
// (36 logits + value, padded to 48 columns) is split over the boards instead.  Layer 1 is the dense K = 180 product
// over the to_vector encoding, which the workgroup builds in LDS from the packed state (the gather form is priced
// against it in DESIGN.md §10).  Everything is bounded by compile-time trip counts or by n; no atomics; no scratch.
#ifndef QTTT_NN_KERNELS_H
#define QTTT_NN_KERNELS_H
#include "qttt_board_forms.h"

namespace {

typedef float nn_f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 nn_bf16x8 __attribute__((ext_vector_type(8)));

#define QTTT_NN_BLOCK 256
#define QTTT_NN_HIDDEN 256
#define QTTT_NN_HEAD_COLS 48           // 36 logits, the value, 11 zero columns
#define QTTT_NN_BIASES (3 * QTTT_NN_HIDDEN + QTTT_NN_HEAD_COLS)
#define QTTT_NN_OUT_LD 49              // f32 row stride of the head's output tile in LDS

template <int PREC> struct NNCfg;
template <> struct NNCfg<0> {          // QTTT_NN_F32
    typedef float T;                   // weight / activation element
    typedef float Frag;                // one lane's A or B fragment
    static constexpr int M = 64;       // boards per workgroup tile
    static constexpr int KS = 4;       // K of one MFMA
    static constexpr int K1 = 180;     // layer-1 K padded to a multiple of KS
    static constexpr int LD = 260;     // LDS row stride in elements: 260 mod 64 = 4, the 16 rows x 4 k of a fragment hit 64 banks
};
template <> struct NNCfg<1> {          // QTTT_NN_BF16
    typedef __bf16 T;
    typedef nn_bf16x8 Frag;
    static constexpr int M = 128;
    static constexpr int KS = 32;
    static constexpr int K1 = 192;
    static constexpr int LD = 264;     // 528 B rows: the 16 rows of a 16-lane b128 read land 16 B apart in the banks
};

// element offsets of the four weight matrices in the blob, then the f32 biases
template <int PREC> struct NNBlob {
    static constexpr int64_t W1 = 0;
    static constexpr int64_t W2 = W1 + (int64_t)NNCfg<PREC>::K1 * QTTT_NN_HIDDEN;
    static constexpr int64_t W3 = W2 + (int64_t)QTTT_NN_HIDDEN * QTTT_NN_HIDDEN;
    static constexpr int64_t WH = W3 + (int64_t)QTTT_NN_HIDDEN * QTTT_NN_HIDDEN;
    static constexpr int64_t END = WH + (int64_t)QTTT_NN_HIDDEN * QTTT_NN_HEAD_COLS;
    static constexpr int64_t BYTES = END * (int64_t)sizeof(typename NNCfg<PREC>::T) + QTTT_NN_BIASES * 4;
};

__device__ __forceinline__ nn_f32x4 nn_mfma(float a, float b, nn_f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ nn_f32x4 nn_mfma(nn_bf16x8 a, nn_bf16x8 b, nn_f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// One hidden layer H <- relu(H[:, :K] . B + bias) on the tile, B = W^T in fragment order (relu as torch's: NaN
// propagates, include/qttt_nn.h).  A fragment (k-step s, row
// tile mt): lane l reads row mt*16 + (l & 15), k = s*KS + (l >> 4)*EPL .. +EPL-1; B fragment (s, column tile t) is the
// blob's fragment s*16 + t, lane l's EPL elements at ((s*16 + t)*64 + l)*EPL.  The next k-step's B fragments are loaded
// before this step's MFMAs (the L2 latency of the weights is the exposed part of the loop).
template <int PREC>
__device__ __forceinline__ void nn_hidden(const typename NNCfg<PREC>::T *__restrict__ W, const float *__restrict__ bias,
                                          int ksteps, typename NNCfg<PREC>::T *H, u32 wave, u32 lane) {
    typedef NNCfg<PREC> C;
    typedef typename C::T T;
    typedef typename C::Frag Frag;
    constexpr int MT = C::M / 16, EPL = C::KS / 4, NTW = 4;
    nn_f32x4 acc[MT][NTW];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int j = 0; j < NTW; ++j) acc[mt][j] = nn_f32x4{0.f, 0.f, 0.f, 0.f};
    const Frag *Wf = reinterpret_cast<const Frag *>(W) + wave * NTW * 64 + lane;
    const T *Hr = H + (lane & 15u) * C::LD + (lane >> 4) * EPL;
    Frag b[NTW], bn[NTW];
#pragma unroll
    for (int j = 0; j < NTW; ++j) b[j] = Wf[j * 64];
    for (int s = 0; s < ksteps; ++s) {
        const int sn = s + 1 < ksteps ? s + 1 : s;
#pragma unroll
        for (int j = 0; j < NTW; ++j) bn[j] = Wf[(sn * 16 + j) * 64];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const Frag a = *reinterpret_cast<const Frag *>(Hr + mt * 16 * C::LD + s * C::KS);
#pragma unroll
            for (int j = 0; j < NTW; ++j) acc[mt][j] = nn_mfma(a, b[j], acc[mt][j]);
        }
#pragma unroll
        for (int j = 0; j < NTW; ++j) b[j] = bn[j];
    }
    __syncthreads();                                             // every wave is done reading the layer's input
#pragma unroll
    for (int j = 0; j < NTW; ++j) {
        const u32 col = (wave * NTW + j) * 16u + (lane & 15u);
        const float bv = bias[col];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {                        // C/D: column = lane & 15, row = (lane >> 4)*4 + r
                const float z = acc[mt][j][r] + bv;              // torch.relu: a NaN stays a NaN (fmaxf would return 0)
                H[(mt * 16 + (lane >> 4) * 4 + r) * C::LD + col] = (T)(z < 0.f ? 0.f : z);
            }
    }
    __syncthreads();
}

// The fused head: O[m][0..47] = H . BH + bias (no ReLU; nn.py's head ReLU repeats the trunk's).  Wave w owns the row
// tiles w, w + 4, ...  O is an f32 [M][QTTT_NN_OUT_LD] tile that overlays H.
template <int PREC>
__device__ __forceinline__ void nn_head(const typename NNCfg<PREC>::T *__restrict__ W, const float *__restrict__ bias,
                                        typename NNCfg<PREC>::T *H, float *O, u32 wave, u32 lane) {
    typedef NNCfg<PREC> C;
    typedef typename C::T T;
    typedef typename C::Frag Frag;
    constexpr int MTW = C::M / 64, EPL = C::KS / 4, NT = QTTT_NN_HEAD_COLS / 16;
    nn_f32x4 acc[MTW][NT];
#pragma unroll
    for (int i = 0; i < MTW; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = nn_f32x4{0.f, 0.f, 0.f, 0.f};
    const Frag *Wf = reinterpret_cast<const Frag *>(W) + lane;
    const T *Hr = H + (wave * 16u + (lane & 15u)) * C::LD + (lane >> 4) * EPL;
    for (int s = 0; s < QTTT_NN_HIDDEN / C::KS; ++s) {
        Frag b[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) b[j] = Wf[(s * NT + j) * 64];
#pragma unroll
        for (int i = 0; i < MTW; ++i) {
            const Frag a = *reinterpret_cast<const Frag *>(Hr + i * 64 * C::LD + s * C::KS);
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[i][j] = nn_mfma(a, b[j], acc[i][j]);
        }
    }
    __syncthreads();                                             // O overwrites H
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const u32 col = j * 16u + (lane & 15u);
        const float bv = bias[col];
#pragma unroll
        for (int i = 0; i < MTW; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                O[((wave + 4u * i) * 16u + (lane >> 4) * 4u + r) * QTTT_NN_OUT_LD + col] = acc[i][j][r] + bv;
    }
    __syncthreads();
}

// Row b of the to_vector encoding (mcts.py:67-85, as encode_kernel) at x, the quarter `part` of it (four threads per row),
// and legal[b], the row's legal mask (GameState.actions of the autofilled board, nn.py:44-61's mask).  A row that is not
// `live` gets zeros and an empty mask; the board P[base + b] / Q[base + b] (global memory or LDS) is read only for a live
// row.  Shared by evaluate_kernel
// and rollout_policy_kernel.
template <int PREC>
__device__ __forceinline__ void nn_encode_row(typename NNCfg<PREC>::T *x, u64 *legal, u32 b, bool live, const u64 *P,
                                              const u64 *Q, int64_t base, u32 part) {
    typedef NNCfg<PREC> C;
    typedef typename C::T T;
    if (live) {
        Cold s;
        cold_unpack(P[base + b], Q[base + b], s);
        const u32 qsets = s.comp(0) | s.comp(1) | s.comp(2) | s.comp(3);
        for (u32 v = part; v < 9u; v += 4u) {
            const u32 col = (s.cl >> v & 1u) ? s.sqv(v) : 9u;        // board -1 indexes column 9
            u32 touched = 0;
            for (u32 t = 0; t < s.n; ++t)
                if ((s.mv(t) & 0xFu) == v || (s.mv(t) >> 4) == v) touched |= 1u << t;
            for (u32 c = 0; c < 10u; ++c) {
                x[v * 10u + c] = (T)(c == col ? 1.0f : 0.0f);
                float q = (touched >> c & 1u) ? (1.0f / 3.0f) : 0.0f;   // 1/math.sqrt(9)
                if (c == 9u && !(qsets >> v & 1u)) q = 1.0f;            // square in no qstruct
                x[90u + v * 10u + c] = (T)q;
            }
        }
        if (part == 3u) legal[b] = fast_legal_mask(s.cl);
    } else {                                                             // tail rows: zeros, outputs not written
        for (u32 k = part; k < 180u; k += 4u) x[k] = (T)0.0f;
        if (part == 3u) legal[b] = 0;
    }
    for (u32 k = 180u + part; k < (u32)C::K1; k += 4u) x[k] = (T)0.0f;  // K padding (bf16)
}

// The mask and softmax of one head row o[0..35] (nn.py:44-61: action (i,j) -> -inf iff square i or j is classical;
// torch.softmax / Categorical(logits).probs): the max and the exp-sum over the legal actions, in ascending action
// order, and a probability from them.  A row with every action masked gives NaN probabilities, like torch.
__device__ __forceinline__ void nn_softmax_stats(const float *o, u64 lm, float &mx_out, float &sum_out) {
    float mx = -INFINITY, sum = 0.f;
    for (u32 a = 0; a < 36u; ++a)
        if (lm >> a & 1ull) mx = fmaxf(mx, o[a]);
    for (u32 a = 0; a < 36u; ++a)
        if (lm >> a & 1ull) sum += expf(o[a] - mx);
    mx_out = mx;
    sum_out = sum;
}
__device__ __forceinline__ float nn_prob(float lg, bool ok, u64 lm, float mx, float sum) {
    return ok ? expf(lg - mx) / sum : (lm ? 0.f : __builtin_nanf(""));
}

template <int PREC>
__global__ __launch_bounds__(QTTT_NN_BLOCK) void evaluate_kernel(const u64 *pP, const u64 *pQ, const void *weights,
                                                                 float *value, float *logits, float *probs, int64_t n) {
    typedef NNCfg<PREC> C;
    typedef typename C::T T;
    typedef NNBlob<PREC> L;
    static_assert(C::M * QTTT_NN_OUT_LD * 4 <= C::M * C::LD * (int)sizeof(T), "head tile must fit over the activations");
    __shared__ __attribute__((aligned(16))) T H[C::M * C::LD];
    __shared__ u64 legal[C::M];
    __shared__ float rmax[C::M], rsum[C::M];
    const u32 tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const int64_t base = (int64_t)blockIdx.x * C::M;
    const u32 valid = (u32)min((int64_t)C::M, n - base);
    const T *W = reinterpret_cast<const T *>(weights);
    const float *bias = reinterpret_cast<const float *>(W + L::END);

    // ---- the to_vector encoding (mcts.py:67-85, as encode_kernel) of the tile's boards: four threads per board
    for (u32 b = tid >> 2; b < (u32)C::M; b += QTTT_NN_BLOCK / 4) {
        const u32 part = tid & 3u;
        nn_encode_row<PREC>(H + b * C::LD, legal, b, b < valid, pP, pQ, base, part);
    }
    __syncthreads();

    // ---- the trunk and the head on the matrix cores
    nn_hidden<PREC>(W + L::W1, bias, C::K1 / C::KS, H, wave, lane);
    nn_hidden<PREC>(W + L::W2, bias + QTTT_NN_HIDDEN, QTTT_NN_HIDDEN / C::KS, H, wave, lane);
    nn_hidden<PREC>(W + L::W3, bias + 2 * QTTT_NN_HIDDEN, QTTT_NN_HIDDEN / C::KS, H, wave, lane);
    float *O = reinterpret_cast<float *>(H);
    nn_head<PREC>(W + L::WH, bias + 3 * QTTT_NN_HIDDEN, H, O, wave, lane);

    // ---- mask and softmax (nn_softmax_stats, nn_prob)
    if (probs && tid < valid) {
        nn_softmax_stats(O + tid * QTTT_NN_OUT_LD, legal[tid], rmax[tid], rsum[tid]);
    }
    __syncthreads();
    if (value)
        for (u32 b = tid; b < valid; b += QTTT_NN_BLOCK) value[base + b] = O[b * QTTT_NN_OUT_LD + 36u];
    if (logits || probs) {                                       // the tile's rows are contiguous: coalesced stores
        const u32 cnt = valid * 36u;
        for (u32 k = tid; k < cnt; k += QTTT_NN_BLOCK) {
            const u32 b = k / 36u, a = k - b * 36u;
            const u64 lm = legal[b];
            const bool ok = lm >> a & 1ull;
            const float lg = O[b * QTTT_NN_OUT_LD + a];
            if (logits) logits[base * 36 + k] = ok ? lg : -INFINITY;
            if (probs) probs[base * 36 + k] = nn_prob(lg, ok, lm, rmax[b], rsum[b]);
        }
    }
}

}  // namespace

#endif  // QTTT_NN_KERNELS_H
