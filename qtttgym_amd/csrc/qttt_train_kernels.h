// qttt_train_kernels.h — the training step of the policy/value network (include/qttt_train.h): the
// reference's loss (self_play.py:226-236), its gradients with respect to the packed f32 weight blob, and the AMSGrad step
// on that blob.  f32 on v_mfma_f32_16x16x4_f32, with qttt_nn_kernels.h's configuration, blob offsets, hidden layer, head
// and softmax statistics; the launch plan and the workspace layout are qttt_train_host.h's.
//
// Five launches make the gradients, ordered by the stream, none waiting on another workgroup:
//   train_count_kernel     n_keep = the number of non-terminal samples (an integer sum)
//   train_forward_kernel   a tile of 64 samples per workgroup: the trunk (nn_hidden), each layer's activations stored, the
//                          head (nn_head), then L, J and the output gradient dOut f32[n, 48]
//   train_backward_kernel  a tile per workgroup: dZ3 = (dOut . WH^T) * (h3 > 0), dZ2 = (dZ3 . W3^T) * (h2 > 0), dZ1 likewise;
//                          the B operand is the packed matrix read transposed (4-byte loads, L2-resident)
//   train_wgrad_kernel     dW[k][c] = sum_i hprev[i][k] dZ[i][c] and db[c] = sum_i dZ[i][c]: a workgroup owns a 64 x 64 block
//                          of one matrix for one chunk of QTTT_TRAIN_CHUNK samples; the samples are the MFMA's K; the partial
//                          goes to the workspace at the element's blob offset
//   train_reduce_kernel    grads[e] = the partials of element e added in ascending chunk order
// Rows past n are read as zeros and contribute exactly nothing.  No atomics, no scratch; every loop is bounded by a
// compile-time count or by n.
#ifndef QTTT_TRAIN_KERNELS_H
#define QTTT_TRAIN_KERNELS_H
#include "qttt_nn_kernels.h"
#include "qttt_train_host.h"

namespace {

static_assert(TRAIN_BLOB_FLOATS * 4 == NNBlob<0>::BYTES, "the host plan and the kernels agree on the blob");
static_assert(TRAIN_TILE == NNCfg<0>::M && TRAIN_HIDDEN == QTTT_NN_HIDDEN && TRAIN_HEAD_COLS == QTTT_NN_HEAD_COLS &&
              TRAIN_IN == NNCfg<0>::K1, "the host plan and the kernels agree on the network");
static_assert(QTTT_TRAIN_CHUNK % 4 == 0, "a chunk is a whole number of MFMA k-steps");

__global__ __launch_bounds__(QTTT_NN_BLOCK) void train_count_kernel(const uint8_t *__restrict__ done, int64_t n, u32 *n_keep) {
    __shared__ u32 part[QTTT_NN_BLOCK];
    u32 c = 0;
    for (int64_t i = threadIdx.x; i < n; i += QTTT_NN_BLOCK) c += done[i] == 0;
    part[threadIdx.x] = c;
    __syncthreads();
    for (u32 w = QTTT_NN_BLOCK / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) *n_keep = part[0];
}

// the tile's rows [0, valid) of the LDS activations to h[base ..][256], coalesced
__device__ __forceinline__ void train_store_tile(const float *H, float *__restrict__ h, int64_t base, u32 valid, u32 tid) {
    for (u32 k = tid; k < valid * QTTT_NN_HIDDEN; k += QTTT_NN_BLOCK)
        h[base * QTTT_NN_HIDDEN + k] = H[(k >> 8) * NNCfg<0>::LD + (k & 255u)];
}

// WEIGHTED (qttt_train_gradients_weighted, include/qttt_train_weighted.h): the loss tail multiplies the sample's output
// gradient, rounded as without weights, by weight[i] in f32; L and J stay unweighted.  A compile-time variant: the
// unweighted instantiation never looks at `weight` and keeps its code and registers (profiles/priority/kernel_resources.txt).
template <bool WEIGHTED>
__global__ __launch_bounds__(QTTT_NN_BLOCK) void train_forward_kernel(
    const float *__restrict__ s, const double *__restrict__ pi, const uint8_t *__restrict__ mask, const float *__restrict__ v,
    const uint8_t *__restrict__ done, int64_t n, const float *__restrict__ W, const u32 *__restrict__ n_keep_p,
    float *__restrict__ h1, float *__restrict__ h2, float *__restrict__ h3, float *__restrict__ dOut, float *__restrict__ Lout,
    float *__restrict__ Jout, const float *__restrict__ weight) {
    typedef NNCfg<0> C;
    typedef NNBlob<0> B;
    __shared__ __attribute__((aligned(16))) float H[C::M * C::LD];
    const u32 tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const int64_t base = (int64_t)blockIdx.x * C::M;
    const u32 valid = (u32)min((int64_t)C::M, n - base);
    const float *bias = W + B::END;

    // ---- the tile's rows of s (GameState.to_vector, 180 f32 each, contiguous); rows past n are zeros
    for (u32 k = tid; k < (u32)(C::M * C::K1); k += QTTT_NN_BLOCK) {
        const u32 b = k / (u32)C::K1, c = k - b * (u32)C::K1;
        H[b * C::LD + c] = b < valid ? s[base * C::K1 + k] : 0.f;
    }
    __syncthreads();

    // ---- the trunk and the head, as evaluate_kernel<0>; every layer's activations go to the workspace
    nn_hidden<0>(W + B::W1, bias, C::K1 / C::KS, H, wave, lane);
    train_store_tile(H, h1, base, valid, tid);
    nn_hidden<0>(W + B::W2, bias + QTTT_NN_HIDDEN, QTTT_NN_HIDDEN / C::KS, H, wave, lane);
    train_store_tile(H, h2, base, valid, tid);
    nn_hidden<0>(W + B::W3, bias + 2 * QTTT_NN_HIDDEN, QTTT_NN_HIDDEN / C::KS, H, wave, lane);
    train_store_tile(H, h3, base, valid, tid);
    float *O = H;
    nn_head<0>(W + B::WH, bias + 3 * QTTT_NN_HIDDEN, H, O, wave, lane);

    // ---- loss terms and the gradient at the outputs, a thread per sample
    if (tid < valid) {
        const int64_t i = base + tid;
        const float *o = O + tid * QTTT_NN_OUT_LD;
        float *dO = dOut + i * QTTT_NN_HEAD_COLS;
        const float diff = o[36] - v[i];
        float wi = 1.0f;
        if constexpr (WEIGHTED) wi = weight[i];
        float Jv = 0.f;
        if (done[i] == 0) {
            u64 lm = 0;
            for (u32 a = 0; a < 36u; ++a) lm |= (u64)(mask[i * 36 + a] != 0) << a;
            float mx, sum;
            nn_softmax_stats(o, lm, mx, sum);
            const float lse = logf(sum);
            const double keep = (double)*n_keep_p;
            double S = 0.0, Jd = 0.0;
            for (u32 a = 0; a < 36u; ++a)
                if (lm >> a & 1ull) S += pi[i * 36 + a];
            for (u32 a = 0; a < 36u; ++a) {
                float d = 0.f;
                if (lm >> a & 1ull) {
                    const double p = pi[i * 36 + a];
                    const float z = o[a] - mx;
                    Jd += p * (log(p + 1e-7) - (double)(z - lse));
                    d = (float)(((double)(expf(z) / sum) * S - p) / keep);
                }
                dO[a] = WEIGHTED ? d * wi : d;
            }
            Jv = (float)Jd;
        } else {
            for (u32 a = 0; a < 36u; ++a) dO[a] = 0.f;
        }
        dO[36] = WEIGHTED ? (diff / (float)n) * wi : diff / (float)n;
        for (u32 a = 37u; a < (u32)QTTT_NN_HEAD_COLS; ++a) dO[a] = 0.f;
        if (Lout) Lout[i] = 0.5f * diff * diff;
        if (Jout) Jout[i] = Jv;
    }
}

// One layer backwards on the tile: D <- (D[:, :4 KSTEPS] . B^T) * (hprev > 0), B the packed [256][16 NC] matrix at Wm, and
// the result's rows below `valid` to dz.  The transposed B fragment (k-step s, column tile t): lane l needs
// B[kk = 16 t + (l & 15)][c = 4 s + (l >> 4)], which the fragment order puts at ((kk/4 * NC + c/16) * 64 + kk%4 * 16 + c%16).
// Wave w owns the 64 output columns [64 w, 64 w + 64) for all 64 rows, as nn_hidden.
template <int NC, int KSTEPS>
__device__ __forceinline__ void train_back_layer(const float *__restrict__ Wm, const float *__restrict__ hprev,
                                                 float *__restrict__ dz, float *D, int64_t base, u32 valid, u32 wave, u32 lane) {
    typedef NNCfg<0> C;
    constexpr int MT = C::M / 16, NTW = 4;
    const u32 q = lane >> 4, j = lane & 15u;
    nn_f32x4 acc[MT][NTW];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int t = 0; t < NTW; ++t) acc[mt][t] = nn_f32x4{0.f, 0.f, 0.f, 0.f};
    u32 at[NTW];
#pragma unroll
    for (int t = 0; t < NTW; ++t) {
        const u32 kk = (wave * NTW + t) * 16u + j;
        at[t] = (kk >> 2) * NC * 64u + (kk & 3u) * 16u;
    }
    const float *Dr = D + j * C::LD + q;
#pragma unroll 2
    for (int s = 0; s < KSTEPS; ++s) {
        const u32 c = 4u * s + q, co = (c >> 4) * 64u + (c & 15u);
        float b[NTW];
#pragma unroll
        for (int t = 0; t < NTW; ++t) b[t] = Wm[at[t] + co];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const float a = Dr[mt * 16 * C::LD + s * 4];
#pragma unroll
            for (int t = 0; t < NTW; ++t) acc[mt][t] = nn_mfma(a, b[t], acc[mt][t]);
        }
    }
    __syncthreads();                                             // every wave is done reading D
#pragma unroll
    for (int t = 0; t < NTW; ++t) {
        const u32 col = (wave * NTW + t) * 16u + j;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const u32 row = mt * 16u + q * 4u + r;
                float g = 0.f;
                if (row < valid) {
                    const int64_t e = (base + row) * QTTT_NN_HIDDEN + col;
                    g = hprev[e] > 0.f ? acc[mt][t][r] : 0.f;
                    dz[e] = g;
                }
                D[row * C::LD + col] = g;
            }
    }
    __syncthreads();
}

__global__ __launch_bounds__(QTTT_NN_BLOCK) void train_backward_kernel(
    const float *__restrict__ W, const float *__restrict__ dOut, const float *__restrict__ h1, const float *__restrict__ h2,
    const float *__restrict__ h3, float *__restrict__ dz1, float *__restrict__ dz2, float *__restrict__ dz3, int64_t n) {
    typedef NNCfg<0> C;
    typedef NNBlob<0> B;
    __shared__ __attribute__((aligned(16))) float D[C::M * C::LD];
    const u32 tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const int64_t base = (int64_t)blockIdx.x * C::M;
    const u32 valid = (u32)min((int64_t)C::M, n - base);
    for (u32 k = tid; k < (u32)(C::M * QTTT_NN_HEAD_COLS); k += QTTT_NN_BLOCK) {
        const u32 b = k / (u32)QTTT_NN_HEAD_COLS, c = k - b * (u32)QTTT_NN_HEAD_COLS;
        D[b * C::LD + c] = b < valid ? dOut[base * QTTT_NN_HEAD_COLS + k] : 0.f;
    }
    __syncthreads();
    train_back_layer<QTTT_NN_HEAD_COLS / 16, QTTT_NN_HEAD_COLS / 4>(W + B::WH, h3, dz3, D, base, valid, wave, lane);
    train_back_layer<QTTT_NN_HIDDEN / 16, QTTT_NN_HIDDEN / 4>(W + B::W3, h2, dz2, D, base, valid, wave, lane);
    train_back_layer<QTTT_NN_HIDDEN / 16, QTTT_NN_HIDDEN / 4>(W + B::W2, h1, dz1, D, base, valid, wave, lane);
}

// The pointers of the weight-gradient launch: layer L's input rows x[L] (row stride ldx[L], K[L] of them used) and output
// gradient g[L] (row stride ldg[L] = 16 NC[L] columns), its matrix's and its biases' element offsets in the blob.
struct TrainWgradArgs {
    const float *x[4], *g[4];
};

__global__ __launch_bounds__(QTTT_NN_BLOCK) void train_wgrad_kernel(TrainWgradArgs a, int64_t n, float *__restrict__ partials) {
    typedef NNBlob<0> B;
    const u32 wave = threadIdx.x >> 6, lane = threadIdx.x & 63u, q = lane >> 4, j = lane & 15u;
    const int64_t chunk = blockIdx.x / (u32)TRAIN_WGRAD_BLOCKS;
    const TrainBlock blk = train_block((int)(blockIdx.x % (u32)TRAIN_WGRAD_BLOCKS));
    const bool head = blk.layer == 3;
    const u32 K = blk.layer == 0 ? (u32)TRAIN_IN : (u32)QTTT_NN_HIDDEN, ldx = K;
    const u32 NC = head ? QTTT_NN_HEAD_COLS / 16 : QTTT_NN_HIDDEN / 16, ldg = NC * 16u;
    const u32 t = (u32)blk.col_block * 4u + wave;                // this wave's column tile
    if (t >= NC) return;                                         // the head has three (no barrier below)
    const int64_t woff = blk.layer == 0 ? B::W1 : blk.layer == 1 ? B::W2 : blk.layer == 2 ? B::W3 : B::WH;
    const float *__restrict__ X = a.x[blk.layer];
    const float *__restrict__ G = a.g[blk.layer];
    const int64_t i0 = chunk * QTTT_TRAIN_CHUNK, i1 = min(n, i0 + (int64_t)QTTT_TRAIN_CHUNK);
    const u32 k0 = (u32)blk.row_block * 64u + j;                 // the row of the A fragment of row tile 0
    const float one = j == 0 ? 1.f : 0.f;                        // an A fragment whose row 0 is ones: the column sums
    nn_f32x4 acc[4], accb = nn_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) acc[mt] = nn_f32x4{0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < QTTT_TRAIN_CHUNK / 4; ++s) {
        const int64_t i = i0 + 4 * s + q;
        const bool live = i < i1;
        const float b = live ? G[i * ldg + t * 16u + j] : 0.f;
        float x[4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const u32 k = k0 + mt * 16u;
            x[mt] = (live && k < K) ? X[i * ldx + k] : 0.f;
        }
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) acc[mt] = nn_mfma(x[mt], b, acc[mt]);
        if (blk.row_block == 0) accb = nn_mfma(one, b, accb);
    }
    float *P = partials + chunk * TRAIN_BLOB_FLOATS;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {                            // C/D: row = (lane >> 4)*4 + r, column = lane & 15
            const u32 k = (u32)blk.row_block * 64u + mt * 16u + q * 4u + r;
            if (k < K) P[woff + ((k >> 2) * NC + t) * 64u + (k & 3u) * 16u + j] = acc[mt][r];
        }
    if (blk.row_block == 0 && q == 0) P[B::END + blk.layer * QTTT_NN_HIDDEN + t * 16u + j] = accb[0];
}

__global__ __launch_bounds__(QTTT_NN_BLOCK) void train_reduce_kernel(const float *__restrict__ partials, int64_t chunks,
                                                                     float *__restrict__ grads) {
    const u32 e = blockIdx.x * QTTT_NN_BLOCK + threadIdx.x;
    if (e >= (u32)TRAIN_BLOB_FLOATS) return;
    float sum = partials[e];
    for (int64_t c = 1; c < chunks; ++c) sum += partials[c * TRAIN_BLOB_FLOATS + e];
    grads[e] = sum;
}

// The element offset, in the QTTT_NN_BF16 blob's matrices, of the f32 blob's weight element e < NNBlob<0>::END.
__device__ __forceinline__ u32 train_bf16_offset(u32 e) {
    typedef NNBlob<0> F;
    typedef NNBlob<1> H;
    u32 local, nc, start;
    if (e < (u32)F::W2) { local = e; nc = 16; start = (u32)H::W1; }
    else if (e < (u32)F::W3) { local = e - (u32)F::W2; nc = 16; start = (u32)H::W2; }
    else if (e < (u32)F::WH) { local = e - (u32)F::W3; nc = 16; start = (u32)H::W3; }
    else { local = e - (u32)F::WH; nc = 3; start = (u32)H::WH; }
    const u32 frag = local >> 6, k = (frag / nc) * 4u + ((local >> 4) & 3u), ct = frag % nc, cj = local & 15u;
    return start + (((k >> 5) * nc + ct) * 64u + ((k & 31u) >> 3) * 16u + cj) * 8u + (k & 7u);
}

struct TrainAdam {
    float beta1, beta2, eps, weight_decay, step_size, bc2_sqrt;  // step_size = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t)
};

__global__ __launch_bounds__(QTTT_NN_BLOCK) void train_adam_kernel(float *__restrict__ w, const float *__restrict__ grads,
                                                                   float *__restrict__ m, float *__restrict__ v2,
                                                                   float *__restrict__ vmax, TrainAdam h, void *bf16) {
    const u32 e = blockIdx.x * QTTT_NN_BLOCK + threadIdx.x;
    if (e >= (u32)TRAIN_BLOB_FLOATS) return;
    const float w0 = w[e];
    const float g = grads[e] + h.weight_decay * w0;
    const float m1 = h.beta1 * m[e] + (1.f - h.beta1) * g;
    const float v1 = h.beta2 * v2[e] + (1.f - h.beta2) * g * g;
    const float vm = fmaxf(vmax[e], v1);
    const float w1 = w0 - h.step_size * (m1 / (sqrtf(vm) / h.bc2_sqrt + h.eps));
    m[e] = m1;
    v2[e] = v1;
    vmax[e] = vm;
    w[e] = w1;
    if (bf16) {
        if (e < (u32)NNBlob<0>::END) static_cast<__bf16 *>(bf16)[train_bf16_offset(e)] = (__bf16)w1;
        else reinterpret_cast<float *>(static_cast<__bf16 *>(bf16) + NNBlob<1>::END)[e - (u32)NNBlob<0>::END] = w1;
    }
}

}  // namespace

#endif  // QTTT_TRAIN_KERNELS_H
