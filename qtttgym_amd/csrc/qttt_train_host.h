// qttt_train_host.h — host only, plain C++ without HIP: the workspace layout and the launch plan of
// include/qttt_train.h's qttt_train_gradients.  Kept apart from the kernels so that a stand-alone program can exercise
// this code under the host sanitizers (tools/train_host_check.cpp).  qttt_train_workspace_bytes is train_plan(n).bytes.
#ifndef QTTT_TRAIN_HOST_H
#define QTTT_TRAIN_HOST_H
#include <stdint.h>
#include "qttt.h"

namespace {

constexpr int64_t TRAIN_TILE = 64;                   // samples per workgroup of the forward and backward launches
constexpr int64_t TRAIN_HIDDEN = 256, TRAIN_HEAD_COLS = 48, TRAIN_IN = 180;
// f32 elements of the QTTT_NN_F32 blob: W1, W2, W3, the head, the biases (qttt_train_kernels.h asserts it is NNBlob<0>'s)
constexpr int64_t TRAIN_BLOB_FLOATS = TRAIN_IN * TRAIN_HIDDEN + 2 * TRAIN_HIDDEN * TRAIN_HIDDEN +
                                      TRAIN_HIDDEN * TRAIN_HEAD_COLS + 3 * TRAIN_HIDDEN + TRAIN_HEAD_COLS;
// output blocks (64 rows x 64 columns) of the weight-gradient launch per chunk: layer 1 has 3 x 4 (180 rows), layers 2
// and 3 have 4 x 4, the head 4 x 1 (48 columns)
constexpr int64_t TRAIN_WGRAD_BLOCKS = 12 + 16 + 16 + 4;

inline bool train_samples_bad(int64_t n) { return n < 1 || n > QTTT_TRAIN_MAX_SAMPLES; }
inline int64_t train_align256(int64_t bytes) { return (bytes + 255) & ~(int64_t)255; }

// Byte offsets into the workspace, each 256-byte aligned: h[L] = the post-ReLU activations of layer L + 1 and dz[L] =
// the gradient at its pre-activations, f32[n, 256] each; dout f32[n, 48]; partials f32[chunks, TRAIN_BLOB_FLOATS]; count
// = u32 n_keep.  tiles / chunks / wgrad_groups / reduce_groups: the grids of the launches.
struct TrainPlan {
    int64_t tiles, chunks, wgrad_groups, reduce_groups;
    int64_t h[3], dz[3], dout, partials, count;
    int64_t bytes;
};
inline TrainPlan train_plan(int64_t n) {
    TrainPlan p = {};
    p.tiles = (n + TRAIN_TILE - 1) / TRAIN_TILE;
    p.chunks = (n + QTTT_TRAIN_CHUNK - 1) / QTTT_TRAIN_CHUNK;
    p.wgrad_groups = p.chunks * TRAIN_WGRAD_BLOCKS;
    p.reduce_groups = (TRAIN_BLOB_FLOATS + 255) / 256;
    int64_t at = 0;
    const int64_t act = train_align256(n * TRAIN_HIDDEN * 4);
    for (int k = 0; k < 3; ++k) { p.h[k] = at; at += act; }
    for (int k = 0; k < 3; ++k) { p.dz[k] = at; at += act; }
    p.dout = at;
    at += train_align256(n * TRAIN_HEAD_COLS * 4);
    p.partials = at;
    at += train_align256(p.chunks * TRAIN_BLOB_FLOATS * 4);
    p.count = at;
    at += 256;
    p.bytes = at;
    return p;
}

// The output block `job` (0 .. TRAIN_WGRAD_BLOCKS - 1) of the weight-gradient launch: which layer (0, 1, 2 = the trunk, 3 =
// the head), which 64 rows and which 64 columns of its matrix.  Shared by the kernel and the host check.
struct TrainBlock { int layer, row_block, col_block; };
inline
#if defined(__HIPCC__)
__host__ __device__
#endif
TrainBlock train_block(int job) {
    if (job < 12) return {0, job / 4, job % 4};
    if (job < 28) return {1, (job - 12) / 4, (job - 12) % 4};
    if (job < 44) return {2, (job - 28) / 4, (job - 28) % 4};
    return {3, job - 44, 0};
}

}  // namespace

#endif  // QTTT_TRAIN_HOST_H
