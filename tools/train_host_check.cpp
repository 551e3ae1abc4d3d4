// train_host_check.cpp — a stand-alone host program over qtttgym_amd/csrc/qttt_train_host.h (the workspace layout and the
// launch plan of include/qttt_train.h), meant to be built with the host sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Iqtttgym_amd/csrc
//       tools/train_host_check.cpp -o train_host_check && ./train_host_check
// No GPU and no HIP: it walks batch sizes up to the limit (where a 32-bit intermediate would overflow), checks that the
// workspace's arrays are aligned, ordered and disjoint, and replays the stores of the weight-gradient launch (every output
// block, wave, lane and register, with the kernel's own index arithmetic) into an exactly-sized blob: an offset past the
// blob is a heap overflow the sanitizer reports, and every element must be stored exactly once.
#include <cstdio>
#include <vector>
#include "qttt_train_host.h"

static int failures = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);             \
            ++failures;                                                       \
        }                                                                     \
    } while (0)

static void check_plan(int64_t n) {
    const TrainPlan p = train_plan(n);
    EXPECT(p.tiles == (n + 63) / 64 && p.chunks == (n + QTTT_TRAIN_CHUNK - 1) / QTTT_TRAIN_CHUNK);
    EXPECT(p.wgrad_groups == p.chunks * 48 && p.reduce_groups * 256 >= TRAIN_BLOB_FLOATS && (p.reduce_groups - 1) * 256 < TRAIN_BLOB_FLOATS);
    EXPECT(p.tiles <= 0x7FFFFFFF && p.wgrad_groups <= 0x7FFFFFFF);          // a grid's x dimension
    const int64_t off[9] = {p.h[0], p.h[1], p.h[2], p.dz[0], p.dz[1], p.dz[2], p.dout, p.partials, p.count};
    const int64_t size[9] = {n * 1024, n * 1024, n * 1024, n * 1024, n * 1024, n * 1024, n * 192, p.chunks * TRAIN_BLOB_FLOATS * 4, 4};
    int64_t end = 0;
    for (int k = 0; k < 9; ++k) {
        EXPECT(off[k] % 256 == 0 && off[k] >= end && off[k] - end < 256);
        end = off[k] + size[k];
    }
    EXPECT(p.bytes >= end && p.bytes % 256 == 0 && p.bytes - end <= 256);
}

// the stores of train_wgrad_kernel for one chunk
static void check_wgrad_cover() {
    std::vector<uint8_t> hit((size_t)TRAIN_BLOB_FLOATS, 0);
    const int64_t W[4] = {0, TRAIN_IN * 256, TRAIN_IN * 256 + 65536, TRAIN_IN * 256 + 2 * 65536};
    const int64_t END = W[3] + 256 * 48;
    int seen[4][4][4] = {};
    for (int job = 0; job < (int)TRAIN_WGRAD_BLOCKS; ++job) {
        const TrainBlock b = train_block(job);
        EXPECT(b.layer >= 0 && b.layer < 4 && b.row_block >= 0 && b.row_block < 4 && b.col_block >= 0 && b.col_block < 4);
        ++seen[b.layer][b.row_block][b.col_block];
        const unsigned K = b.layer == 0 ? 180u : 256u, NC = b.layer == 3 ? 3u : 16u;
        for (unsigned wave = 0; wave < 4; ++wave) {
            const unsigned t = (unsigned)b.col_block * 4u + wave;
            if (t >= NC) continue;
            for (unsigned lane = 0; lane < 64; ++lane) {
                const unsigned q = lane >> 4, j = lane & 15u;
                for (unsigned mt = 0; mt < 4; ++mt)
                    for (unsigned r = 0; r < 4; ++r) {
                        const unsigned k = (unsigned)b.row_block * 64u + mt * 16u + q * 4u + r;
                        if (k < K) ++hit[(size_t)(W[b.layer] + ((k >> 2) * NC + t) * 64u + (k & 3u) * 16u + j)];
                    }
                if (b.row_block == 0 && q == 0) ++hit[(size_t)(END + b.layer * 256 + t * 16u + j)];
            }
        }
    }
    int64_t wrong = 0;
    for (uint8_t h : hit) wrong += h != 1;
    EXPECT(wrong == 0);
    for (int l = 0; l < 4; ++l)
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) EXPECT(seen[l][r][c] == ((l == 0 && r == 3) || (l == 3 && c > 0) ? 0 : 1));
}

int main() {
    EXPECT(TRAIN_BLOB_FLOATS * 4 == 761024);
    const int64_t C = QTTT_TRAIN_CHUNK, MAX = QTTT_TRAIN_MAX_SAMPLES;
    for (int64_t n : {(int64_t)1, (int64_t)2, (int64_t)63, (int64_t)64, (int64_t)65, C - 1, C, C + 1, 2 * C + 1, (int64_t)4096, (int64_t)65536,
                      (int64_t)1000003, MAX - 1, MAX})
        check_plan(n);
    EXPECT(train_samples_bad(0) && train_samples_bad(-1) && train_samples_bad(MAX + 1) && !train_samples_bad(1) && !train_samples_bad(MAX));
    EXPECT(train_plan(MAX).bytes > ((int64_t)1 << 32));
    check_wgrad_cover();
    std::printf(failures ? "train_host_check: %d FAILED\n" : "train_host_check: ok\n", failures);
    return failures ? 1 : 0;
}
