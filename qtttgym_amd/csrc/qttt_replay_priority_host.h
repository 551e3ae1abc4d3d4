// qttt_replay_priority_host.h — host only, plain C++ without HIP: the layout of the priority table, the plan of the sum
// launches, the index arithmetic that the kernels of qttt_replay_priority_kernels.h share with the host, the quantiser,
// and the argument checks of include/qttt_replay_priority.h in the order that header promises.  Kept apart from the
// kernels so that a stand-alone program can exercise this code under the host sanitizers (tools/priority_host_check.cpp).
#ifndef QTTT_REPLAY_PRIORITY_HOST_H
#define QTTT_REPLAY_PRIORITY_HOST_H
#include "qttt_checks.h"
#include "qttt_replay_host.h"
#include "qttt_replay_priority.h"

namespace {

// Level 0 (u32 per slot) and the sum levels (u64 per block of the level below) behind the header, each at a 64-byte-aligned
// offset.  n[0] = capacity, n[k] = ceil(n[k - 1] / SCAN_BLOCK); `levels` sum levels, the last with one entry.
struct PriorityLayout {
    int levels;
    int64_t n[QTTT_PRIORITY_MAX_LEVELS + 1], off[QTTT_PRIORITY_MAX_LEVELS + 1];
    int64_t bytes;
};
inline PriorityLayout priority_layout(int64_t capacity) {
    PriorityLayout l = {};
    int64_t at = QTTT_PRIORITY_HEADER_BYTES, n = capacity;
    l.n[0] = n;
    l.off[0] = at;
    at += replay_align64(4 * n);
    int k = 0;
    while (k < QTTT_PRIORITY_MAX_LEVELS) {
        ++k;
        n = (n + QTTT_REPLAY_SCAN_BLOCK - 1) / QTTT_REPLAY_SCAN_BLOCK;
        l.n[k] = n;
        l.off[k] = at;
        at += replay_align64(8 * n);
        if (n <= 1) break;
    }
    l.levels = k;
    l.bytes = at;
    return l;
}

// The table's header as the kernels read it.
constexpr int64_t PRIORITY_SEEN_WORD = 0;         // u64 index
constexpr int64_t PRIORITY_PMAX_WORD = 2;         // u32 index (byte 8)
QTTT_REPLAY_HD inline uint32_t priority_pmax(uint32_t stored) { return stored ? stored : (uint32_t)QTTT_PRIORITY_ONE; }

// The sum launch of level k -> k + 1: one workgroup of SCAN_BLOCK lanes per entry of level k + 1; lane t of workgroup b
// reads entry b * SCAN_BLOCK + t of level k when that is below n[k].
QTTT_REPLAY_HD inline int64_t priority_child(int64_t block, uint32_t t) { return block * QTTT_REPLAY_SCAN_BLOCK + (int64_t)t; }

// Sync: is slot s < capacity one that a sample number in [max(seen, written - capacity), written) lives in?
QTTT_REPLAY_HD inline bool priority_slot_is_new(uint64_t s, uint64_t seen, uint64_t written, uint64_t capacity) {
    const uint64_t F = written < capacity ? written : capacity;
    if (s >= F || seen >= written) return false;
    return replay_holder(s, written, capacity) >= seen;         // the holder is >= written - capacity by construction
}

// The guard of qttt_replay_priority_update.
QTTT_REPLAY_HD inline bool priority_entry_passes(int32_t slot, int64_t number, uint64_t seen, uint64_t written, uint64_t capacity) {
    const uint64_t F = written < capacity ? written : capacity;
    if (slot < 0 || (uint64_t)slot >= F) return false;
    return replay_holder((uint64_t)slot, written, capacity) == (uint64_t)number && (uint64_t)number < seen;
}

// Q(p): the product with 2^16 is exact in f64, so rint (to nearest even) sees the real product.
QTTT_REPLAY_HD inline uint32_t priority_quantise(float p) {
    if (!(p > 0.0f)) return 1u;                                  // p <= 0 and NaN
    const double x = __builtin_rint((double)p * 65536.0);        // +inf stays +inf
    if (x < 1.0) return 1u;
    if (x >= 4294967295.0) return 0xFFFFFFFFu;
    return (uint32_t)x;
}

// One step of the descent on the host: among `count` children (sums c[0..count)), the first whose running sum passes t;
// t loses the sum of the children before it.  The kernels do this with a wave scan; this is what they must agree with.
template <typename T>
inline int64_t priority_first_past(const T *c, int64_t count, uint64_t &t) {
    uint64_t run = 0;
    for (int64_t j = 0; j < count; ++j) {
        if (run + (uint64_t)c[j] > t) {
            t -= run;
            return j;
        }
        run += (uint64_t)c[j];
    }
    t = 0;                                                       // a table out of sync: stay inside the block
    return count - 1;
}

// The checks of qttt_replay_priority_sync.
inline int priority_sync_check(const void *replay, const void *prio, int64_t capacity) {
    if (replay_capacity_bad(capacity)) return QTTT_ERR_SIZE;
    if (!replay || !prio) return QTTT_ERR_NULL;
    if (misaligned(replay, 64) || misaligned(prio, 64)) return QTTT_ERR_ACTION;
    return 0;
}

// The checks of qttt_replay_priority_update; launch = there is device work to do.
inline int priority_update_check(const void *replay, const void *prio, int64_t capacity, int64_t n, const int32_t *slot,
                                 const int64_t *number, const float *priority, bool &launch) {
    launch = false;
    if (replay_capacity_bad(capacity) || n < 0 || n > QTTT_REPLAY_MAX_CAPACITY) return QTTT_ERR_SIZE;
    if (n == 0) return 0;
    if (!replay || !prio || !slot || !number || !priority) return QTTT_ERR_NULL;
    if (misaligned(replay, 64) || misaligned(prio, 64) || misaligned(number, 8) ||
        misaligned(slot, 4) || misaligned(priority, 4))
        return QTTT_ERR_ACTION;
    launch = true;
    return 0;
}

// The checks of qttt_replay_sample_prioritized: replay_sample_check's, with prio beside replay and the three new outputs.
inline int priority_sample_check(const void *replay, const void *prio, int64_t capacity, int64_t n, uint32_t draw,
                                 const float *s_out, const double *pi_out, const uint8_t *mask_out, const float *v_out,
                                 const uint8_t *done_out, const int32_t *index_out, const int64_t *number_out,
                                 const uint32_t *q_out, const uint64_t *total_out, bool &launch) {
    launch = false;
    if (replay_capacity_bad(capacity) || n < 0 || n > QTTT_REPLAY_MAX_CAPACITY || draw >= 0x80000000u) return QTTT_ERR_SIZE;
    if (n == 0) return 0;
    if (!replay || !prio || !s_out || !pi_out || !mask_out || !v_out || !done_out) return QTTT_ERR_NULL;
    if (misaligned(replay, 64) || misaligned(prio, 64) || misaligned(s_out, 16) ||
        misaligned(pi_out, 16) || misaligned(mask_out, 4) || misaligned(v_out, 4) ||
        misaligned(index_out, 4) || misaligned(number_out, 8) || misaligned(q_out, 4) ||
        misaligned(total_out, 8))
        return QTTT_ERR_ACTION;
    launch = true;
    return 0;
}

}  // namespace

#endif  // QTTT_REPLAY_PRIORITY_HOST_H
