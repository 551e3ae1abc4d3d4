// qttt_replay_host.h — host only, plain C++ without HIP: the layout of the replay ring, the plan of the append's scan
// levels and the argument checks of include/qttt_replay.h, in the order that header promises (on qttt_checks.h).  Kept apart from the
// kernels so that a stand-alone program can exercise this code under the host sanitizers (tools/replay_host_check.cpp).
#ifndef QTTT_REPLAY_HOST_H
#define QTTT_REPLAY_HOST_H
#include "qttt_checks.h"

#ifdef __HIPCC__
#define QTTT_REPLAY_HD __host__ __device__
#else
#define QTTT_REPLAY_HD
#endif

namespace {

inline int64_t replay_align64(int64_t bytes) { return (bytes + 63) & ~(int64_t)63; }
inline bool replay_capacity_bad(int64_t capacity) { return capacity < 1 || capacity > QTTT_REPLAY_MAX_CAPACITY; }
inline bool replay_games_bad(int64_t games) { return games < 0 || games > QTTT_REPLAY_MAX_GAMES; }

// P, Q, pi, mask, v, done behind the header, each at a 64-byte-aligned offset; bytes = the whole ring
struct ReplayLayout {
    int64_t off[6];
    int64_t bytes;
};
inline ReplayLayout replay_layout(int64_t capacity) {
    const int64_t elem[6] = {8, 8, 8 * 36, 8, 4, 1};
    ReplayLayout l;
    int64_t at = QTTT_REPLAY_HEADER_BYTES;
    for (int k = 0; k < 6; ++k) {
        l.off[k] = at;
        at += replay_align64(elem[k] * capacity);
    }
    l.bytes = at;
    return l;
}

// The append's scratch, in u64 words: word 0 = `written` as the first launch found it, words 1..7 unused, then the
// arrays of the scan levels: level k has n[k] entries at word off[k], n[0] = games, n[k + 1] = ceil(n[k] / SCAN_BLOCK),
// down to the one grand total n[levels] = 1.  Level k's launch turns its array into the exclusive prefix inside every
// block and writes the blocks' totals, level k + 1's input.  games <= 2^30, so at most four levels.
constexpr int REPLAY_MAX_LEVELS = 4;
constexpr int64_t REPLAY_SCRATCH_HEAD_WORDS = 8;
struct ReplayScanPlan {
    int levels;
    int64_t n[REPLAY_MAX_LEVELS + 1], off[REPLAY_MAX_LEVELS + 1];
    int64_t words;
};
inline ReplayScanPlan replay_scan_plan(int64_t games) {
    ReplayScanPlan p = {};
    int64_t at = REPLAY_SCRATCH_HEAD_WORDS, n = games;
    int k = 0;
    for (;; ++k) {
        p.n[k] = n;
        p.off[k] = at;
        at += n;
        if (k > 0 && n <= 1) break;
        if (k == REPLAY_MAX_LEVELS) break;                       // (not reached for games <= 2^30)
        n = (n + QTTT_REPLAY_SCAN_BLOCK - 1) / QTTT_REPLAY_SCAN_BLOCK;
    }
    p.levels = k;
    p.words = at;
    return p;
}

// The checks of qttt_replay_append; launch = there is device work to do.
inline int replay_append_check(const void *replay, int64_t capacity, int64_t games, const void *states, const double *pi,
                               const uint8_t *mask, const uint8_t *done, const float *v, const uint8_t *length,
                               const void *scratch, bool &launch) {
    launch = false;
    if (replay_capacity_bad(capacity) || replay_games_bad(games)) return QTTT_ERR_SIZE;
    if (games == 0) return 0;
    if (!replay || !states || !pi || !mask || !done || !v || !length || !scratch) return QTTT_ERR_NULL;
    if (misaligned(replay, 64) || misaligned(states, 16) || misaligned(pi, 8) ||
        misaligned(scratch, 8) || misaligned(v, 4))
        return QTTT_ERR_ACTION;
    launch = true;
    return 0;
}

// The checks of qttt_replay_sample.
inline int replay_sample_check(const void *replay, int64_t capacity, int64_t n, uint32_t draw, const float *s_out,
                               const double *pi_out, const uint8_t *mask_out, const float *v_out, const uint8_t *done_out,
                               const int32_t *index_out, bool &launch) {
    launch = false;
    if (replay_capacity_bad(capacity) || n < 0 || n > QTTT_REPLAY_MAX_CAPACITY || draw >= 0x80000000u) return QTTT_ERR_SIZE;
    if (n == 0) return 0;
    if (!replay || !s_out || !pi_out || !mask_out || !v_out || !done_out) return QTTT_ERR_NULL;
    if (misaligned(replay, 64) || misaligned(s_out, 16) || misaligned(pi_out, 16) ||
        misaligned(mask_out, 4) || misaligned(v_out, 4) || misaligned(index_out, 4))
        return QTTT_ERR_ACTION;
    launch = true;
    return 0;
}

// ---- reanalysis (include/qttt_replay_reanalyse.h): the arithmetic the two kernels and the host program share.
// The sample number that slot s < min(written, capacity) holds: the largest w < written with w % capacity == s.
QTTT_REPLAY_HD inline uint64_t replay_holder(uint64_t s, uint64_t written, uint64_t capacity) {
    return written - 1u - (written - 1u - s) % capacity;
}
// The slot of sample i < F of a window that starts at s0 < F: (s0 + i) mod F without a division.
QTTT_REPLAY_HD inline uint64_t replay_window_slot(uint64_t s0, uint64_t i, uint64_t F) {
    const uint64_t s = s0 + i;
    return s >= F ? s - F : s;
}
// The window's first slot: start mod F when start >= 0, else the high 64 bits of hash * F (hash = the window's draw).
QTTT_REPLAY_HD inline uint64_t replay_window_start(int64_t start, uint64_t hash, uint64_t F) {
    if (start >= 0) return (uint64_t)start % F;
#ifdef __HIP_DEVICE_COMPILE__
    return __umul64hi(hash, F);
#else
    return (uint64_t)(((unsigned __int128)hash * F) >> 64);
#endif
}

// The checks of qttt_replay_gather.
inline int replay_gather_check(const void *replay, int64_t capacity, int64_t n, uint32_t draw, const void *state_out,
                               const int32_t *slot_out, const int64_t *number_out, const float *v_out, bool &launch) {
    launch = false;
    if (replay_capacity_bad(capacity) || n < 0 || n > QTTT_REPLAY_MAX_CAPACITY || draw >= 0x80000000u) return QTTT_ERR_SIZE;
    if (n == 0) return 0;
    if (!replay || !state_out || !slot_out || !number_out) return QTTT_ERR_NULL;
    if (misaligned(replay, 64) || misaligned(state_out, 16) || misaligned(number_out, 8) ||
        misaligned(slot_out, 4) || misaligned(v_out, 4))
        return QTTT_ERR_ACTION;
    launch = true;
    return 0;
}

// The checks of qttt_replay_update.
inline int replay_update_check(const void *replay, int64_t capacity, int64_t n, const int32_t *slot, const int64_t *number,
                               const double *pi, const float *v, bool &launch) {
    launch = false;
    if (replay_capacity_bad(capacity) || n < 0 || n > QTTT_REPLAY_MAX_CAPACITY) return QTTT_ERR_SIZE;
    if (n == 0) return 0;
    if (!replay || !slot || !number || (!pi && !v)) return QTTT_ERR_NULL;
    if (misaligned(replay, 64) || misaligned(pi, 8) || misaligned(number, 8) ||
        misaligned(slot, 4) || misaligned(v, 4))
        return QTTT_ERR_ACTION;
    launch = true;
    return 0;
}

}  // namespace

#endif  // QTTT_REPLAY_HOST_H
