/* qttt_replay_priority.h — prioritised replay on the device (Schaul et al., "Prioritized Experience Replay"; the replay
 * MuZero trains from): a priority per slot of the replay ring, a proportional draw in one launch, and a guarded
 * write-back of new priorities.  Part of the C ABI of libqttt_hip.so (additive entries of
 * QTTT_ABI_VERSION 6; included by qttt.h after qttt_replay_reanalyse.h; the conventions of qttt_replay.h hold here:
 * device pointers owned by the caller, work enqueued on `stream`, 0 / hipError_t / negative argument error, no call waits
 * for the device, and no kernel waits on another workgroup's store).  The importance weights that go with a prioritised
 * draw enter the loss through qttt_train_gradients_weighted (qttt_train_weighted.h).
 *
 * Priorities are unsigned fixed-point integers, the real priority times QTTT_PRIORITY_ONE = 2^16, and every sum is a
 * u64: the slot drawn is a pure integer function of (seed, draw, i, table), whatever the order of summation and the
 * shape of the launches.
 *
 * ---- The table.  `prio` is the caller's buffer of qttt_replay_priority_bytes(capacity) bytes, 64-byte aligned, SEPARATE
 * from the ring (the ring's bytes are what they were), for the same `capacity`.  A zero-filled buffer is a fresh table.
 *   0            a 64-byte header: u64 seen at byte 0, every sample number below it has been given a priority; u32 pmax at
 *                byte 8, the largest priority ever stored, 0 read as QTTT_PRIORITY_ONE; the rest is 0
 *   offsets[0]   level 0: u32 q[capacity], the priority of every slot: 1 .. 2^32 - 1 for a slot that holds a sample that
 *                has been given one, 0 for every other slot
 *   offsets[k]   level k = 1 .. levels: u64 sums of blocks of QTTT_REPLAY_SCAN_BLOCK (256) entries of the level below, the
 *                last block short; n_0 = capacity, n_k = ceil(n_(k-1) / 256), and the last level is the first with one
 *                entry, the total T.  capacity <= 256: one sum level; <= 65 536: two; <= 2^24: three; else four
 *                (QTTT_PRIORITY_MAX_LEVELS).  T < 2^30 * 2^32 = 2^62.
 * every array at a 64-byte-aligned offset, in this order, without overlap.  qttt_replay_priority_bytes returns the size
 * or QTTT_ERR_SIZE for a capacity outside 1..QTTT_REPLAY_MAX_CAPACITY.  qttt_replay_priority_layout writes
 * 1 + QTTT_PRIORITY_MAX_LEVELS offsets (HOST memory; 0 for a level the capacity does not have) and returns the number of
 * sum levels (1..4), QTTT_ERR_SIZE for a capacity out of range (checked first) or QTTT_ERR_NULL for a null `offsets`.
 * Both are host-callable and do no device work.
 *
 * ---- qttt_replay_priority_sync.  Gives every sample appended since the last sync the largest priority seen, and
 * rebuilds the sums.  It reads `written` from the ring's header and nothing else of the ring (a 64-byte header alone is a
 * valid `replay` here).  Every sample number w in [max(seen, written - capacity), written) gets q[w % capacity] = pmax
 * (read as above); then seen = written and every sum level is rebuilt from the level below.  pmax itself is not written.
 * 1 + levels launches that the stream orders: the first assigns and sums level 0, the last writes `seen`.  A second call
 * without an append in between changes no byte.
 *   Errors, in this order, before any device work: QTTT_ERR_SIZE for capacity outside 1..QTTT_REPLAY_MAX_CAPACITY;
 * QTTT_ERR_NULL for a null replay or prio; QTTT_ERR_ACTION for replay or prio not 64-byte aligned.
 *
 * ---- qttt_replay_priority_update.  Writes new priorities for n draws: slot i32[n], number i64[n] (the sample number the
 * slot held when it was drawn), priority f32[n]; updated_out u8[n], nullable, receives 1 where entry i passed, else 0.
 * Entry i passes iff 0 <= slot[i] < F, holder(slot[i], written) == number[i] and number[i] < seen: the guard of
 * qttt_replay_update, so a slot appended over since the draw keeps the newcomer's priority.  The stored value is
 *   Q(p) = min(max(rint(p * 2^16), 1), 2^32 - 1) for a finite p > 0, rint to nearest even (the product taken exactly);
 *          1 for p <= 0 or NaN; 2^32 - 1 for +inf.
 * Duplicates are allowed (a minibatch draws with replacement): a slot addressed by several passing entries receives the
 * LARGEST of their Q, a rule with no order in it; a slot addressed by no passing entry keeps its value.  pmax becomes
 * the maximum of itself (read as above) and every stored value.  Then every sum level is rebuilt.  2 + levels launches:
 * the passing entries clear their slots; they raise them with atomicMax on u32 (the only atomics, integer ones); the sums.
 *   Errors, in this order, before any device work: QTTT_ERR_SIZE for capacity outside 1..QTTT_REPLAY_MAX_CAPACITY or n
 * outside 0..QTTT_REPLAY_MAX_CAPACITY; 0 with no device work for n == 0; QTTT_ERR_NULL for a null replay, prio, slot,
 * number or priority; QTTT_ERR_ACTION for replay or prio not 64-byte, number not 8-byte, or slot or priority not 4-byte
 * aligned.
 *
 * ---- qttt_replay_sample_prioritized.  qttt_replay_sample with the slot drawn in proportion to its priority, ONE launch.
 * The table must be in sync with the ring (qttt_replay_priority_sync after the last append): that is the caller's duty.
 * With T the top total, sample i takes
 *   t = mulhi64(qttt_hash(seed, i, draw), T)   and   slot = the smallest s with q[0] + ... + q[s] > t,
 * found by a descent through the sum levels, a wavefront per sample.  A slot with priority 0 is never drawn.  The
 * symmetry draw, the rows, the alignments and the order of the errors are qttt_replay_sample's, word for word (prio is
 * checked where replay is: null, then 64-byte alignment; number_out must be 8-byte, q_out 4-byte and total_out 8-byte
 * aligned, QTTT_ERR_ACTION).  Outputs beyond that entry's, each nullable:
 *   number_out i64[n]  the sample number the slot holds          q_out u32[n]  q[slot]
 *   total_out  u64[1]  T
 * With T == 0 every output row is zero, index_out and number_out are -1 and q_out is 0, as an empty ring gives. */
#ifndef QTTT_REPLAY_PRIORITY_H
#define QTTT_REPLAY_PRIORITY_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QTTT_PRIORITY_ONE (1 << 16)
#define QTTT_PRIORITY_HEADER_BYTES 64
#define QTTT_PRIORITY_MAX_LEVELS 4

int64_t qttt_replay_priority_bytes(int64_t capacity);
int qttt_replay_priority_layout(int64_t capacity, int64_t *offsets);

int qttt_replay_priority_sync(const void *replay, void *prio, int64_t capacity, void *stream);

int qttt_replay_priority_update(const void *replay, void *prio, int64_t capacity, int64_t n, const int32_t *slot,
                                const int64_t *number, const float *priority, uint8_t *updated_out, void *stream);

int qttt_replay_sample_prioritized(const void *replay, const void *prio, int64_t capacity, int64_t n, uint64_t seed,
                                   uint32_t draw, const uint8_t *sym, int random_symmetry, float *s_out, double *pi_out,
                                   uint8_t *mask_out, float *v_out, uint8_t *done_out, int32_t *index_out, uint8_t *sym_out,
                                   int64_t *number_out, uint32_t *q_out, uint64_t *total_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif
