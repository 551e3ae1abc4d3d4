/* qttt_replay_reanalyse.h — reanalysis of the replay ring: take a window of the ring's positions out as a
 * state buffer, so that they can be searched again with the current network, and write the refreshed targets back into
 * their slots, guarded against the ring having moved on in between.  Part of the C ABI of libqttt_hip.so (additive
 * entries of QTTT_ABI_VERSION 6; included by qttt.h after qttt_selfplay_exact.h; the ring, its layout and the conventions
 * are qttt_replay.h's: device pointers owned by the caller, work enqueued on `stream`, 0 / hipError_t / negative argument
 * error, and no call waits for the device).  The search between the two calls is the caller's: qttt_tree_reset takes the
 * gathered state buffer, qttt_selfplay_record turns the searched roots into pi.
 *
 * ---- Shared by both entries.  `written` is the header's first word as the kernel reads it, F = min(written, capacity).
 * The sample number held by slot s < F is
 *   holder(s, written) = written - 1 - ((written - 1 - s) mod capacity),
 * the largest w < written with w mod capacity == s (qttt_replay.h: sample number w lives in slot w % capacity).  Both
 * kernels read `written` on the device; neither waits for the host, takes an atomic or writes the header.
 *
 * ---- qttt_replay_gather.  A window of n consecutive slots as a state buffer, ONE launch.  Sample i takes slot
 * (s0 + i) mod F when i < F and no slot otherwise, where s0 = start mod F when start >= 0, and else
 *   s0 = mulhi64(qttt_hash(seed, QTTT_REPLAY_WINDOW_ID, draw), F).
 * No minibatch index reaches the board id 2^32, so the window's draw is none of qttt_replay_sample's slot or symmetry
 * draws.  Consecutive slots: a window holds no slot twice, so the update below never has two writers to one slot, and a
 * refresh sweep, unlike an SGD minibatch, has no need of decorrelated samples.  Outputs:
 *   state_out  qttt_state_bytes(n) bytes, planes P / Q at the plane stride of n: the state buffer of n boards.  Board i gets
 *              the two stored words of its slot, moved; a sample without a slot — and the padding behind board n - 1 — the
 *              words qttt_reset gives a board
 *   slot_out   i32[n]  the slot, or -1              number_out i64[n]  holder(slot, written), or -1
 *   v_out      f32[n], nullable: the four stored bytes, or 0
 *   done_out   u8[n], nullable: the stored byte, or 0
 * An empty ring (F == 0) gives every sample no slot.  The ring is read only.
 *   Errors, in this order, before any device work: QTTT_ERR_SIZE for capacity outside 1..QTTT_REPLAY_MAX_CAPACITY, n
 * outside 0..QTTT_REPLAY_MAX_CAPACITY or draw >= 2^31; 0 with no device work for n == 0; QTTT_ERR_NULL for a null replay,
 * state_out, slot_out or number_out; QTTT_ERR_ACTION for replay not 64-byte, state_out not 16-byte, number_out not 8-byte,
 * or slot_out or v_out not 4-byte aligned.
 *
 * ---- qttt_replay_update.  Writes refreshed targets back, ONE launch.  Sample i is written iff slot[i] >= 0, slot[i] < F,
 * holder(slot[i], written) == number[i] (nothing has been appended over it since the gather) and the slot's stored done
 * byte is 0.  Then the 36 eight-byte words of pi[i] (f64[n, 36], nullable) are moved into the slot's pi row — a NaN with a
 * payload survives — and the four bytes of v[i] (f32[n], nullable) into the slot's v; at least one of the two must be
 * given.  updated_out[i] (u8[n], nullable) is 1 when written and 0 otherwise.  No other byte of the ring changes: states,
 * masks, done bytes, the header and every unaddressed slot stay.  The non-negative values of `slot` must be distinct, as
 * a gather's are: then no two lanes store to one slot.
 *   Errors, in this order, before any device work: QTTT_ERR_SIZE for capacity outside 1..QTTT_REPLAY_MAX_CAPACITY or n
 * outside 0..QTTT_REPLAY_MAX_CAPACITY; 0 with no device work for n == 0; QTTT_ERR_NULL for a null replay, slot or number, or
 * for pi and v both null; QTTT_ERR_ACTION for replay not 64-byte, pi or number not 8-byte, or slot or v not 4-byte
 * aligned. */
#ifndef QTTT_REPLAY_REANALYSE_H
#define QTTT_REPLAY_REANALYSE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QTTT_REPLAY_WINDOW_ID 0x100000000ull   /* the board id of the window's draw: 2^32 */

int qttt_replay_gather(const void *replay, int64_t capacity, int64_t n, uint64_t seed, uint32_t draw, int64_t start,
                       void *state_out, int32_t *slot_out, int64_t *number_out, float *v_out, uint8_t *done_out,
                       void *stream);

int qttt_replay_update(void *replay, int64_t capacity, int64_t n, const int32_t *slot, const int64_t *number,
                       const double *pi, const float *v, uint8_t *updated_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif
