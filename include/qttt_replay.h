/* qttt_replay.h — the replay buffer on the device: a ring of training samples that self-play batches are appended to
 * and minibatches are drawn from, with an optional random symmetry per sample.  Part of the C ABI of
 * libqttt_hip.so (additive entries of QTTT_ABI_VERSION 6; included by qttt.h after qttt_tree_gumbel.h; the conventions
 * of qttt_selfplay.h and qttt_symmetry.h hold here: device pointers owned by the caller, work enqueued on `stream`,
 * 0 / hipError_t / negative argument error, and no call waits for the device).  Loss, gradients and the optimiser are
 * not here: the sample's outputs are the trainer's tensors.
 *
 * ---- The ring.  `replay` is the caller's buffer of qttt_replay_bytes(capacity) bytes, 64-byte aligned, for `capacity`
 * samples, 1 <= capacity <= QTTT_REPLAY_MAX_CAPACITY.  A zero-filled buffer is an empty ring.  Byte offsets:
 *   0            a 64-byte header whose first word is u64 written, the number of samples ever appended (the rest is 0)
 *   offsets[0]   P    u64[capacity]      plane P of the sample's packed state
 *   offsets[1]   Q    u64[capacity]      plane Q
 *   offsets[2]   pi   f64[capacity, 36]  the policy target
 *   offsets[3]   mask u64[capacity]      bit a = (the row's mask[a] != 0); the terminal row's 36 ones are 36 set bits
 *   offsets[4]   v    f32[capacity]      the value target
 *   offsets[5]   done u8[capacity]       the row's done byte
 * every array at a 64-byte-aligned offset, in this order, without overlap.  qttt_replay_bytes and qttt_replay_layout are
 * host-callable and do no device work: qttt_replay_bytes returns the size or QTTT_ERR_SIZE for a capacity out of range;
 * qttt_replay_layout writes the six offsets (HOST memory) and returns 0, QTTT_ERR_SIZE for a capacity out of range (checked
 * first) or QTTT_ERR_NULL for a null `offsets`.  Sample number w of all that were ever appended lives in slot
 * w % capacity; the ring holds the last F = min(written, capacity) of them.
 *
 * ---- qttt_replay_append.  Takes a self-play batch of `games` games (the buffers of qttt_selfplay_record: states, pi,
 * mask, done, v, length) and appends its samples.  The samples are the rows t < min(length[g], QTTT_SELFPLAY_ROWS) of every
 * game, game-major: g ascending, then t ascending (the order of the reference's batch, self_play.py:200-216).  With n of
 * them, sample number r goes to slot (written + r) % capacity and afterwards written += n; if n > capacity the first
 * n - capacity samples are skipped, so no two lanes ever store to one slot.  The two state words, the eight bytes of every
 * pi entry, the four of v and the done byte are moved, never recomputed (a NaN row survives).  The batch is read only.
 *   The ranks come from a device-wide exclusive scan of the clamped lengths, done as separate launches that the stream
 * orders: level 0 scans blocks of QTTT_REPLAY_SCAN_BLOCK games and writes one total per block, level k + 1 scans the
 * totals of level k the same way, until one total is left (games <= 256: one scan launch, <= 65 536: two, <= 2^24: three,
 * else four); then one launch moves the samples, a wave per game, adding up its game's prefix over the levels, and one
 * lane of it writes the header.  No atomic counter, and no kernel waits on another workgroup's store.  `scratch` is the
 * caller's buffer of qttt_replay_append_scratch_bytes(games) bytes (host-callable; QTTT_ERR_SIZE for games out of range),
 * 8-byte aligned, used by this call only; calls that share a scratch buffer must be ordered by their streams.
 *   Errors, in this order, before any device work: QTTT_ERR_SIZE for capacity outside 1..QTTT_REPLAY_MAX_CAPACITY or games
 * outside 0..QTTT_REPLAY_MAX_GAMES; 0 with no device work for games == 0; QTTT_ERR_NULL for any null buffer;
 * QTTT_ERR_ACTION for replay not 64-byte, states not 16-byte, pi or scratch not 8-byte or v not 4-byte aligned.
 *
 * ---- qttt_replay_sample.  Draws a minibatch of n samples, ONE launch.  With F = min(written, capacity) read from the
 * header on the device, sample i takes
 *   slot = mulhi64(qttt_hash(seed, i, draw), F), the high 64 bits of the 128-bit product,
 * and its symmetry k is sym[i] when `sym` (u8[n], device) is given, a value past 7 taken as the identity as qttt_transform
 * does; else qttt_hash(seed, i, draw | 2^31) >> 61 when random_symmetry != 0; else 0.  draw < 2^31: the caller counts its
 * calls.  Outputs, with sigma_k / tau_k of qttt_symmetry.h:
 *   s_out    f32[n, 18, 10]  s_out[i, sigma_k(v), :] = row v of GameState.to_vector (mcts.py:67-85, as qttt_encode) of the
 *                            stored state, and s_out[i, 9 + sigma_k(v), :] = its row 9 + v: the encoding of the state's
 *                            image under k (qttt_transform), which is the encoding with its square blocks permuted
 *   pi_out   f64[n, 36]      pi_out[i, tau_k(a)] = pi[slot, a], the eight bytes moved
 *   mask_out u8[n, 36]       mask_out[i, tau_k(a)] = bit a of the stored mask, 0 or 1
 *   v_out    f32[n]          the four bytes moved        done_out u8[n]   1 where the stored byte is not 0, else 0
 *   index_out i32[n], nullable: slot                     sym_out  u8[n], nullable: k (0 for a sym[i] past 7)
 * With F == 0 every output row is zero and index_out is -1.
 *   Errors, in this order, before any device work: QTTT_ERR_SIZE for capacity outside 1..QTTT_REPLAY_MAX_CAPACITY, n
 * outside 0..QTTT_REPLAY_MAX_CAPACITY or draw >= 2^31; 0 with no device work for n == 0; QTTT_ERR_NULL for a null replay,
 * s_out, pi_out, mask_out, v_out or done_out; QTTT_ERR_ACTION for replay not 64-byte, s_out or pi_out not 16-byte (the
 * tiles leave as 16-byte stores), or mask_out, v_out or index_out not 4-byte aligned.
 *
 * ---- Reanalysis.  qttt_replay_gather (a window of consecutive slots as a state buffer, with the sample number each slot
 * holds) and qttt_replay_update (refreshed pi / v written back into those slots, unless a later append went over them or
 * the row is terminal) work on this ring and are declared in qttt_replay_reanalyse.h, which qttt.h includes as well. */
#ifndef QTTT_REPLAY_H
#define QTTT_REPLAY_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QTTT_REPLAY_MAX_CAPACITY (1 << 30)
#define QTTT_REPLAY_MAX_GAMES (1 << 30)
#define QTTT_REPLAY_HEADER_BYTES 64
#define QTTT_REPLAY_SCAN_BLOCK 256     /* games (or totals) per workgroup of one scan level */

int64_t qttt_replay_bytes(int64_t capacity);
int qttt_replay_layout(int64_t capacity, int64_t *offsets);
int64_t qttt_replay_append_scratch_bytes(int64_t games);

int qttt_replay_append(void *replay, int64_t capacity, int64_t games, const void *states, const double *pi,
                       const uint8_t *mask, const uint8_t *done, const float *v, const uint8_t *length, void *scratch,
                       void *stream);

int qttt_replay_sample(const void *replay, int64_t capacity, int64_t n, uint64_t seed, uint32_t draw, const uint8_t *sym,
                       int random_symmetry, float *s_out, double *pi_out, uint8_t *mask_out, float *v_out,
                       uint8_t *done_out, int32_t *index_out, uint8_t *sym_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif
