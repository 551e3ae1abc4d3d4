"""A numpy / Python-integer model of include/qttt_replay_reanalyse.h, for the tests: the window (its hashed start through
the library's host-callable qttt_hash), holder, the gather's outputs over the ring's arrays, and the update's guard and
byte moves over an image of the ring's arrays.  Nothing here runs on a device."""
import numpy as np

from qtttgym_amd import _native

WINDOW_ID = 1 << 32


def holder(s, written, capacity):
    """The sample number slot s < min(written, capacity) holds."""
    return written - 1 - ((written - 1 - s) % capacity)


def window(n, written, capacity, start=None, seed=0, draw=0):
    """The slots of samples 0..n-1 (-1: no slot): n consecutive slots from s0, modulo F."""
    F = min(written, capacity)
    if F == 0:
        return [-1] * n
    if start is None or start < 0:
        s0 = (int(_native.lib().qttt_hash(seed, WINDOW_ID, draw)) * F) >> 64
    else:
        s0 = start % F
    return [(s0 + i) % F if i < F else -1 for i in range(n)]


def gather(arrays, written, capacity, n, start=None, seed=0, draw=0):
    """The gather's outputs over the ring's arrays (P, Q u64 / i64[cap], v word array [cap], done u8[cap]): state (2 x
    stride words: planes P / Q, zeros for a sample without a slot and in the padding), slot i32[n], number i64[n], v words
    [n], done u8[n]."""
    slots = window(n, written, capacity, start, seed, draw)
    stride = (n + 63) // 64 * 64
    state = np.zeros(2 * stride, np.uint64)
    v = np.zeros(n, np.uint32)
    done = np.zeros(n, np.uint8)
    number = np.full(n, -1, np.int64)
    for i, s in enumerate(slots):
        if s < 0:
            continue
        state[i], state[stride + i] = arrays["P"].view(np.uint64)[s], arrays["Q"].view(np.uint64)[s]
        v[i], done[i] = arrays["v"].view(np.uint32)[s], arrays["done"][s]
        number[i] = holder(s, written, capacity)
    return state, np.array(slots, np.int32), number, v, done


def update(arrays, written, capacity, slot, number, pi=None, v=None):
    """Applies the update to `arrays` in place (pi u64[cap, 36] words, v u32[cap] words, done u8[cap]); pi u64[n, 36] and v
    u32[n] words or None.  Returns updated u8[n]."""
    F = min(written, capacity)
    updated = np.zeros(len(slot), np.uint8)
    for i, (s, w) in enumerate(zip(slot.tolist(), number.tolist())):
        if s < 0 or s >= F or holder(s, written, capacity) != w or arrays["done"][s] != 0:
            continue
        if pi is not None:
            arrays["pi"][s] = pi[i]
        if v is not None:
            arrays["v"][s] = v[i]
        updated[i] = 1
    return updated
