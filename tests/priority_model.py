"""A numpy / Python-integer model of include/qttt_replay_priority.h, for the tests: the table (sync, the quantiser, the
guarded update with its max rule, the sums), the slot rule of the prioritised draw and ReplayBuffer.weights.  Every sum
is a Python integer or a u64; nothing here runs on a device."""
import ctypes
import math

import numpy as np

from qtttgym_amd import _native

ONE = _native.PRIORITY_ONE
BLOCK = _native.REPLAY_SCAN_BLOCK
QMAX = (1 << 32) - 1


def layout(capacity):
    """(offsets of level 0 and of every sum level, bytes) of the table, from the library."""
    L = _native.lib()
    off = (ctypes.c_int64 * (_native.PRIORITY_MAX_LEVELS + 1))()
    levels = L.qttt_replay_priority_layout(capacity, off)
    assert 1 <= levels <= _native.PRIORITY_MAX_LEVELS
    assert all(o == 0 for o in list(off)[levels + 1:])
    return list(off)[:levels + 1], int(L.qttt_replay_priority_bytes(capacity))


def level_sizes(capacity):
    """n_0 = capacity, n_k = ceil(n_(k-1) / 256), down to the first level of one entry."""
    n = [capacity]
    while True:
        n.append(-(-n[-1] // BLOCK))
        if n[-1] == 1:
            return n


def holder(s, written, capacity):
    """The sample number slot s < min(written, capacity) holds."""
    return written - 1 - (written - 1 - s) % capacity


def quantise(p):
    """Q(p) of one float32 value: the real product with 2^16 rounded to nearest even, clamped to 1..2^32-1."""
    p = float(np.float32(p))
    if not p > 0.0:                                             # p <= 0 and NaN
        return 1
    if math.isinf(p):
        return QMAX
    x = p * 65536.0                                             # exact in f64 for every float32
    r = math.floor(x)
    frac = x - r
    if frac > 0.5 or (frac == 0.5 and r % 2 == 1):
        r += 1
    return min(max(int(r), 1), QMAX)


class Table:
    """seen, pmax (as stored: 0 until an update passes) and q u32[capacity]; sums() builds the levels."""

    def __init__(self, capacity):
        self.capacity = int(capacity)
        self.seen, self.pmax = 0, 0
        self.q = np.zeros(self.capacity, np.uint32)

    def sync(self, written):
        C = self.capacity
        p = self.pmax or ONE
        lo = max(self.seen, written - C)
        if written - lo >= C:
            self.q[:] = p
        else:
            w = np.arange(lo, written, dtype=np.int64)
            self.q[w % C] = p
        self.seen = written

    def update(self, written, slot, number, priority):
        """The guarded write-back; returns updated u8[n]."""
        C, F = self.capacity, min(written, self.capacity)
        best = {}
        updated = np.zeros(len(slot), np.uint8)
        for i, (s, w, p) in enumerate(zip(slot.tolist(), number.tolist(), priority.tolist())):
            if 0 <= s < F and holder(s, written, C) == w and w < self.seen:
                updated[i] = 1
                best[s] = max(best.get(s, 0), quantise(p))
        for s, v in best.items():
            self.q[s] = v
        if best:
            self.pmax = max(self.pmax or ONE, max(best.values()))
        return updated

    def sums(self):
        """The sum levels, u64 arrays, the last of one entry."""
        out, cur = [], self.q.astype(np.uint64)
        for n in level_sizes(self.capacity)[1:]:
            pad = np.zeros(n * BLOCK, np.uint64)
            pad[:len(cur)] = cur
            cur = pad.reshape(n, BLOCK).sum(1, dtype=np.uint64)
            out.append(cur)
        return out

    def total(self):
        return int(self.sums()[-1][0])                          # < 2^62: a u64 holds it

    def image(self):
        """The table's bytes as the device must hold them (a u8 array of qttt_replay_priority_bytes).  The bytes between
        the arrays are zero: nothing ever writes them."""
        off, size = layout(self.capacity)
        img = np.zeros(size, np.uint8)
        img[0:8] = np.array([self.seen], np.uint64).view(np.uint8)
        img[8:12] = np.array([self.pmax], np.uint32).view(np.uint8)
        img[off[0]:off[0] + 4 * self.capacity] = self.q.view(np.uint8)
        for o, a in zip(off[1:], self.sums()):
            img[o:o + 8 * len(a)] = a.view(np.uint8)
        return img

    def draw(self, seed, draw, n):
        """(slots, q of the slots, T) of sample() call `draw`: t = mulhi64(qttt_hash(seed, i, draw), T) and the smallest s
        with q[0] + ... + q[s] > t, by a binary search in the running sums."""
        h = _native.lib().qttt_hash
        T = self.total()
        if T == 0:
            return [-1] * n, [0] * n, 0
        cum = np.cumsum(self.q.astype(np.uint64), dtype=np.uint64)
        ts = np.array([(int(h(seed, i, draw)) * T) >> 64 for i in range(n)], np.uint64)
        slots = np.searchsorted(cum, ts, side="right").tolist()
        return slots, [int(self.q[s]) for s in slots], T


def slot_of(q, t):
    """The slot rule alone, by brute force: the smallest s with q[0] + ... + q[s] > t."""
    run = 0
    for s, x in enumerate(q):
        run += int(x)
        if run > t:
            return s
    raise AssertionError("t >= T")


def weights(q, T, filled, beta):
    """ReplayBuffer.weights: (F q / T) ** -beta over its maximum, f64 throughout, rounded to f32 at the end."""
    p = float(filled) * (np.asarray(q, np.float64) / np.float64(T))
    w = p ** (-float(beta))
    return (w / w.max()).astype(np.float32)
