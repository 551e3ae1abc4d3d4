"""A numpy model of the replay ring (include/qttt_replay.h), for the tests: the ring with wrap and skip, the draw
streams from the library's host-callable qttt_hash with Python integers, and the permutation of a sample by the tables of
qtttgym_amd.symmetry.  Nothing here runs on a device."""
import ctypes

import numpy as np

from qtttgym_amd import _native, symmetry

ROWS = _native.SELFPLAY_ROWS
MASK64 = (1 << 64) - 1


def layout(capacity):
    """({name: byte offset}, bytes) of a ring of `capacity` samples, from the library."""
    L = _native.lib()
    off = (ctypes.c_int64 * 6)()
    assert L.qttt_replay_layout(capacity, off) == 0
    return dict(zip(_native.REPLAY_ARRAYS, off)), int(L.qttt_replay_bytes(capacity))


# ---------------------------------------------------------------- the draw streams
def slot_stream(seed, draw, n, filled):
    """The slot of samples 0..n-1 of sample() call `draw`: mulhi64(qttt_hash(seed, i, draw), filled)."""
    h = _native.lib().qttt_hash
    return [(int(h(seed, i, draw)) * filled) >> 64 for i in range(n)]


def symmetry_stream(seed, draw, n):
    """Their random symmetries: qttt_hash(seed, i, draw | 2^31) >> 61."""
    h = _native.lib().qttt_hash
    return [int(h(seed, i, draw | (1 << 31))) >> 61 for i in range(n)]


# ---------------------------------------------------------------- the ring
class Ring:
    """The ring's arrays as words: P, Q, mask u64[cap], pi u64[cap, 36] (the doubles' bits), v u32[cap] (the floats'
    bits), done u8[cap], and `written`."""

    def __init__(self, capacity):
        C = self.capacity = int(capacity)
        self.written = 0
        self.P, self.Q, self.mask = (np.zeros(C, np.uint64) for _ in range(3))
        self.pi = np.zeros((C, 36), np.uint64)
        self.v = np.zeros(C, np.uint32)
        self.done = np.zeros(C, np.uint8)

    @property
    def filled(self):
        return min(self.written, self.capacity)

    def append(self, states, pi, mask, done, v, length):
        """A batch as numpy arrays of the SelfPlayBatch's tensors: states u8[10, state bytes], pi f64[10, G, 36], mask
        u8[10, G, 36], done u8[10, G], v f32[10, G], length u8[G].  Returns the number of samples of the batch."""
        G = len(length)
        stride = (G + 63) // 64 * 64
        planes = np.ascontiguousarray(states).view(np.uint64).reshape(ROWS, 2, stride)
        rows = np.minimum(length.astype(np.int64), ROWS)
        live = (np.arange(ROWS)[None, :] < rows[:, None])                    # [G, 10], game-major
        g, t = np.nonzero(live)
        n = len(g)
        bits = ((mask[t, g] != 0).astype(np.uint64) << np.arange(36, dtype=np.uint64)[None, :]).sum(1, dtype=np.uint64)
        src = {"P": planes[t, 0, g], "Q": planes[t, 1, g], "pi": np.ascontiguousarray(pi).view(np.uint64)[t, g], "mask": bits,
               "v": np.ascontiguousarray(v).view(np.uint32)[t, g], "done": done[t, g]}
        skip = max(n - self.capacity, 0)                                     # the first n - capacity samples go nowhere
        slots = (self.written + np.arange(skip, n)) % self.capacity
        assert len(set(slots.tolist())) == len(slots)                        # no slot is stored to twice
        for k, a in src.items():
            getattr(self, k)[slots] = a[skip:]
        self.written += n
        return n


def batch_arrays(batch):
    """A SelfPlayBatch's tensors as the numpy arrays Ring.append takes."""
    return tuple(getattr(batch, k).cpu().numpy() for k in ("states", "pi", "mask", "done", "v", "length"))


# ---------------------------------------------------------------- the permutation
def permute(s, pi, mask, ks):
    """Samples (s [n, 18, 10], pi [n, 36], mask [n, 36]) under the symmetries ks [n]: the square blocks of s moved by
    sigma, the entries of pi and mask by tau (qtttgym_amd.symmetry's tables)."""
    cells, actions = np.array(symmetry.CELLS), np.array(symmetry.ACTIONS)
    s2, pi2, mask2 = np.empty_like(s), np.empty_like(pi), np.empty_like(mask)
    for i, k in enumerate(ks):
        s2[i, cells[k]] = s[i, :9]
        s2[i, 9 + cells[k]] = s[i, 9:]
        pi2[i, actions[k]] = pi[i]
        mask2[i, actions[k]] = mask[i]
    return s2, pi2, mask2
