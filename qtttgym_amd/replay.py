"""ReplayBuffer — the window of recent self-play samples an AlphaZero-style trainer draws its minibatches from, on the
device (include/qttt_replay.h): a ring of `capacity` samples that SelfPlayBatches are appended to in
flat()'s order without a host read-back, and that one launch samples from with an optional random symmetry per sample.

    rb = ReplayBuffer(1 << 20)
    rb.add(sp.play())                                     # no host synchronisation
    s, pi, mask, v, done = rb.sample(4096, "random")      # the trainer's tensors, one launch

    window = rb.gather(4096)                              # reanalysis: positions out as a VecEnv ...
    rb.update(window, pi=new_pi)                          # ... and refreshed targets back, unless appended over since

    rb = ReplayBuffer(1 << 20, prioritized=True)          # prioritised replay: slots drawn by priority,
    batch = rb.sample(4096, "random")                     # ... two entries, no read-back ...
    L, J = trainer.step(*batch, weight=rb.weights(1.0))   # ... importance weights in the loss ...
    rb.update_priorities((L + J) ** 0.5)                  # ... and the per-sample loss back as the new priorities

Loss, gradients and the optimiser are ordinary torch or qtttgym_amd.Trainer (examples/selfplay_train.py --replay
[--device-train]).
"""
import ctypes

import torch

from . import _native
from ._host import LibCaller, _ptr, check_tensor, resolve_device
from .selfplay import ROWS, SelfPlayBatch
from .vec_env import VecEnv

_MAX_DRAW = 1 << 31
# the ring's arrays as torch sees them (torch has no arithmetic on uint64: the words travel as int64)
_VIEWS = {"P": (torch.int64, 8, ()), "Q": (torch.int64, 8, ()), "pi": (torch.float64, 8, (36,)),
          "mask": (torch.int64, 8, ()), "v": (torch.float32, 4, ()), "done": (torch.uint8, 1, ())}
_OUT = (("s", torch.float32, (18, 10)), ("pi", torch.float64, (36,)), ("mask", torch.bool, (36,)), ("v", torch.float32, ()),
        ("done", torch.bool, ()))


class ReplayBuffer(LibCaller):
    """A ring of `capacity` training samples in device memory.  add(batch) appends a SelfPlayBatch's samples (the rows
    below every game's length, game-major: flat()'s order); once the ring is full the oldest samples are overwritten.
    sample(n, symmetries) draws n of the samples held, uniformly with replacement, by the counter hash of (seed, the
    number of sample() calls so far): the same seed and call number give the same minibatch.  prioritized=True: the ring
    owns a priority table (include/qttt_replay_priority.h) and sample() draws slot s with probability q[s] / T, the
    fixed-point priorities and their total; a new sample enters at the largest priority stored so far, and
    update_priorities() writes the trainer's per-sample loss back.  The ring's own bytes are the same either way."""

    def __init__(self, capacity, device=None, seed=0, prioritized=False):
        self.capacity, self.seed = int(capacity), int(seed) & (2 ** 64 - 1)
        if not 1 <= self.capacity <= _native.REPLAY_MAX_CAPACITY:
            raise ValueError("capacity must be in 1..%d" % _native.REPLAY_MAX_CAPACITY)
        self._open(resolve_device("cuda" if device is None else device, "ReplayBuffer"))
        offsets = (ctypes.c_int64 * len(_native.REPLAY_ARRAYS))()
        _native.check(self._lib.qttt_replay_layout(self.capacity, offsets), "qttt_replay_layout")
        self.offsets = dict(zip(_native.REPLAY_ARRAYS, offsets))
        self.buffer = torch.zeros(int(self._lib.qttt_replay_bytes(self.capacity)), dtype=torch.uint8, device=self.device)
        self.draw = 0                   # sample() calls so far: the draw index of the next
        self.adds = 0                   # add() calls that appended games
        self.gathers = 0                # gather() calls so far: the draw index of the next window
        self.last_index = self.last_symmetry = None
        self._scratch = None
        self.prioritized = bool(prioritized)
        self.last_number = self.last_priority = self.last_total = None
        if self.prioritized:
            offs = (ctypes.c_int64 * (_native.PRIORITY_MAX_LEVELS + 1))()
            self.priority_levels = self._lib.qttt_replay_priority_layout(self.capacity, offs)
            if self.priority_levels < 1:
                _native.check(self.priority_levels, "qttt_replay_priority_layout")
            self.priority_offsets = list(offs)[:self.priority_levels + 1]
            self.priority = torch.zeros(int(self._lib.qttt_replay_priority_bytes(self.capacity)), dtype=torch.uint8,
                                        device=self.device)

    def views(self):
        """The ring's arrays as views of `buffer` (qttt_replay_layout): written i64[1], P, Q and mask i64[capacity] (the
        u64 words), pi f64[capacity, 36], v f32[capacity], done u8[capacity]."""
        C, out = self.capacity, {"written": self.buffer[:8].view(torch.int64)}
        for name, (dtype, size, shape) in _VIEWS.items():
            at, count = self.offsets[name], C * (36 if shape else 1)
            out[name] = self.buffer[at:at + size * count].view(dtype).view((C,) + shape)
        return out

    def priority_views(self):
        """The priority table's arrays as views of `priority` (qttt_replay_priority_layout): seen i64[1], pmax i32[1] (the
        u32 word), q i32[capacity] (the u32 words) and sums, one i64 tensor per sum level, the last of one entry: T."""
        self._need_priorities("priority_views()")
        n, out = self.capacity, {"seen": self.priority[:8].view(torch.int64), "pmax": self.priority[8:12].view(torch.int32)}
        at = self.priority_offsets[0]
        out["q"] = self.priority[at:at + 4 * n].view(torch.int32)
        out["sums"] = []
        for at in self.priority_offsets[1:]:
            n = -(-n // _native.REPLAY_SCAN_BLOCK)
            out["sums"].append(self.priority[at:at + 8 * n].view(torch.int64))
        return out

    def _need_priorities(self, what):
        if not self.prioritized:
            raise ValueError("%s needs a ring built with prioritized=True" % what)

    def sync_priorities(self):
        """qttt_replay_priority_sync: the samples appended since the last sync get the largest priority stored so far, and
        the sums are rebuilt.  sample() does this itself; no host read-back."""
        self._need_priorities("sync_priorities()")
        self._call("qttt_replay_priority_sync", self.buffer.data_ptr(), self.priority.data_ptr(), self.capacity)

    def weights(self, beta):
        """The importance weights of the last draw, f32[n]: (F q / T) ** -beta divided by its maximum, with q / T the f64
        quotient of the drawn slot's priority and the total, and F the samples held.  Torch ops on device tensors; no host
        read.  What Trainer.step(..., weight=) takes."""
        self._need_priorities("weights()")
        if self.last_priority is None:
            raise ValueError("weights() before any sample()")
        q = (self._last_q.to(torch.int64) & 0xFFFFFFFF).to(torch.float64)
        held = self.views()["written"].clamp(max=self.capacity).to(torch.float64)
        w = (held * (q / self.last_total.to(torch.float64))) ** (-float(beta))
        return (w / w.max()).to(torch.float32)

    def update_priorities(self, priority, index=None, number=None):
        """New priorities (f32[n], the real values: they are stored as fixed point, times 2**16, in 1..2**32-1) for the
        slots `index` (i32[n]) that held the samples `number` (i64[n]) when drawn; both default to the last sample()'s.
        qttt_replay_priority_update: a slot appended over since the draw keeps the newcomer's priority, a slot drawn
        several times receives the largest of its values.  No host read-back.  Returns updated bool[n]."""
        self._need_priorities("update_priorities()")
        if (index is None) != (number is None):
            raise ValueError("give index and number together, or neither for the last draw's")
        if index is None:
            if self.last_number is None:
                raise ValueError("update_priorities() before any sample()")
            index, number = self.last_index, self.last_number
        n, dev = int(index.numel()), self.device
        check_tensor(index, torch.int32, (n,), dev, "index")
        check_tensor(number, torch.int64, (n,), dev, "number")
        check_tensor(priority, torch.float32, (n,), dev, "priority")
        updated = torch.zeros(n, dtype=torch.uint8, device=dev)
        self._call("qttt_replay_priority_update", self.buffer.data_ptr(), self.priority.data_ptr(), self.capacity, n,
                   index.data_ptr(), number.data_ptr(), priority.data_ptr(), updated.data_ptr())
        return updated.view(torch.bool)

    def size(self):
        """Samples held, min(written, capacity).  One host read-back."""
        return min(int(self.views()["written"].item()), self.capacity)

    def add(self, batch, length=None):
        """Appends the samples of a SelfPlayBatch (qttt_replay_append).  No host read-back; the batch is not changed.
        length (u8[G], optional) stands in for batch.length: the rows below length[g] of game g are appended, none of a
        game with 0 (SelfPlay.stream appends the games that finished at a ply this way)."""
        G, dev = batch.num_games, self.device
        check_tensor(batch.states, torch.uint8, (ROWS, int(self._lib.qttt_state_bytes(G))), dev, "batch.states")
        for k in ("pi", "mask", "done", "v"):
            dt, shp = SelfPlayBatch._ROWS[k]
            check_tensor(getattr(batch, k), dt, (ROWS, G) + shp, dev, "batch." + k)
        length = check_tensor(batch.length if length is None else length, torch.uint8, (G,), dev,
                              "batch.length" if length is None else "length")
        if G == 0:
            return
        need = int(self._lib.qttt_replay_append_scratch_bytes(G))
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = torch.empty(need, dtype=torch.uint8, device=dev)
        self._call("qttt_replay_append", self.buffer.data_ptr(), self.capacity, G, batch.states.data_ptr(), batch.pi.data_ptr(),
                   batch.mask.data_ptr(), batch.done.data_ptr(), batch.v.data_ptr(), length.data_ptr(),
                   self._scratch.data_ptr())
        self.adds += 1

    def sample(self, n, symmetries=None, out=None):
        """A minibatch (s f32[n, 18, 10], pi f64[n, 36], mask bool[n, 36], v f32[n], done bool[n]) of samples drawn from
        the ring, one launch (qttt_replay_sample).  symmetries: None = the samples as stored; "random" = every sample
        under a symmetry of its own, drawn by the hash; a uint8 tensor [n] = sample i under symmetries[i] (a value past 7:
        the identity).  out: the five tensors of an earlier call, to be written again.  The slots and symmetries drawn
        are kept as last_index i32[n] and last_symmetry u8[n]; a prioritised ring syncs its table and draws by priority
        (qttt_replay_priority_sync, qttt_replay_sample_prioritized), and keeps last_number i64[n] (the sample number each
        slot held), last_priority u32[n] and last_total i64[1] (T) as well.  Raises before any add() of games: that is the host's count
        of add() calls, because `written` lives on the device and sample() reads nothing back.  What the ring holds is
        decided on the device: after adds whose games all had length 0 the rows are zero and last_index is -1, as the C
        entry gives for an empty ring."""
        n, dev = int(n), self.device
        if n < 0:
            raise ValueError("n must be >= 0")
        if self.adds == 0:
            raise ValueError("sample() before any add(): the ring is empty")
        if self.draw >= _MAX_DRAW:
            raise ValueError("the draw counter is exhausted (2**31 sample() calls): take a new seed")
        sym, random_symmetry = None, 0
        if isinstance(symmetries, str):
            if symmetries != "random":
                raise ValueError('symmetries must be None, "random" or a uint8 tensor')
            random_symmetry = 1
        elif symmetries is not None:
            sym = check_tensor(symmetries, torch.uint8, (n,), dev, "symmetries")
        if out is None:                 # mask and done: u8 outputs of the kernel (0 / 1), handed out as bool views
            out = tuple(torch.empty((n,) + shp, dtype=torch.uint8 if dt == torch.bool else dt, device=dev).view(dt)
                        for _, dt, shp in _OUT)
        elif len(out) != len(_OUT):
            raise ValueError("out must hold the %d tensors sample() returns" % len(_OUT))
        else:
            for t, (name, dt, shp) in zip(out, _OUT):
                check_tensor(t, dt, (n,) + shp, dev, "out." + name)
        index = torch.empty(n, dtype=torch.int32, device=dev)
        k = torch.empty(n, dtype=torch.uint8, device=dev)
        if self.prioritized:            # sync, then the proportional draw: two entries, nothing read back
            number = torch.empty(n, dtype=torch.int64, device=dev)
            q = torch.empty(n, dtype=torch.int32, device=dev)
            total = torch.zeros(1, dtype=torch.int64, device=dev)
            self.sync_priorities()
            self._call("qttt_replay_sample_prioritized", self.buffer.data_ptr(), self.priority.data_ptr(), self.capacity, n,
                       self.seed, self.draw, _ptr(sym), random_symmetry, *[t.data_ptr() for t in out], index.data_ptr(),
                       k.data_ptr(), number.data_ptr(), q.data_ptr(), total.data_ptr())
            self.last_number, self._last_q, self.last_total = number, q, total
            self.last_priority = q.view(torch.uint32)
        else:
            self._call("qttt_replay_sample", self.buffer.data_ptr(), self.capacity, n, self.seed, self.draw, _ptr(sym),
                       random_symmetry, *[t.data_ptr() for t in out], index.data_ptr(), k.data_ptr())
        self.draw += 1
        self.last_index, self.last_symmetry = index, k
        return tuple(out)

    def gather(self, n, start=None, env=None):
        """A window of n consecutive slots of the ring as a state buffer, one launch and no host read-back
        (include/qttt_replay_reanalyse.h qttt_replay_gather): a ReplayWindow of env (a VecEnv of n boards at the stored
        positions; made here, or the caller's, whose state is overwritten), slot i32[n], number i64[n] (the sample number
        each slot held, what update() compares), v f32[n] and done u8[n] as stored.  start=None draws the window's first
        slot by the counter hash of (seed, the number of gather() calls so far); an integer is taken modulo the samples
        held.  Sample i of a window longer than the ring holds has no slot: slot and number -1, the empty board.  Raises
        before any add() of games, as sample() does."""
        n, dev = int(n), self.device
        if n < 0:
            raise ValueError("n must be >= 0")
        if self.adds == 0:
            raise ValueError("gather() before any add(): the ring is empty")
        if self.gathers >= _MAX_DRAW:
            raise ValueError("the draw counter is exhausted (2**31 gather() calls): take a new seed")
        start = -1 if start is None else int(start)
        if start < -1:
            raise ValueError("start must be None or >= 0")
        if env is None:
            env = VecEnv(n, device=dev)
        elif not isinstance(env, VecEnv) or env.num_envs != n or env.state.device != dev:
            raise ValueError("env must be a VecEnv of %d boards on %s" % (n, dev))
        slot = torch.empty(n, dtype=torch.int32, device=dev)
        number = torch.empty(n, dtype=torch.int64, device=dev)
        v = torch.empty(n, dtype=torch.float32, device=dev)
        done = torch.empty(n, dtype=torch.uint8, device=dev)
        self._call("qttt_replay_gather", self.buffer.data_ptr(), self.capacity, n, self.seed, self.gathers, start,
                   env.state.data_ptr(), slot.data_ptr(), number.data_ptr(), v.data_ptr(), done.data_ptr())
        self.gathers += 1
        return ReplayWindow(self, env, slot, number, v, done)

    def update(self, window, pi=None, v=None):
        """Writes refreshed targets into the slots of a gather()'s window, one launch and no host read-back
        (qttt_replay_update): pi f64[n, 36] and / or v f32[n], at least one.  A sample is written only while its slot
        still holds the sample it was gathered for — an add() since then that went over the slot leaves the newer
        sample alone — and only where the stored done byte is 0: a terminal row keeps its targets.  Nothing but pi and v
        of the written slots changes.  Returns updated bool[n]."""
        if not isinstance(window, ReplayWindow) or window.ring is not self:
            raise ValueError("window must be a ReplayWindow of this ring's gather()")
        n, dev = len(window.slot), self.device
        if pi is None and v is None:
            raise ValueError("update() needs pi, v or both")
        if pi is not None:
            check_tensor(pi, torch.float64, (n, 36), dev, "pi")
        if v is not None:
            check_tensor(v, torch.float32, (n,), dev, "v")
        updated = torch.zeros(n, dtype=torch.uint8, device=dev)
        self._call("qttt_replay_update", self.buffer.data_ptr(), self.capacity, n, window.slot.data_ptr(),
                   window.number.data_ptr(), _ptr(pi), _ptr(v), updated.data_ptr())
        return updated.view(torch.bool)


class ReplayWindow:
    """What ReplayBuffer.gather returns: env (VecEnv of n boards), slot i32[n] (-1: no slot), number i64[n], v f32[n], done
    u8[n]; and mask i64[n], the legal-mask words of the window's slots (0 where there is none), indexed out of the ring
    by torch when first asked for."""

    def __init__(self, ring, env, slot, number, v, done):
        self.ring, self.env, self.slot, self.number, self.v, self.done = ring, env, slot, number, v, done
        self._mask = None

    @property
    def mask(self):
        if self._mask is None:
            held = self.slot >= 0
            words = self.ring.views()["mask"][self.slot.clamp(min=0).to(torch.int64)]
            self._mask = torch.where(held, words, torch.zeros_like(words))
        return self._mask
