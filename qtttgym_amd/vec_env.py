"""VecEnv — N independent Quantum Tic-Tac-Toe boards advanced per call on one MI355X.

Same method names as the reference's gymnasium-style `Env` (env.py:15-85): reset / step /
observ / turn / action_space / observation_space, returning tensors of leading dimension N.
All arithmetic happens in libqttt_hip.so (include/qttt.h); torch is used for device memory
and streams only.
"""
import ctypes
import math
import sys

import torch

from . import _native
from ._host import LibCaller, _ptr, _raw_stream, check_net, check_tensor, out_rows, out_tensor, out_tensors, resolve_device
from .spaces import reference_action_space, reference_observation_space
from .symmetry import check_eval_symmetries
from .solve import SolveResult, check_min_ply, default_boards_per_launch

# The eight tensors of one step's outputs, in the order a default step() carves them out of one allocation
# (csrc/fastviews.cpp has the same order, checked by tests/test_fastviews_cpu.py): key in the observation dict (None: not
# part of it), field of struct qttt_env (include/qttt.h), dtype, per-board shape
_OUTPUTS = (
    (None, "reward", torch.float32, ()),
    (None, "terminated", torch.bool, ()),
    ("q_states_p1", "q_p1", torch.uint8, (5, 2)),
    ("q_states_p1_len", "q_p1_len", torch.uint8, ()),
    ("q_states_p2", "q_p2", torch.uint8, (4, 2)),
    ("q_states_p2_len", "q_p2_len", torch.uint8, ()),
    ("classical", "classical", torch.int8, (9,)),
    ("turn", "turn", torch.uint8, ()),
)
_OBS_KEYS = tuple(k for k, _, _, _ in _OUTPUTS[2:])
_OBS_ROWS = {k: (dt, shp) for k, _, dt, shp in _OUTPUTS[2:]}         # env.py:19-25,68-85
# the order in which qttt_observe / qttt_reset_observe take the observation's addresses (qttt_env fields)
_OBSERVE_ARGS = ("classical", "q_p1", "q_p1_len", "q_p2", "q_p2_len", "turn")
# per output: dtype, one board's shape, the strides of the [n, *shape] tensor (they do not depend on n), bytes per board
_CUTS = tuple((dt, shp, tuple(math.prod(shp[i:]) for i in range(len(shp) + 1)), math.prod(shp) * dt.itemsize)
              for _, _, dt, shp in _OUTPUTS)


def _layout(n):
    """Byte offsets of the eight tensors a default step() returns inside their one allocation (_OUTPUTS, each [n, ...];
    every one starts on a 512-byte boundary) and, last, the allocation's size.  csrc/fastviews.cpp has the same
    arithmetic (checked by tests/test_fastviews_cpu.py)."""
    offs, total = [], 0
    for _, _, _, nbytes in _CUTS:
        offs.append(total)
        total += (n * nbytes + 511) // 512 * 512
    return tuple(offs) + (total,)


def _carve_py(n, dev):
    """One allocation from torch's caching allocator and the eight tensors as views of it: (tensors, address)."""
    o = _layout(n)
    buf = torch.empty(o[8], dtype=torch.uint8, device=dev)
    # whole-buffer views per dtype, cut by element offset: every offset and the size are multiples of 512 bytes
    typed = {dt: buf.view(dt) for dt in (torch.float32, torch.bool, torch.int8)}
    typed[torch.uint8] = buf
    return ([torch.as_strided(typed[dt], (n,) + shp, stride, o[k] // dt.itemsize)
             for k, (dt, shp, stride, _) in enumerate(_CUTS)], buf.data_ptr())


# The same in C++ when qtttgym_amd/_fastviews.so is built (csrc/fastviews.cpp, __graft_entry__.build()): ~2 us of host
# time per call instead of ~12 for the twelve torch calls above — what lets the default step() take a FRESH allocation
# every call and still stay ahead of the kernel at 1 M boards.
try:
    from . import _fastviews
    _carve = _fastviews.carve
except ImportError:
    _fastviews = None
    _carve = _carve_py

# Re-using an output set (VecEnv(output_pool=N), opt-in) needs two counters torch keeps but does not document (the
# storage's and the TensorImpl's use counts); without either, the pool is off and every call allocates
_storage_use_count = getattr(torch._C, "_storage_Use_Count", None)
if not hasattr(torch.Tensor, "_use_count"):
    _storage_use_count = None
_is_capturing = getattr(torch._C, "_cuda_isCurrentStreamCapturing", None) or torch.cuda.is_current_stream_capturing


class _OutputSet:
    """VecEnv(output_pool=N > 0): one step's outputs kept for RE-USE — for loops whose host time per step matters more
    than plain allocator semantics (a pooled step() costs ~2 us of host time less than a fresh allocation; without
    _fastviews.so ~10 us less).

    A set is handed out again only when nothing outside the environment can still see it, which `free()` checks
    exactly: no Python reference to any of its eight tensors beyond the environment's own (sys.getrefcount), no C++
    reference to their TensorImpls (autograd, DLPack: Tensor._use_count) and no other tensor on their storage (views,
    .detach(), .data: the storage's use count) — and only on the stream that wrote it last.  A caller that rebinds
    `obs, reward, terminated, ... = env.step(a)` every step alternates between two sets with no allocation at all; a
    caller that keeps every observation gets a new allocation every step.  What the pool does NOT see: work queued on
    ANOTHER stream that reads a tensor the caller has already dropped — Tensor.record_stream protects an allocation of
    the caching allocator, not a pooled set.  That is why the pool is opt-in and the default step() allocates."""
    __slots__ = ("t", "base", "stream", "_st", "_base")

    def __init__(self, env):
        t, self.base = _carve(env.num_envs, env.device)
        self.t = tuple(t)
        del t
        self.stream = None
        self._st = self.t[0].untyped_storage() if _storage_use_count is not None else None
        self._base = self._probe() if self._st is not None else None

    def _probe(self):
        rc, m = sys.getrefcount, 0
        for t in self.t:
            c = rc(t) + (t._use_count() << 20)
            if c > m:
                m = c
        return m, _storage_use_count(self._st._cdata)

    def free(self):
        return self._st is not None and self._probe() == self._base


class VecEnv(LibCaller):
    """Thread-safety: the C library may be called from any number of host threads at once; ONE VecEnv
    (its state, its output buffers and its qttt_env record) belongs to one thread at a time, exactly
    like the reference's mutable Env (env.py:15)."""

    def __init__(self, num_envs, device="cuda", seed=0, auto_reset=False, board_offset=0, launch_shape=None,
                 output_pool=0):
        n = int(num_envs)
        if n < 0:
            raise ValueError("num_envs must be >= 0")
        dev = resolve_device(device, "VecEnv")
        state = torch.empty(int(_native.lib().qttt_state_bytes(n)), dtype=torch.uint8, device=dev)
        self._init(state, n, seed, auto_reset, board_offset, launch_shape, output_pool)
        self.reset_raw()

    def _init(self, state, n, seed, auto_reset, board_offset, launch_shape=None, output_pool=0):
        """Every field of an environment over `state` (a checked tensor on an indexed cuda device): __init__ and
        from_state (the second constructor: cls.__new__ + _init, nothing else) both end here."""
        self._open(state.device)
        self.num_envs, self.state = n, state
        self.seed = int(seed)
        self.auto_reset = bool(auto_reset)
        self.board_offset = int(board_offset)     # global index of board 0 (multi-GPU shards)
        self._step_host, self._ctr = 0, None      # the step index: a host int, or (graph mode) a device u32
        # (boards per lane, workgroup size) of this environment's step launches, carried by every call's
        # flags (QTTT_FLAG_SHAPE); None = the library picks it from the batch size.  Never changes results.
        self._shape_flags = _native.flag_shape(*launch_shape) if launch_shape else 0
        self.action_space = reference_action_space()
        self.observation_space = reference_observation_space()
        dev = self.device
        self._reward = torch.empty(n, dtype=torch.float32, device=dev)
        self._terminated = torch.empty(n, dtype=torch.bool, device=dev)
        self._truncated = torch.zeros(n, dtype=torch.bool, device=dev)  # env.py:52
        self._obs = None
        # default step() / reset(): a fresh allocation per call (0, the default), or at most this many output sets kept
        # for re-use (_OutputSet)
        self._pool, self._pool_i, self._pool_max = [], 0, max(0, int(output_pool))
        # include/qttt.h struct qttt_env: the per-step calls then pass 6 arguments instead of 11 - 17 (the per-step calls
        # are host-bound below ~500 K boards: every data_ptr() and context switch saved is throughput)
        self._rec = _native.EnvRecord(state=state.data_ptr(), n=n, reward=self._reward.data_ptr(),
                                      terminated=self._terminated.data_ptr())
        self._rec_ref = ctypes.byref(self._rec)
        # the record a default step() / reset() points at ITS output tensors (read by the library during the call only):
        # (field, byte offset in the one allocation) of each of them
        self._rec_out = _native.EnvRecord(n=n)
        self._rec_out_ref = ctypes.byref(self._rec_out)
        self._out_fields = tuple(zip((f for _, f, _, _ in _OUTPUTS), _layout(n)))

    # ------------------------------------------------------------------ the step index
    @property
    def step_idx(self):
        """Steps taken since reset: keys the collapse-bit / policy hash.  A host int — or, once
        use_device_step_counter() / capture() was called, a device-side u32 (reading it then synchronises)."""
        return self._step_host + (0 if self._ctr is None else int(self._ctr))

    @step_idx.setter
    def step_idx(self, v):
        if self._ctr is None:
            self._step_host = int(v)
        else:
            self._step_host = 0
            self._ctr.fill_(int(v))

    def use_device_step_counter(self):
        """Moves the step index into a device-side u32 that the step kernels read when they RUN
        (qttt_env.step_counter): launches captured in a hipGraph then use a fresh index on every replay.
        Eager calls keep working; each of them advances the counter with one extra one-lane launch, and the
        step launches that read the counter run in one shape (one board per lane, 256-thread workgroups): this is the
        mode for small, launch-bound batches — at 1 M boards the ordinary path is ~20 % faster."""
        if self._ctr is None:
            self._ctr = torch.tensor(self._step_host, dtype=torch.int32, device=self.device)
            self._step_host = 0
            # (the only writer of step_counter: both records carry it, keep them in step)
            self._rec.step_counter = self._rec_out.step_counter = self._ctr.data_ptr()
        return self._ctr

    def _advance(self, k):
        if self._ctr is None:
            self._step_host += k
        else:
            self._call("qttt_counter_add", self._ctr.data_ptr(), k)

    # ------------------------------------------------------------------ helpers
    def _record(self, fresh=False):
        """The qttt_env record — the environment's own, or (fresh) the one _fresh_outputs pointed at new tensors —
        with the fields a caller may have changed since the last step."""
        if fresh:
            r, ref = self._rec_out, self._rec_out_ref
        else:
            r, ref = self._rec, self._rec_ref
        r.state = self.state.data_ptr()
        r.board_offset, r.seed, r.flags = self.board_offset, self.seed, self._flags()
        return ref

    def _flags(self):
        return (_native.FLAG_AUTO_RESET if self.auto_reset else 0) | self._shape_flags

    def _as_actions(self, actions):
        if not torch.is_tensor(actions):
            actions = torch.as_tensor(actions)
        if actions.shape != (self.num_envs, 2):
            raise ValueError("actions must have shape (%d, 2), got %s" % (self.num_envs, tuple(actions.shape)))
        if actions.dtype != torch.uint8:
            # anything outside 0..8 is a noop in the reference (IndexError swallowed at env.py:41);
            # map it to 255 before narrowing so that e.g. 256 does not wrap to square 0
            a = actions.to(torch.int64)
            actions = torch.where((a < 0) | (a > 255), torch.full_like(a, 255), a).to(torch.uint8)
        return actions.to(self.device).contiguous()

    def _like(self, env=None, what=None):
        """An environment over a state buffer of this one's size, for a kernel to fill: a new one, or the caller's
        `env` checked."""
        if env is None:
            return VecEnv.from_state(torch.empty_like(self.state), self.num_envs, seed=self.seed,
                                     board_offset=self.board_offset)
        if env.num_envs != self.num_envs or env.state.device != self.device:
            raise ValueError("%s must be a VecEnv of N boards on this device" % what)
        return env

    # what gym-style callers touch besides reset / step (gymnasium.vector's names for the per-board spaces; the reference's
    # Env declares the per-board spaces, env.py:19-25, and those are what action_space / observation_space hold here)
    @property
    def single_action_space(self):
        return self.action_space

    @property
    def single_observation_space(self):
        return self.observation_space

    @property
    def unwrapped(self):
        return self

    def close(self):
        """Drops the pooled output sets (the state and the tensors a caller holds stay valid)."""
        self._pool, self._pool_i = [], 0

    def synchronize(self):
        """torch.cuda.synchronize(device) for a process that also uses the single-board façades (Board, Env): their
        mailbox wave (include/qttt.h, qttt_board_op_host) is asked to leave first, so the device-wide wait has nothing
        of this library to wait for (otherwise: up to the wave's idle window, 20 us by default)."""
        self._lib.qttt_board_mailbox_retire(1)
        torch.cuda.synchronize(self.device)

    # ------------------------------------------------------------------ gym surface
    def reset_raw(self, seed=None):
        """Fresh boards without building the observation (one launch of zero stores on the stream)."""
        if seed is not None:
            self.seed = int(seed)
        self.step_idx = 0                         # (the device counter's fill is ordered on the stream like the memset)
        self._call("qttt_reset", self.state.data_ptr(), self.num_envs)

    def _fresh_outputs(self):
        """The eight tensors of one default step() / reset() (_OUTPUTS), which nobody else holds, and self._rec_out
        pointing at them.
        Default: ONE new allocation from torch's caching allocator per call, carved into the eight views (csrc/fastviews.cpp
        when built): plain allocator semantics, nothing is ever re-used behind the caller's back.  With output_pool=N: a
        pooled set that is free (_OutputSet), else a new one.  Inside a hipGraph capture every call allocates (from the
        graph's private pool, which lives as long as the graph): a captured launch keeps writing where it was captured."""
        if self._pool_max and not _is_capturing():
            stream = _raw_stream(self._dev_index)
            pool, i = self._pool, self._pool_i
            k = len(pool)
            s = None
            for _ in range(k):
                i = i + 1 if i + 1 < k else 0
                c = pool[i]
                # (re-use only on the stream that wrote it last: the same rule as torch's caching allocator)
                if c.stream == stream and c.free():
                    s = c
                    break
            if s is None:
                s = _OutputSet(self)
                s.stream = stream
                if k < self._pool_max:
                    pool.append(s)
                    i = k
                else:                               # every set is still held by the caller: forget the oldest one
                    i = self._pool_i + 1 if self._pool_i + 1 < k else 0
                    pool[i] = s
            self._pool_i = i
            t, base = s.t, s.base
        else:
            t, base = _carve(self.num_envs, self.device)
        r = self._rec_out
        for field, off in self._out_fields:
            setattr(r, field, base + off)
        return t

    def _observe(self, name, rec):
        """qttt_observe / qttt_reset_observe into the observation tensors the record `rec` points at."""
        self._call(name, self.state.data_ptr(), *[getattr(rec, f) for f in _OBSERVE_ARGS], self.num_envs)

    def reset(self, *, seed=None, options=None, copy_obs=True):
        """env.py:55-57: fresh boards and their observation, ONE kernel (qttt_reset_observe); `seed`/`options`
        accepted and ignored like the reference, except that an int `seed` re-keys the collapse-bit hash (the
        reference has no per-env RNG).  The observation is made of fresh tensors (written by the kernel itself, never
        copied) unless copy_obs=False (then: the environment's own buffers, which the next copy_obs=False step() /
        observ() overwrites)."""
        if seed is not None:
            self.seed = int(seed)
        self.step_idx = 0
        if copy_obs:
            obs, rec = dict(zip(_OBS_KEYS, self._fresh_outputs()[2:])), self._rec_out
        else:
            obs, rec = self._obs_buffers(), self._rec
        self._observe("qttt_reset_observe", rec)
        return obs, {}

    def step_raw(self, actions, bits=None):
        """The hot path alone: one fused kernel launch, no observation unpack.
        actions u8[N,2] on the device; bits u8[N] (explicit collapse bits, parity mode) or None
        (bit = counter hash of (seed, board_offset+i, step_idx)).
        Returns (reward f32[N], terminated bool[N]) — buffers reused across calls."""
        n, dev = self.num_envs, self.device
        check_tensor(actions, torch.uint8, (n, 2), dev, "actions", True)       # (any view of 2 N / N elements)
        if bits is not None:
            check_tensor(bits, torch.uint8, (n,), dev, "bits", True)
        self._call("qttt_env_step", self._record(), actions.data_ptr(), _ptr(bits), self._step_host, _native.ENV_STEP)
        self._advance(1)
        return self._reward, self._terminated

    def step_random(self, actions_out=None):
        """One step under the synthetic uniform-legal policy, policy and step fused in one kernel
        (== sample_actions() followed by step_raw()).  Returns (reward, terminated); the actions
        played are written to `actions_out` (u8[N,2]) if given."""
        if actions_out is not None:
            check_tensor(actions_out, torch.uint8, (self.num_envs, 2), self.device, "actions_out", True)
        self._call("qttt_env_step", self._record(), _ptr(actions_out), None, self._step_host, _native.ENV_STEP_RANDOM)
        self._advance(1)
        return self._reward, self._terminated

    def step_many(self, actions, bits=None, reward=None, terminated=None, fused=False):
        """T consecutive steps from pre-recorded device tensors actions u8[T,N,2] (bits u8[T,N]),
        enqueued from C with no per-step host work.  With `reward`/`terminated` of shape [T,N]
        every step's outputs are kept; otherwise only the last step's (returned).
        fused=True runs the T steps with the boards in registers, one launch per 256 steps (per 64 when every step's
        outputs are kept; same results); without
        output buffers the library does so by itself for 448 K < N <= 1536 K boards, T >= 16 and no launch shape named
        (one launch per step otherwise)."""
        n, dev = self.num_envs, self.device
        T = int(actions.shape[0])
        check_tensor(actions, torch.uint8, (T, n, 2), dev, "actions")
        if bits is not None:
            check_tensor(bits, torch.uint8, (T, n), dev, "bits")
        r, tm, stride = self._kept_outputs(T, reward, terminated)
        self._call("qttt_step_many", self.state.data_ptr(), actions.data_ptr(), _ptr(bits), self.seed, self.step_idx,
                   self.board_offset, self._flags() | (_native.FLAG_FUSED if fused else 0), r.data_ptr(), tm.data_ptr(),
                   stride, n, T)
        self._advance(T)
        return r, tm

    def _kept_outputs(self, T, reward, terminated):
        """(reward, terminated, their step stride) of a T-step call: the caller's [T,N] pair, which keeps every step's
        outputs, or the environment's own buffers, which keep the last step's."""
        if reward is None and terminated is None:
            return self._reward, self._terminated, 0
        if reward is None or terminated is None:
            raise ValueError("reward f32[T,N] and terminated bool[T,N] must be given together")
        n, dev = self.num_envs, self.device
        return (check_tensor(reward, torch.float32, (T, n), dev, "reward"),
                check_tensor(terminated, torch.bool, (T, n), dev, "terminated"), n)

    def step(self, actions, bits=None, verbose=False, copy_obs=True):
        """env.py:34-53 for N boards: (obs, reward, terminated, truncated, info) from ONE kernel launch and nothing
        else (the step kernel writes the observation from the registers it holds, straight into the tensors returned).
        copy_obs=True (default): the returned observation, reward and terminated are tensors nobody else holds — as
        the reference's Env.step builds new lists every call (env.py:46,68-85), a gym caller may keep (obs, next_obs)
        pairs, or every observation of an episode: one fresh allocation per call, carved into the eight tensors
        (_fresh_outputs; VecEnv(output_pool=N) re-uses sets the caller has dropped instead).  The eight tensors of one
        call share that one allocation (34 bytes per board + padding): keeping — or torch.save-ing — any one of them
        keeps all of it, so a replay buffer that stores one field for long should store `.clone()`s.  copy_obs=False returns the environment's own buffers, overwritten by the next such step() /
        observ() — = step_observe_raw."""
        dev = self.device
        if not (torch.is_tensor(actions) and actions.dtype == torch.uint8 and actions.device == dev
                and actions.shape == (self.num_envs, 2) and actions.is_contiguous()):
            actions = self._as_actions(actions)
        if bits is not None and not (torch.is_tensor(bits) and bits.dtype == torch.uint8 and bits.device == dev
                                     and bits.is_contiguous()):
            bits = torch.as_tensor(bits).to(torch.uint8).to(dev).contiguous()
        if not copy_obs:
            obs, reward, terminated = self.step_observe_raw(actions, bits)
            return obs, reward, terminated, self._truncated, {}
        if bits is not None:
            check_tensor(bits, torch.uint8, (self.num_envs,), dev, "bits", True)
        t = self._fresh_outputs()
        self._call("qttt_env_step", self._record(True), actions.data_ptr(), _ptr(bits), self._step_host,
                   _native.ENV_STEP_OBSERVE)
        self._advance(1)
        return dict(zip(_OBS_KEYS, t[2:])), t[0], t[1], self._truncated, {}

    def _obs_buffers(self):
        """The observation tensors (env.py:19-25,68-85), allocated once per environment; self._rec points at them."""
        if self._obs is None:
            self._obs = out_rows(_OBS_ROWS, self.num_envs, self.device)
            for key, field, _, _ in _OUTPUTS[2:]:
                setattr(self._rec, field, self._obs[key].data_ptr())
        return self._obs

    def step_observe_raw(self, actions, bits=None):
        """Env.step for N boards including the observation (env.py:46), one fused kernel:
        qttt_step_observe.  Same argument rules as step_raw.  Returns (obs dict, reward, terminated),
        all buffers owned by the environment and reused across calls."""
        n, dev = self.num_envs, self.device
        check_tensor(actions, torch.uint8, (n, 2), dev, "actions", True)       # (any view of 2 N / N elements)
        if bits is not None:
            check_tensor(bits, torch.uint8, (n,), dev, "bits", True)
        o = self._obs_buffers()
        self._call("qttt_env_step", self._record(), actions.data_ptr(), _ptr(bits), self._step_host,
                   _native.ENV_STEP_OBSERVE)
        self._advance(1)
        return o, self._reward, self._terminated

    def observ(self):
        """env.py:62-63,68-85 as tensors: q_states_p{1,2} u8[N,5|4,2] (255 pad) with *_len,
        classical i8[N,9], turn u8[N].  The tensors are the environment's own buffers (allocated
        once), overwritten by the next observ()/step()."""
        obs = self._obs_buffers()
        self._observe("qttt_observe", self._rec)
        return obs

    def turn(self, out=None):
        """env.py:65-66: len(moves) per board (counts the autofill move), u8[N]: qttt_export asked for
        n_moves alone (8 bytes read and 1 written per board).  `out` = a tensor to overwrite."""
        out = out_tensor(torch.uint8, (), self.num_envs, self.device, out)
        self._call("qttt_export", self.state.data_ptr(), None, out.data_ptr(), None, None, None, self.num_envs)
        return out

    def render(self, index=0):
        from .board import Board, displayBoard
        displayBoard(Board.from_export(self.export_boards(), index))

    # ------------------------------------------------------------------ Board-level access
    def check_win(self, out=None):
        """board.py:71-115 per board: (p1_round i8[N], p2_round i8[N]).  `out` = a pair returned by an
        earlier call, to be overwritten instead of allocating (half the cost of the call at 1 M boards)."""
        p1, p2 = out_tensors(((torch.int8, ()),) * 2, self.num_envs, self.device, out, numel=True)
        self._call("qttt_check_win", self.state.data_ptr(), p1.data_ptr(), p2.data_ptr(), self.num_envs)
        return p1, p2

    # Named output rows: name -> (dtype, per-board shape), for _host.out_rows
    _EXPORT_ROWS = {"moves": (torch.uint8, (9, 2)), "n_moves": (torch.uint8, ()), "board": (torch.int8, (9,)),
                    "qmask": (torch.int16, (4,)), "n_q": (torch.uint8, ())}
    _EXPORT_SPEC = tuple((k,) + v for k, v in _EXPORT_ROWS.items())    # (name, dtype, shape): the form older callers read
    _NODE_ROWS = {"winner": (torch.int8, ()), "terminal": (torch.bool, ()), "legal": (torch.int64, ()),
                  "state_key": (torch.int64, ()), "key": (torch.int64, ())}
    _EXPAND_ROWS = {"n_children": (torch.uint8, ()), "winner": (torch.int8, (2,)), "terminal": (torch.bool, (2,)),
                    "legal": (torch.int64, (2,)), "state_key": (torch.int64, (2,)), "key": (torch.int64, (2,))}
    _EVAL_ROWS = {"value": (torch.float32, ()), "logits": (torch.float32, (36,)), "probs": (torch.float32, (36,))}
    _LEAF_ROWS = {"value": _EVAL_ROWS["value"], "probs": _EVAL_ROWS["probs"]}

    @staticmethod
    def _expand_rollout_rows(n_sims):
        return {"value_sum": (torch.int32, (2,)), "result": (torch.int8, (2, n_sims))}

    @staticmethod
    def _policy_rows(n_sims):
        return {"result": (torch.int8, (n_sims,)), "plies": (torch.uint8, (n_sims,)), "trace": (torch.uint8, (n_sims, 9)),
                **VecEnv._LEAF_ROWS}

    def export_boards(self, out=None):
        """Board.moves / .board / .qstructs (board.py:4-6) as tensors.  `out` = the dict of an earlier
        call, to be overwritten instead of allocating."""
        out = out_rows(self._EXPORT_ROWS, self.num_envs, self.device, out, required=self._EXPORT_ROWS)
        self._call("qttt_export", self.state.data_ptr(), out["moves"].data_ptr(), out["n_moves"].data_ptr(),
                   out["board"].data_ptr(), out["qmask"].data_ptr(), out["n_q"].data_ptr(), self.num_envs)
        return out

    def import_boards(self, moves, n_moves, board, qmask, n_q):
        n = self.num_envs
        given = {"moves": moves, "n_moves": n_moves, "board": board, "qmask": qmask, "n_q": n_q}
        ptrs = []
        for k, (dtype, shape) in self._EXPORT_ROWS.items():
            t = torch.as_tensor(given[k]).to(dtype).to(self.device).contiguous()
            if tuple(t.shape) != (n,) + shape:
                raise ValueError("expected shape %s, got %s" % ((n,) + shape, tuple(t.shape)))
            given[k] = t                                   # (alive until the launch is enqueued)
            ptrs.append(t.data_ptr())
        self._call("qttt_import", self.state.data_ptr(), *ptrs, n)

    def sample_actions(self, out=None):
        """Uniform-legal synthetic policy for the *next* step.  `out` u8[N,2] to overwrite."""
        out = out_tensor(torch.uint8, (2,), self.num_envs, self.device, out, numel=True)
        # through the qttt_env record: with a device-side step counter the call stays capturable in a hipGraph
        self._call("qttt_env_step", self._record(), out.data_ptr(), None, self._step_host, _native.ENV_SAMPLE)
        return out

    def step_random_many(self, n_steps, actions_out=None, reward=None, terminated=None, returns=None):
        """n_steps steps under the in-kernel uniform-legal policy with the boards in registers, ONE launch per
        64 plies (qttt_step_random_many) == n_steps calls of step_random().  With reward f32[T,N] +
        terminated bool[T,N] (and optionally actions_out u8[T,N,2]) every step's outputs are kept; without
        them only the last step's are written (to the environment's own reward / terminated buffers, which
        are returned; actions_out u8[N,2] optional).  returns f32[N] (optional) is ACCUMULATED: += the sum of each
        board's rewards over these plies (env.py:49) — the per-board episode returns, with no per-ply output kept."""
        n, T, dev = self.num_envs, int(n_steps), self.device
        r, tm, stride = self._kept_outputs(T, reward, terminated)
        if actions_out is not None:        # one out_stride for all outputs: [T,N,2] with reward/terminated [T,N], else [N,2]
            check_tensor(actions_out, torch.uint8, (T, n, 2) if reward is not None else (n, 2), dev, "actions_out")
        if returns is not None:
            check_tensor(returns, torch.float32, (n,), dev, "returns")
        self._call("qttt_step_random_many", self.state.data_ptr(), self.seed, self.step_idx, self.board_offset,
                   self._flags(), _ptr(actions_out), r.data_ptr(), tm.data_ptr(), stride, _ptr(returns), n, T)
        self._advance(T)
        return r, tm

    # ------------------------------------------------------------------ MCTS-side rows
    @classmethod
    def from_state(cls, state, num_envs, seed=0, auto_reset=False, board_offset=0):
        """Wraps an existing packed state tensor (e.g. a child buffer written by expand()): a contiguous uint8 tensor
        of qttt_state_bytes(num_envs) bytes on a cuda device.

        The tensor must hold states this library wrote (reset, step, expand, import_boards ...).  Two things are relied
        on and NOT re-checked: the cached qstructs and rooted forest are consistent with the moves, and the done bit
        (bit 63 of plane P) is set iff the board has a completed line or at least eight classical squares — the step
        only ever SETS that bit (a line stays a line), and with auto_reset the in-kernel policy trusts "not done" to
        mean "at least two empty squares".  A hand-made tensor with a wrong done bit is stepped without faults (the
        kernels keep everything in registers, every loop is bounded) but gives states the reference never reaches;
        to bring boards from attributes use import_boards(), which computes the bit."""
        n = int(num_envs)
        if not torch.is_tensor(state):
            raise ValueError("state must be a tensor")
        check_tensor(state, torch.uint8, (int(_native.lib().qttt_state_bytes(n)),), state.device, "state", numel=True)
        if state.device.type != "cuda":      # (check_tensor compares with ONE expected device; any cuda device will do here)
            raise ValueError("state must be a tensor on a cuda device")
        env = cls.__new__(cls)
        env._init(state, n, seed, auto_reset, board_offset)
        return env

    def take(self, index, seed=None, auto_reset=None, board_offset=None):
        """A new VecEnv holding boards self[index] (any int64 index tensor; repeats allowed): the batched form of
        `copy.deepcopy(node)` + attribute assignment in MCTS._step (mcts.py:236-241) — e.g.
        `env.take(torch.arange(N).repeat_interleave(36))` lines every leaf up 36 times for one expand() over all
        its actions.  Pure indexing of the two packed planes; nothing is unpacked."""
        idx = torch.as_tensor(index, device=self.device).to(torch.int64).reshape(-1)
        m = int(idx.numel())
        planes = self.state.view(torch.int64).view(2, -1)
        st = torch.zeros(int(self._lib.qttt_state_bytes(m)), dtype=torch.uint8, device=self.device)
        if m:
            st.view(torch.int64).view(2, -1)[:, :m] = planes[:, idx]
        return VecEnv.from_state(st, m, seed=self.seed if seed is None else seed,
                                 auto_reset=self.auto_reset if auto_reset is None else auto_reset,
                                 board_offset=self.board_offset if board_offset is None else board_offset)

    def transformed(self, k, out=None):
        """The boards' images under a symmetry (include/qttt_symmetry.h qttt_transform; qtttgym_amd.symmetry numbers
        the eight): a VecEnv over the states that stepping reaches when the mirrored games are played, bit for bit.
        k = an int 0..7 for every board, or a uint8 tensor [N] with one per board (an entry past 7 leaves that board as
        it is).  out = a VecEnv of N boards on this device to overwrite — `self` for in place; default: a new one with
        this one's seed and board_offset."""
        n = self.num_envs
        if torch.is_tensor(k):
            sym, k = check_tensor(k, torch.uint8, (n,), self.device, "k"), 0
        else:
            sym, k = None, int(k)
            if not 0 <= k < _native.SYMMETRIES:
                raise ValueError("a symmetry is 0..%d, got %d" % (_native.SYMMETRIES - 1, k))
        out = self._like(out, "out")
        self._call("qttt_transform", self.state.data_ptr(), out.state.data_ptr(), _ptr(sym), k, n)
        return out

    def node_info(self, out=None, python_key=True):
        """GameState bookkeeping per board (mcts.py:20-27,52-65,93-94): winner i8 (1/0/-1 = True/
        False/None), terminal bool, legal int64 (bit a = action a legal), state_key int64 (the native 64-bit
        position key: equal <=> equal (board, moves); qttt_state_key of the packed words) and — with
        python_key — key int64 = Python's hash(tuple(board)+tuple(moves)), for host-side dicts built by
        reference code (three quarters of the kernel's work: a device-side search passes python_key=False).
        `out` = the dict of an earlier call, to be overwritten: only the entries it holds are computed."""
        keys = [k for k in self._NODE_ROWS if k != "key" or python_key]
        out = out_rows(self._NODE_ROWS, self.num_envs, self.device, out, keys, numel=True)
        self._call("qttt_node_info", self.state.data_ptr(), _ptr(out.get("winner")), _ptr(out.get("terminal")),
                   _ptr(out.get("legal")), _ptr(out.get("key")), _ptr(out.get("state_key")), self.num_envs)
        return out

    def state_keys(self, out=None):
        """The native position keys alone (int64[N]): 16 bytes read and 8 written per board."""
        out = out_tensor(torch.int64, (), self.num_envs, self.device, out)
        self._call("qttt_node_info", self.state.data_ptr(), None, None, None, None, out.data_ptr(), self.num_envs)
        return out

    def _expand_out(self, out, python_key, extra=None):
        """The output dict of expand / expand_rollout: allocated, or the one of an earlier call checked (its per-child
        rows are optional, only what the dict holds is computed — but the `extra` rows, and "key" with python_key, are
        required: e.g. the dict of expand() handed to expand_rollout(), or python_key=True with a dict made without it)."""
        extra = extra or {}
        spec = {**self._EXPAND_ROWS, **extra}
        required = tuple(extra) + (("key",) if python_key else ())
        if out is None:
            keys = [k for k in spec if k != "key"] + (["key"] if python_key else [])
            return {"child0": self._like(), "child1": self._like(), **out_rows(spec, self.num_envs, self.device, keys=keys)}
        for c in ("child0", "child1"):
            if c not in out:
                raise ValueError("out[%r] is required" % c)
            self._like(out[c], "out[%r]" % c)
        return out_rows(spec, self.num_envs, self.device, out, required=required)

    def _as_action36(self, action36):
        a = action36
        if not (torch.is_tensor(a) and a.dtype == torch.uint8 and a.device == self.device and a.is_contiguous()):
            a = torch.as_tensor(a).to(torch.uint8).to(self.device).contiguous()
        if a.shape != (self.num_envs,):
            raise ValueError("action36 must have shape (%d,)" % self.num_envs)
        return a

    def expand(self, action36, out=None, python_key=None):
        """MCTS._step (mcts.py:233-267) for every board: action36 u8[N] (ind2move index).
        Returns dict(child0, child1 = VecEnv over the child states, n_children u8[N],
        winner i8[N,2], terminal bool[N,2], legal int64[N,2], state_key int64[N,2] and — with python_key —
        key int64[N,2] = Python's hash of each child, see node_info).
        `out` = the dict of an earlier call: its child states and tensors are overwritten (a search loop
        then allocates nothing per expansion); its "key" entry decides python_key (python_key=True with a dict
        that has no "key" entry raises ValueError).  python_key=None: True for a fresh dict, the dict's choice otherwise."""
        a = self._as_action36(action36)
        out = self._expand_out(out, (out is None) if python_key is None else bool(python_key))
        self._call("qttt_expand", self.state.data_ptr(), a.data_ptr(), out["child0"].state.data_ptr(),
                   out["child1"].state.data_ptr(), _ptr(out.get("n_children")), _ptr(out.get("winner")),
                   _ptr(out.get("terminal")), _ptr(out.get("legal")), _ptr(out.get("key")),
                   _ptr(out.get("state_key")), self.num_envs)
        return out

    def expand_rollout(self, action36, n_sims=1, step_idx0=None, out=None, python_key=None, with_result=False):
        """One MCTS._rollout below the selected node in ONE launch (mcts.py:166-176,210-221,233-267): expand() plus
        n_sims random playouts from EACH child.  Returns expand()'s dict with two more entries:
        value_sum int32[N,2] = the sum over a child's playouts of `r if leaf.turn else -r` (mcts.py:174; divide by
        n_sims for the value _backpropogate receives) and — with_result — result int8[N,2,n_sims], every playout's
        MCTS._reward.  Bit-identical to expand() followed by child0.rollout_many(n_sims, step_idx0) and
        child1.rollout_many(n_sims, step_idx0 + 16 * n_sims).  `out` = the dict of an earlier call with the same
        n_sims, overwritten."""
        S = int(n_sims)
        if not 1 <= S <= _native.EXPAND_ROLLOUT_MAX_SIMS:
            raise ValueError("n_sims must be in 1..%d" % _native.EXPAND_ROLLOUT_MAX_SIMS)
        if step_idx0 is None:
            step_idx0 = self.step_idx
        a = self._as_action36(action36)
        extra = self._expand_rollout_rows(S)
        if not (with_result or (out is not None and "result" in out)):
            del extra["result"]
        out = self._expand_out(out, bool(python_key), extra)       # None = False for a fresh dict, the dict's choice otherwise
        self._call("qttt_expand_rollout", self.state.data_ptr(), a.data_ptr(), out["child0"].state.data_ptr(),
                   out["child1"].state.data_ptr(), _ptr(out.get("n_children")), _ptr(out.get("winner")),
                   _ptr(out.get("terminal")), _ptr(out.get("legal")), _ptr(out.get("key")), _ptr(out.get("state_key")),
                   self.seed, int(step_idx0), self.board_offset, S, out["value_sum"].data_ptr(), _ptr(out.get("result")),
                   self.num_envs)
        return out

    def rollout(self, step_idx0=None, return_final=False, out=None):
        """MCTS._simulate (mcts.py:185-198) under uniform priors: one fused random playout per
        board, boards unchanged.  Returns (result i8[N] in {+1,-1,0}, plies u8[N][, final VecEnv]).
        `out` = the tuple of an earlier call with the same return_final, to be overwritten."""
        if step_idx0 is None:
            step_idx0 = self.step_idx
        result, plies = out_tensors(((torch.int8, ()), (torch.uint8, ())), self.num_envs, self.device,
                                None if out is None else out[:2])
        final = self._like(None if out is None else out[2], "out[2]") if return_final else None
        self._call("qttt_rollout", self.state.data_ptr(), self.seed, int(step_idx0), self.board_offset,
                   result.data_ptr(), plies.data_ptr(), None if final is None else final.state.data_ptr(), self.num_envs)
        return (result, plies, final) if return_final else (result, plies)

    def rollout_many(self, n_sims, step_idx0=None, with_plies=False, out=None):
        """MCTS._rollout's simulation loop (mcts.py:170-176: num_simulations playouts from each leaf) in ONE launch,
        one lane per (board, simulation): result i8[N, n_sims] (+1 / -1 / 0 per MCTS._reward), optionally plies
        u8[N, n_sims].  Column s equals rollout(step_idx0 + s * 16).  `out` = what an earlier call returned."""
        S = int(n_sims)
        if S < 1:
            raise ValueError("n_sims must be >= 1")
        if step_idx0 is None:
            step_idx0 = self.step_idx
        spec = ((torch.int8, (S,)), (torch.uint8, (S,)))
        if with_plies:
            result, plies = out_tensors(spec, self.num_envs, self.device, out)
        else:
            result, plies = out_tensor(*spec[0], self.num_envs, self.device, out), None
        self._call("qttt_rollout_many", self.state.data_ptr(), self.seed, int(step_idx0), self.board_offset, S,
                   result.data_ptr(), _ptr(plies), self.num_envs)
        return (result, plies) if with_plies else result

    _SOLVE_ROWS = ((torch.float32, ()), (torch.float32, (36,)), (torch.uint8, ()), (torch.int64, ()), (torch.bool, ()))

    def solve(self, min_ply=5, out=None, boards_per_launch=None):
        """The exact expectimax solution of every board with at least min_ply (4..9) moves played, and of every finished
        board (include/qttt_solve.h qttt_solve: the full tree below the position, one workgroup per board, nothing
        sampled or pruned): a SolveResult of value f32[N], q f32[N, 36], best u8[N], nodes i64[N], solved bool[N].  An
        earlier, unfinished board is skipped (solved False, NaN) and costs nothing.  The boards are not changed.
        out = the SolveResult of an earlier call on N boards, to be overwritten.  boards_per_launch: the batch goes out
        in launches of at most this many boards, with the same results — at min_ply 4 a board is up to a few 10^7
        positions, and the default (qtttgym_amd.solve.BOARDS_PER_LAUNCH) keeps one launch under a second on a device
        that others share; None at min_ply >= 6 = one launch."""
        n, dev = self.num_envs, self.device
        min_ply = check_min_ply(min_ply)
        per = default_boards_per_launch(min_ply) if boards_per_launch is None else int(boards_per_launch)
        if per is not None and per < 1:
            raise ValueError("boards_per_launch must be >= 1")
        if out is not None and not isinstance(out, SolveResult):
            raise ValueError("out must be a SolveResult")
        given = None if out is None else (out.value, out.q, out.best, out.nodes, out.solved)
        value, q, best, nodes, solved = out_tensors(self._SOLVE_ROWS, n, dev, given)
        status = solved.view(torch.uint8)
        if per is None or n <= per:
            self._call("qttt_solve", self.state.data_ptr(), n, min_ply, value.data_ptr(), q.data_ptr(), best.data_ptr(),
                       nodes.data_ptr(), status.data_ptr())
        else:
            # a launch reads one contiguous run of both planes; their stride is that of the whole batch, so each run is
            # copied into a batch of its own
            for lo in range(0, n, per):
                hi = min(n, lo + per)
                part = self.take(torch.arange(lo, hi, device=dev))
                self._call("qttt_solve", part.state.data_ptr(), hi - lo, min_ply, value[lo:hi].data_ptr(),
                           q[lo:hi].data_ptr(), best[lo:hi].data_ptr(), nodes[lo:hi].data_ptr(), status[lo:hi].data_ptr())
        if n:
            torch.logical_not(solved, out=solved)           # the library's status: 0 = solved, 1 = skipped
        return out if out is not None else SolveResult(value, q, best, nodes, solved)

    def encode(self, with_mask=True, out=None):
        """GameState.to_vector (mcts.py:67-85) as f32[N,18,10] and action_mask (mcts.py:87-91) as
        bool[N,36], without leaving the GPU.  `out` = what an earlier call returned, to be overwritten."""
        spec = ((torch.float32, (18, 10)), (torch.bool, (36,)))
        if with_mask:
            vec, mask = out_tensors(spec, self.num_envs, self.device, out)
        else:
            vec, mask = out_tensor(*spec[0], self.num_envs, self.device, out), None
        self._call("qttt_encode", self.state.data_ptr(), vec.data_ptr(), _ptr(mask), self.num_envs)
        return (vec, mask) if with_mask else vec

    def evaluate(self, net, rows=("value", "logits"), out=None, symmetries=None):
        """nn.Model.forward(GameState.to_vector()) (nn.py:7-72, alphazero.py:294-300) for every board in ONE kernel
        (include/qttt_nn.h qttt_evaluate): a dict of the requested rows among value f32[N], logits f32[N,36] (-inf at
        illegal actions) and probs f32[N,36] (= Categorical(logits).probs; NaN rows where every action is masked).
        `net` = a PolicyValueNet on this device.  `out` = the dict of an earlier call: its tensors are overwritten and
        its keys decide which rows are computed (`rows` is then ignored).  Runs on the current stream.
        symmetries (include/qttt_nn_symmetric.h qttt_evaluate_symmetric, still one kernel): a sequence of 1, 2, 4 or 8
        symmetries 0..7 ("all": the eight in order) — every row is the mean over the board's images under them, each
        image's outputs mapped back to the board's own actions; or a uint8 tensor [N] on this device — board i is
        evaluated under symmetries[i] alone and mapped back (an entry past 7 is the identity)."""
        n, dev = self.num_envs, self.state.device
        check_net(net, dev)
        if torch.is_tensor(symmetries):
            sym, lst = check_tensor(symmetries, torch.uint8, (n,), dev, "symmetries"), (0,)
        elif symmetries is not None:
            sym, lst = None, check_eval_symmetries(symmetries)
        if out is None:
            rows = (rows,) if isinstance(rows, str) else tuple(rows)
            if not rows or any(r not in self._EVAL_ROWS for r in rows):
                raise ValueError("rows must be a non-empty subset of %s" % (tuple(self._EVAL_ROWS),))
        elif not any(out.get(r) is not None for r in self._EVAL_ROWS):
            raise ValueError("out must be a dict returned by evaluate()")
        out = out_rows(self._EVAL_ROWS, n, dev, out, rows, strict=True)
        ptrs = (_ptr(out.get("value")), _ptr(out.get("logits")), _ptr(out.get("probs")), n)
        if symmetries is None:
            self._call("qttt_evaluate", self.state.data_ptr(), net.blob.data_ptr(), net.precision, *ptrs)
        else:
            self._call("qttt_evaluate_symmetric", self.state.data_ptr(), net.blob.data_ptr(), net.precision,
                       (ctypes.c_uint8 * len(lst))(*lst), len(lst), _ptr(sym), *ptrs)
        return out

    def rollout_policy(self, net, n_sims=1, step_idx0=None, with_plies=False, with_trace=False, leaf=(), out=None):
        """AlphaZero._rollout's simulations (alphazero.py:173-180) with _simulate (:192-205) under the policy/value
        network, n_sims per board in ONE launch (include/qttt_policy_rollout.h qttt_rollout_policy): every ply evaluates
        `net` on the board, samples an action from Categorical(logits) and a collapse branch, until the game ends.
        Returns a dict: result int8[N, n_sims] (AlphaZero._reward), and on request plies uint8[N, n_sims], trace
        uint8[N, n_sims, 9] (action36 | bit << 6 per ply, 0xFF after the last) and the leaf's network outputs `leaf` =
        a subset of ("value", "probs"): value f32[N] and probs f32[N, 36], equal to evaluate()'s.  Column s equals the
        one-simulation call with step_idx0 + 16 * s.  `out` = the dict of an earlier call: its tensors are overwritten
        and its keys decide what is written.  The boards and step_idx do not change; runs on the current stream."""
        n, S, dev = self.num_envs, int(n_sims), self.state.device
        check_net(net, dev)
        if not 1 <= S <= _native.POLICY_ROLLOUT_MAX_SIMS:
            raise ValueError("n_sims must be in 1..%d" % _native.POLICY_ROLLOUT_MAX_SIMS)
        if step_idx0 is None:
            step_idx0 = self.step_idx
        keys = None
        if out is None:
            leaf = (leaf,) if isinstance(leaf, str) else tuple(leaf)
            if any(r not in self._LEAF_ROWS for r in leaf):
                raise ValueError("leaf must be a subset of %s" % (tuple(self._LEAF_ROWS),))
            keys = ["result"] + (["plies"] if with_plies else []) + (["trace"] if with_trace else []) + list(leaf)
        out = out_rows(VecEnv._policy_rows(S), n, dev, out, keys, required=("result",), strict=True)
        self._call("qttt_rollout_policy", self.state.data_ptr(), net.blob.data_ptr(), net.precision, self.seed,
                   int(step_idx0), self.board_offset, S, out["result"].data_ptr(), _ptr(out.get("plies")),
                   _ptr(out.get("trace")), _ptr(out.get("value")), _ptr(out.get("probs")), n)
        return out

    # ------------------------------------------------------------------ hipGraph of T step launches
    def capture(self, n_steps, mode="random", actions=None, bits=None, actions_out=None, reward=None, terminated=None):
        """Captures n_steps step LAUNCHES into one hipGraph and returns it (`.replay()`): for loops on small
        batches, where one launch per step is host-bound (4-5 us per call against a ~3 us kernel at <= 262 144
        boards) and the policy must see the state every step, so the fused multi-step kernels do not apply.
        mode "random": step_random() x n_steps (actions_out u8[T,N,2] optional);
        mode "step" / "observe": step_raw / step_observe_raw reading actions u8[T,N,2] (bits u8[T,N] optional) —
        the caller's buffers, refilled between replays (e.g. by a policy network captured in its own graph).
        reward f32[T,N] + terminated bool[T,N] keep every step's outputs; without them the environment's own
        buffers hold the last step's.  The step index lives on the device from here on
        (use_device_step_counter), so every replay draws fresh collapse bits; the graph ends by advancing it."""
        T, n, dev = int(n_steps), self.num_envs, self.device
        if mode not in ("random", "step", "observe") or T < 1:
            raise ValueError("mode must be 'random', 'step' or 'observe' and n_steps >= 1")
        if mode == "random":
            if actions is not None or bits is not None:
                raise ValueError("mode 'random' draws its own actions (actions_out receives them)")
            if actions_out is not None:
                check_tensor(actions_out, torch.uint8, (T, n, 2), dev, "actions_out")
        else:
            if actions is None or actions_out is not None:
                raise ValueError("mode %r reads actions u8[T,N,2]" % mode)
            check_tensor(actions, torch.uint8, (T, n, 2), dev, "actions")
            if bits is not None:
                check_tensor(bits, torch.uint8, (T, n), dev, "bits")
        self._kept_outputs(T, reward, terminated)
        if mode == "observe":
            self._obs_buffers()
        ctr = self.use_device_step_counter()
        self._record()
        code = {"random": _native.ENV_STEP_RANDOM, "step": _native.ENV_STEP, "observe": _native.ENV_STEP_OBSERVE}[mode]
        recs = []
        for t in range(T):                     # one record per node: its own slice of the per-step outputs
            r = _native.EnvRecord.from_buffer_copy(self._rec)
            if reward is not None:
                r.reward, r.terminated = reward[t].data_ptr(), terminated[t].data_ptr()
            recs.append(r)
        a_src = actions_out if mode == "random" else actions

        def launch(t, step):
            self._call("qttt_env_step", ctypes.byref(recs[t]), _ptr(None if a_src is None else a_src[t]),
                       _ptr(None if bits is None else bits[t]), step, code)
        # the kernels' code objects must be resident before the capture: one eager launch of the same entry on a
        # scratch copy of the state, then everything it touched is put back
        written = [self.state, ctr, self._reward, self._terminated]
        written += [x[0] for x in (a_src, reward, terminated) if x is not None]
        written += list(self._obs.values()) if mode == "observe" else []
        saved = [x.clone() for x in written]
        launch(0, 0)
        self._call("qttt_counter_add", ctr.data_ptr(), 0)
        for x, s in zip(written, saved):
            x.copy_(s)
        graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                for t in range(T):
                    launch(t, t)
                self._call("qttt_counter_add", ctr.data_ptr(), T)
        torch.cuda.current_stream(self.device).wait_stream(side)
        return StepGraph(self, graph, T, mode, recs, (actions, bits, actions_out, reward, terminated))

    # ------------------------------------------------------------------ checkpointing
    def state_dict(self):
        return {"state": self.state.clone(), "seed": self.seed, "step_idx": self.step_idx,
                "board_offset": self.board_offset, "auto_reset": self.auto_reset}

    def load_state_dict(self, sd):
        if sd["state"].numel() != self.state.numel():
            raise ValueError("state size mismatch")
        self.state.copy_(sd["state"])
        self.seed, self.step_idx = int(sd["seed"]), int(sd["step_idx"])
        self.board_offset, self.auto_reset = int(sd["board_offset"]), bool(sd["auto_reset"])


class StepGraph:
    """A hipGraph of T step launches of one VecEnv (VecEnv.capture).  replay() enqueues all of them with ONE
    host call on the current stream; reward / terminated / the observation are where capture() was told to
    put them (or the environment's own buffers, holding the last step's)."""

    def __init__(self, env, graph, n_steps, mode, records, buffers):
        self.env, self.graph, self.n_steps, self.mode = env, graph, n_steps, mode
        self._keep = (records, buffers)            # the nodes hold raw pointers into these

    def replay(self):
        self.graph.replay()
        return self.env._reward, self.env._terminated
