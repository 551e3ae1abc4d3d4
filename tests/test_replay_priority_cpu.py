"""CPU tests of prioritised replay (include/qttt_replay_priority.h, include/qttt_train_weighted.h): the headers, the binding
tables and the exports; the layout; every documented argument error, in order, with no device; the model
(tests/priority_model.py) against brute force; and the host arithmetic as a stand-alone program under the host
sanitizers.  No GPU."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import priority_model as M  # noqa: E402
from qtttgym_amd import _native  # noqa: E402

ERR_NULL, ERR_SIZE, ERR_ACTION = -1, -2, -3
MAX = 1 << 30
NAMES = {"qttt_replay_priority_bytes", "qttt_replay_priority_layout", "qttt_replay_priority_sync",
         "qttt_replay_priority_update", "qttt_replay_sample_prioritized"}


def test_headers_binding_tables_and_exports_agree():
    import __graft_entry__ as entry
    for header, table, names in (("qttt_replay_priority.h", "REPLAY_PRIORITY_SIGNATURES", NAMES),
                                 ("qttt_train_weighted.h", "TRAIN_WEIGHTED_SIGNATURES", {"qttt_train_gradients_weighted"})):
        path = os.path.join(ROOT, "include", header)
        src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
        assert set(re.findall(r"^(?:int|int64_t)\s+(qttt_\w+)\s*\(", src, flags=re.M)) == set(getattr(_native, table)) == names
        others = [getattr(_native, t) for t in dir(_native) if t.endswith("SIGNATURES") and t != table]
        assert not any(names & set(t) for t in others)
        assert path in entry.HEADERS
        assert '#include "%s"' % header in open(os.path.join(ROOT, "include", "qttt.h")).read()
        L = _native.lib()
        for name in names:
            assert getattr(L, name).argtypes == getattr(_native, table)[name][1]
        for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
            text = open(os.path.join(ROOT, doc)).read()
            assert all(name in text for name in names), doc
    assert _native.lib().qttt_abi_version() == _native.ABI_VERSION == 6
    src = open(os.path.join(ROOT, "include", "qttt_replay_priority.h")).read()
    assert re.search(r"#define QTTT_PRIORITY_ONE \(1 << 16\)", src) and _native.PRIORITY_ONE == M.ONE == 65536
    for f in ("qttt_replay_priority_kernels.h", "qttt_replay_priority_host.h"):
        assert os.path.join(ROOT, "qtttgym_amd", "csrc", f) in entry.HEADERS


def test_headers_are_plain_c99():
    prog = ('#include "qttt.h"\nint main(void){'
            'int (*s)(const void *, void *, int64_t, void *) = qttt_replay_priority_sync;\n'
            'int (*u)(const void *, void *, int64_t, int64_t, const int32_t *, const int64_t *, const float *, uint8_t *, void *)'
            ' = qttt_replay_priority_update;\n'
            'int (*d)(const void *, const void *, int64_t, int64_t, uint64_t, uint32_t, const uint8_t *, int, float *, double *,'
            ' uint8_t *, float *, uint8_t *, int32_t *, uint8_t *, int64_t *, uint32_t *, uint64_t *, void *)'
            ' = qttt_replay_sample_prioritized;\n'
            'int (*g)(const float *, const double *, const uint8_t *, const float *, const uint8_t *, const float *, int64_t,'
            ' const void *, void *, float *, float *, void *, void *) = qttt_train_gradients_weighted;\n'
            'return s == 0 || u == 0 || d == 0 || g == 0 || QTTT_PRIORITY_ONE != 65536 || QTTT_ABI_VERSION != 6;}\n')
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-x", "c",
                          "-I" + os.path.join(ROOT, "include"), "-"], input=prog, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


@pytest.mark.parametrize("capacity,levels", [(1, 1), (255, 1), (256, 1), (257, 2), (65536, 2), (65537, 3), (1 << 24, 3),
                                             ((1 << 24) + 257, 4), (MAX, 4)])
def test_layout(capacity, levels):
    L = _native.lib()
    off, size = M.layout(capacity)
    n = M.level_sizes(capacity)
    assert len(off) == levels + 1 == len(n) and n[-1] == 1 and all(x > 1 for x in n[1:-1])
    at = 64
    for k, (o, cnt) in enumerate(zip(off, n)):
        assert o == at and o % 64 == 0
        at += -(-cnt * (4 if k == 0 else 8) // 64) * 64
    assert size == at
    assert L.qttt_replay_priority_bytes(0) == ERR_SIZE == L.qttt_replay_priority_bytes(MAX + 1)
    assert L.qttt_replay_priority_layout(0, (ctypes.c_int64 * 5)()) == ERR_SIZE
    assert L.qttt_replay_priority_layout(capacity, None) == ERR_NULL


def test_argument_errors_come_in_order_before_any_device_work():
    """Addresses that are never dereferenced: every call here returns before a launch (there is no device)."""
    L = _native.lib()
    A = 1 << 20                                               # a 64-byte-aligned address
    sync, upd, smp = L.qttt_replay_priority_sync, L.qttt_replay_priority_update, L.qttt_replay_sample_prioritized
    assert sync(None, None, 0, None) == ERR_SIZE == sync(A, A, MAX + 1, None)
    assert sync(None, A, 8, None) == ERR_NULL == sync(A + 1, None, 8, None)
    assert sync(A + 32, A, 8, None) == ERR_ACTION == sync(A, A + 8, 8, None)
    assert upd(None, None, 0, 1, None, None, None, None, None) == ERR_SIZE
    assert upd(A, A, 8, -1, A, A, A, A, None) == ERR_SIZE == upd(A, A, 8, MAX + 1, A, A, A, A, None)
    assert upd(None, None, 8, 0, None, None, None, None, None) == 0
    for k in range(5):
        args = [A + 1, A, A, A, A]
        args[k] = None
        assert upd(args[0], args[1], 8, 1, args[2], args[3], args[4], None, None) == ERR_NULL, k
    for k, delta in enumerate((32, 32, 2, 4, 2)):
        args = [A, A, A, A, A]
        args[k] += delta
        assert upd(args[0], args[1], 8, 1, args[2], args[3], args[4], None, None) == ERR_ACTION, k

    def sample(replay=A, prio=A, capacity=8, n=1, draw=0, outs=(A, A, A, A, A), index=A, sym_out=A, number=A, q=A, total=A):
        return smp(replay, prio, capacity, n, 1, draw, None, 0, *outs, index, sym_out, number, q, total, None)
    assert sample(None, None, capacity=0) == ERR_SIZE == sample(n=-1) == sample(n=MAX + 1) == sample(draw=1 << 31)
    assert sample(None, None, n=0, outs=(None,) * 5) == 0
    assert sample(replay=None) == ERR_NULL == sample(prio=None, replay=A + 1)
    for k in range(5):
        outs = [A + 1] * 5
        outs[k] = None
        assert sample(outs=tuple(outs)) == ERR_NULL, k
    assert sample(replay=A + 32) == ERR_ACTION == sample(prio=A + 32)
    for k, delta in enumerate((8, 8, 2, 2)):
        outs = [A] * 5
        outs[k] += delta
        assert sample(outs=tuple(outs)) == ERR_ACTION, k
    assert sample(index=A + 2) == ERR_ACTION == sample(number=A + 4) == sample(q=A + 2) == sample(total=A + 4)
    g = L.qttt_train_gradients_weighted
    B = 1 << 20
    assert g(B, B, B, B, B, B, 0, B, B, B, B, B, None) == ERR_SIZE
    assert g(B, B, B, B, B, None, 1, B, B, B, B, B, None) == ERR_NULL
    assert g(B, B, B, B, B, B + 2, 1, B, B, B, B, B, None) == ERR_ACTION


# ---------------------------------------------------------------- the model against brute force
def test_slot_rule_is_the_brute_force_cumulative_sum():
    rng = np.random.default_rng(3)
    for cap in (1, 5, 255, 256, 257, 700):
        t = M.Table(cap)
        t.q[:] = rng.integers(0, 50, cap)
        t.q[rng.integers(0, cap)] = M.QMAX                    # the sums leave 32 bits
        T = t.total()
        assert T == sum(int(x) for x in t.q)
        for seed in range(3):
            slots, qs, total = t.draw(seed, 7, 64)
            assert total == T
            h = _native.lib().qttt_hash
            for i, s in enumerate(slots):
                tt = (int(h(seed, i, 7)) * T) >> 64
                assert s == M.slot_of(t.q, tt) and t.q[s] > 0 and qs[i] == int(t.q[s])
    t = M.Table(4)
    assert t.draw(0, 0, 3) == ([-1] * 3, [0] * 3, 0)          # nothing has a priority


def test_equal_priorities_give_the_uniform_sampler():
    """With every q equal to c, t = mulhi64(h, F c) and slot = floor(t / c); that is mulhi64(h, F): floor(floor(h F c / 2^64)
    / c) = floor(h F / 2^64), the nested-floor identity for a positive integer c."""
    import replay_model
    h = _native.lib().qttt_hash
    for F, c in ((1, 65536), (7, 1), (500, 65536), (500, M.QMAX), (65537, 3)):
        t = M.Table(F)
        t.q[:] = c
        slots, _, T = t.draw(2026, 5, 200)
        assert T == F * c
        assert slots == replay_model.slot_stream(2026, 5, 200, F)
        for i in range(50):
            x = int(h(2026, i, 5))
            assert ((x * F * c) >> 64) // c == (x * F) >> 64


def test_quantiser_corners():
    Q = M.quantise
    assert Q(0.0) == 1 and Q(-1.0) == 1 and Q(float("nan")) == 1 and Q(float("inf")) == M.QMAX
    assert Q(2.0 ** -17) == 1                                 # 0.5 ties to the even 0, then the floor of 1
    assert Q(2.0 ** -16 * 1.5) == 2                           # 1.5 ties to the even 2
    assert Q(2.0 ** -16 * 2.5) == 2                           # 2.5 ties to the even 2
    assert Q(65536.0) == M.QMAX                               # 2^32 is clamped
    assert Q(65535.0) == 65535 << 16 and Q(1.0) == M.ONE and Q(3.4e38) == M.QMAX


def test_sync_update_and_the_max_rule():
    t = M.Table(8)
    t.sync(5)
    assert t.q.tolist() == [M.ONE] * 5 + [0] * 3 and t.seen == 5 and t.pmax == 0
    slot = np.array([1, 1, 1, 7, -1, 2, 3], np.int32)
    number = np.array([1, 1, 1, 7, 0, 3, 3], np.int64)         # slot 2 holds sample 2, not 3
    prio = np.array([2.0, 5.0, 3.0, 1.0, 1.0, 9.0, 0.25], np.float32)
    assert t.update(5, slot, number, prio).tolist() == [1, 1, 1, 0, 0, 0, 1]
    assert t.q.tolist() == [M.ONE, 5 * M.ONE, M.ONE, M.ONE // 4, M.ONE, 0, 0, 0] and t.pmax == 5 * M.ONE
    t.sync(5)
    assert t.q[1] == 5 * M.ONE                                # a second sync changes nothing
    t.sync(12)                                                # samples 5..11: slots 5, 6, 7, 0, 1, 2, 3 at pmax
    assert t.q.tolist() == [5 * M.ONE] * 4 + [M.ONE] + [5 * M.ONE] * 3 and t.seen == 12
    # stale numbers after the append: slot 1 now holds sample 9
    assert t.update(12, np.array([1, 4], np.int32), np.array([1, 4], np.int64), np.array([7.0, 7.0], np.float32)).tolist() == [0, 1]
    # an entry whose sample has not been given a priority yet (number >= seen) does not pass
    assert t.update(13, np.array([4], np.int32), np.array([12], np.int64), np.array([1.0], np.float32)).tolist() == [0]
    t2 = M.Table(4)
    t2.sync(100)                                              # more than capacity appended between two syncs
    assert t2.q.tolist() == [M.ONE] * 4
    assert t2.sums()[-1].tolist() == [4 * M.ONE]


def test_weights_of_a_uniform_table_are_all_one():
    for beta in (0.0, 0.4, 1.0):
        w = M.weights([M.ONE] * 9, 500 * M.ONE, 500, beta)
        assert w.dtype == np.float32 and (w == 1.0).all()
    w = M.weights([1, 2, 4], 7, 3, 1.0)
    assert np.array_equal(w, np.array([1.0, 0.5, 0.25], np.float32))


def test_frequencies_of_the_model_draw():
    """2^20 draws from 8 slots with priorities 1..8 (T = 36): slot s is drawn with probability p = q/T up to the 2^-64 of
    the hash's grid, so its count is binomial(n, p) and lies within 6 standard deviations sqrt(n p (1 - p)) of n p with
    probability 1 - 2e-9 per slot.  This tests the hash, not a kernel."""
    n = 1 << 20
    lib = ctypes.CDLL(_native.LIB_PATH)
    lib.qttt_hash.restype, lib.qttt_hash.argtypes = ctypes.c_uint64, [ctypes.c_uint64] * 3
    h = np.array([lib.qttt_hash(99, i, 3) for i in range(n)], np.uint64)
    T = 36
    t = (h >> np.uint64(32)) * np.uint64(T) + (((h & np.uint64(0xFFFFFFFF)) * np.uint64(T)) >> np.uint64(32)) >> np.uint64(32)
    assert all(int(t[i]) == (int(h[i]) * T) >> 64 for i in range(0, n, 4099))          # the split product is mulhi64
    cum = np.cumsum(np.arange(1, 9, dtype=np.uint64))
    counts = np.bincount(np.searchsorted(cum, t, side="right"), minlength=8)
    assert counts.sum() == n
    for s in range(8):
        p = (s + 1) / T
        assert abs(counts[s] - n * p) <= 6 * math.sqrt(n * p * (1 - p)), (s, counts[s], n * p)


def test_host_arithmetic_under_the_host_sanitizers(tmp_path):
    """tools/priority_host_check.cpp: the layout, the sync rule, the guard, the quantiser and every launch's index
    arithmetic replayed into exactly-sized arrays, as a stand-alone program with ASan and UBSan.  CPU only."""
    exe = tmp_path / "priority_host_check"
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "qtttgym_amd", "csrc"), os.path.join(ROOT, "tools", "priority_host_check.cpp"),
                           "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "priority_host_check: ok" in out.stdout, out.stdout + out.stderr
