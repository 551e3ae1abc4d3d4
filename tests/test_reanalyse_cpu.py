"""CPU tests of reanalysis (include/qttt_replay_reanalyse.h, qtttgym_amd.reanalyse): the header, the binding table and the
exports; every documented argument error of gather and update, in order, with no device; and the model
(tests/reanalyse_model.py) against brute force: holder, and the window's slots.  No GPU."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "qttt_replay_reanalyse.h")

import reanalyse_model as M  # noqa: E402
from qtttgym_amd import _native  # noqa: E402

ERR_NULL, ERR_SIZE, ERR_ACTION = -1, -2, -3
MAX = 1 << 30
NAMES = {"qttt_replay_gather", "qttt_replay_update"}


# ---------------------------------------------------------------- header, binding table, exports
def test_binding_header_exports_and_build_list_agree():
    import __graft_entry__ as entry
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = set(re.findall(r"^(?:int|int64_t)\s+(qttt_\w+)\s*\(", src, flags=re.M))
    assert names == set(_native.REPLAY_REANALYSE_SIGNATURES) == NAMES
    others = [getattr(_native, t) for t in dir(_native) if t.endswith("SIGNATURES") and t != "REPLAY_REANALYSE_SIGNATURES"]
    assert len(others) >= 19 and not any(names & set(t) for t in others)
    assert HEADER in entry.HEADERS
    L = _native.lib()                                        # resolves every table, this one included
    for name in names:
        assert getattr(ctypes.CDLL(_native.LIB_PATH), name)
        assert getattr(L, name).argtypes == _native.REPLAY_REANALYSE_SIGNATURES[name][1]
    assert L.qttt_abi_version() == _native.ABI_VERSION == 6             # additive entries: the ABI number stays
    m = re.search(r"#define QTTT_REPLAY_WINDOW_ID (0x[0-9a-fA-F]+)ull", src)
    assert m and int(m.group(1), 16) == _native.REPLAY_WINDOW_ID == M.WINDOW_ID == 1 << 32
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert all(name in text for name in NAMES), doc
    assert "qttt_replay_reanalyse.h" in open(os.path.join(ROOT, "include", "qttt_replay.h")).read()


def test_header_is_plain_c99_and_included_by_qttt_h():
    src = open(os.path.join(ROOT, "include", "qttt.h")).read()
    assert src.index('#include "qttt_replay.h"') < src.index('#include "qttt_replay_reanalyse.h"')
    prog = ('#include "qttt.h"\nint main(void){'
            'int (*g)(const void *, int64_t, int64_t, uint64_t, uint32_t, int64_t, void *, int32_t *, int64_t *, float *,'
            ' uint8_t *, void *) = qttt_replay_gather;\n'
            'int (*u)(void *, int64_t, int64_t, const int32_t *, const int64_t *, const double *, const float *, uint8_t *,'
            ' void *) = qttt_replay_update;\n'
            'return g == 0 || u == 0 || QTTT_REPLAY_WINDOW_ID != 4294967296ull || QTTT_ABI_VERSION != 6;}\n')
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-x", "c",
                          "-I" + os.path.join(ROOT, "include"), "-"], input=prog, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_the_package_exports_the_classes():
    import qtttgym_amd
    from qtttgym_amd import Reanalyser, ReanalyseStats, ReplayBuffer, ReplayWindow
    for name in ("Reanalyser", "ReanalyseStats", "ReplayWindow"):
        assert name in qtttgym_amd.__all__
    assert callable(ReplayBuffer.gather) and callable(ReplayBuffer.update) and callable(Reanalyser.run)
    assert isinstance(ReplayWindow.mask, property) and ReanalyseStats(1, 2, None).exact is None


# ---------------------------------------------------------------- argument errors
def _gather(L, replay=0x10000, capacity=8, n=1, draw=0, start=-1, state=0x20000, slot=0x21000, number=0x22000, v=0x23000,
            done=0x24001):
    """The entry with fake addresses (never dereferenced: every call of this file fails its checks first)."""
    return L.qttt_replay_gather(replay, capacity, n, 5, draw, start, state, slot, number, v, done, None)


def test_gather_return_codes_in_documented_order_without_device_work():
    L = _native.lib()
    nothing = dict(replay=None, state=None, slot=None, number=None, v=None, done=None)
    odd = dict(replay=0x10001, state=0x20001, slot=0x21001, number=0x22001, v=0x23001)
    for kw in (dict(capacity=0), dict(capacity=-3), dict(capacity=MAX + 1), dict(n=-1), dict(n=MAX + 1), dict(draw=1 << 31),
               dict(draw=(1 << 32) - 1)):
        assert _gather(L, **kw) == ERR_SIZE, kw
        assert _gather(L, **nothing, **kw) == ERR_SIZE, kw
        assert _gather(L, **odd, **kw) == ERR_SIZE, kw
    assert _gather(L, n=0, **nothing) == 0                    # nothing to do: no pointer is looked at, before the null checks
    assert _gather(L, n=0, draw=(1 << 31) - 1, start=12345, **odd) == 0
    assert _gather(L, n=0, draw=1 << 31) == ERR_SIZE          # (but the sizes still come first)
    assert _gather(L, n=0, capacity=0) == ERR_SIZE
    for k in ("replay", "state", "slot", "number"):           # nulls before any alignment
        kw = dict(odd)
        kw[k] = None
        assert _gather(L, **kw) == ERR_NULL, k
    # then alignment: replay 64 bytes, state_out 16, number_out 8, slot_out and v_out 4; done_out takes any address, and
    # v_out and done_out may be null (a call with every argument good is never made: it would launch)
    for replay in (0x10001, 0x10020):
        assert _gather(L, replay=replay) == ERR_ACTION
    for k, offs in (("state", (1, 4, 8)), ("number", (1, 4)), ("slot", (1, 2)), ("v", (1, 2))):
        for off in offs:
            kw = {k: dict(state=0x20000, number=0x22000, slot=0x21000, v=0x23000)[k] + off}
            assert _gather(L, **kw) == ERR_ACTION, (k, off)
            if k != "v":
                assert _gather(L, v=None, done=None, **kw) == ERR_ACTION, (k, off)


def _update(L, replay=0x10000, capacity=8, n=1, slot=0x20000, number=0x21000, pi=0x22000, v=0x23000, updated=0x24001):
    return L.qttt_replay_update(replay, capacity, n, slot, number, pi, v, updated, None)


def test_update_return_codes_in_documented_order_without_device_work():
    L = _native.lib()
    nothing = dict(replay=None, slot=None, number=None, pi=None, v=None, updated=None)
    odd = dict(replay=0x10001, slot=0x20001, number=0x21001, pi=0x22001, v=0x23001)
    for kw in (dict(capacity=0), dict(capacity=MAX + 1), dict(n=-1), dict(n=MAX + 1)):
        assert _update(L, **kw) == ERR_SIZE, kw
        assert _update(L, **nothing, **kw) == ERR_SIZE, kw
        assert _update(L, **odd, **kw) == ERR_SIZE, kw
    assert _update(L, n=0, **nothing) == 0                    # nothing to do, before the null checks
    assert _update(L, n=0, **odd) == 0
    assert _update(L, n=0, capacity=0) == ERR_SIZE            # (but the sizes still come first)
    for k in ("replay", "slot", "number"):                    # nulls before any alignment
        kw = dict(odd)
        kw[k] = None
        assert _update(L, **kw) == ERR_NULL, k
    assert _update(L, pi=None, v=None) == ERR_NULL            # one of the two targets at least
    assert _update(L, replay=0x10001, slot=0x20001, number=0x21001, pi=None, v=None) == ERR_NULL
    # then alignment: replay 64 bytes, pi and number 8, slot and v 4; updated_out takes any address or null
    for replay in (0x10001, 0x10020):
        assert _update(L, replay=replay) == ERR_ACTION
    for k, offs in (("pi", (1, 4)), ("number", (1, 4)), ("slot", (1, 2)), ("v", (1, 2))):
        for off in offs:
            kw = {k: dict(pi=0x22000, number=0x21000, slot=0x20000, v=0x23000)[k] + off}
            assert _update(L, **kw) == ERR_ACTION, (k, off)
            assert _update(L, updated=None, **kw) == ERR_ACTION, (k, off)
    assert _update(L, pi=None, v=0x23002) == ERR_ACTION and _update(L, pi=0x22004, v=None) == ERR_ACTION


# ---------------------------------------------------------------- the model
@pytest.mark.parametrize("capacity", [1, 7, 37, 64])
def test_holder_is_the_last_sample_number_of_the_slot(capacity):
    for written in range(3 * capacity + 1):
        for s in range(min(written, capacity)):
            brute = max(w for w in range(written) if w % capacity == s)
            assert M.holder(s, written, capacity) == brute, (written, s)
            assert brute % capacity == s and written - capacity <= brute < written


@pytest.mark.parametrize("capacity", [1, 7, 37, 64])
def test_a_window_has_no_duplicate_slot_and_nothing_past_what_the_ring_holds(capacity):
    for written in (0, 1, capacity - 1, capacity, capacity + 3, 3 * capacity):
        if written < 0:
            continue
        F = min(written, capacity)
        for start in (None, 0, 1, F - 1 if F else 0, F, 5 * capacity + 2):
            for n in sorted({0, 1, F // 2, F, F + 1, F + 9}):
                slots = M.window(n, written, capacity, start, seed=2026, draw=3)
                assert len(slots) == n
                held = slots[:min(n, F)]
                assert len(set(held)) == len(held) and all(0 <= s < F for s in held), (written, start, n)
                assert all(s == -1 for s in slots[F:])
                for a, b in zip(held, held[1:]):              # consecutive, with the one break at the wrap
                    assert b == (a + 1) % F
                if held and start is not None:
                    assert held[0] == start % F


def test_the_hashed_start_is_the_window_stream_and_no_minibatch_stream():
    h = _native.lib().qttt_hash
    F = 1 << 40
    starts = [M.window(1, F, F, None, seed=9, draw=d)[0] for d in range(64)]
    assert starts == [(int(h(9, 1 << 32, d)) * F) >> 64 for d in range(64)]
    assert len(set(starts)) == 64                             # one draw per call
    assert starts != [M.window(1, F, F, None, seed=10, draw=d)[0] for d in range(64)]
    # the hash folds board id 2^32 onto the 32-bit id 0x9E3779B9, past every minibatch index (n <= 2^30): no sample of a
    # minibatch draws the window's start
    assert int(h(9, 0x9E3779B9, 0)) == int(h(9, 1 << 32, 0)) and 0x9E3779B9 >= MAX
    assert all(int(h(9, i, 0)) != int(h(9, 1 << 32, 0)) for i in range(4096))
