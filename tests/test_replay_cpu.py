"""CPU tests of the replay ring (include/qttt_replay.h, qtttgym_amd.replay): the header, the binding table and the
exports; the layout the library reports; every documented argument error of append and sample, with no device; and the
draw streams of the model (tests/replay_model.py), which are what the device must equal exactly.  No GPU."""
import ctypes
import math
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "qttt_replay.h")

import replay_model as M  # noqa: E402
from qtttgym_amd import _native  # noqa: E402

ERR_NULL, ERR_SIZE, ERR_ACTION = -1, -2, -3
MAX = 1 << 30
NAMES = {"qttt_replay_bytes", "qttt_replay_layout", "qttt_replay_append_scratch_bytes", "qttt_replay_append",
         "qttt_replay_sample"}


# ---------------------------------------------------------------- header, binding table, exports
def test_binding_header_exports_and_build_list_agree():
    import __graft_entry__ as entry
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = set(re.findall(r"^(?:int|int64_t)\s+(qttt_\w+)\s*\(", src, flags=re.M))
    assert names == set(_native.REPLAY_SIGNATURES) == NAMES
    others = [getattr(_native, t) for t in dir(_native) if t.endswith("SIGNATURES") and t != "REPLAY_SIGNATURES"]
    assert len(others) >= 12 and not any(names & set(t) for t in others)
    assert HEADER in entry.HEADERS
    for f in ("qttt_replay_kernels.h", "qttt_replay_host.h"):
        assert os.path.join(ROOT, "qtttgym_amd", "csrc", f) in entry.HEADERS
    L = _native.lib()                                        # resolves every table, this one included
    for name in names:
        assert getattr(ctypes.CDLL(_native.LIB_PATH), name)
        assert getattr(L, name).argtypes == _native.REPLAY_SIGNATURES[name][1]
    assert L.qttt_abi_version() == _native.ABI_VERSION == 6             # additive entries: the ABI number stays
    for const in ("MAX_CAPACITY", "MAX_GAMES", "SCAN_BLOCK"):
        m = re.search(r"#define QTTT_REPLAY_%s \(?([^)\s]+(?: << \d+)?)\)?" % const, src)
        assert m and eval(m.group(1)) == getattr(_native, "REPLAY_" + const), const
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert all(name in text for name in ("qttt_replay_append", "qttt_replay_sample")), doc
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all("`%s" % name in integration for name in names)


def test_header_is_plain_c99_and_included_by_qttt_h_after_the_gumbel_root():
    src = open(os.path.join(ROOT, "include", "qttt.h")).read()
    assert src.index('#include "qttt_tree_gumbel.h"') < src.index('#include "qttt_replay.h"')
    own = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert len(set(re.findall(r"\b(qttt_[a-z_0-9]+)\s*\(", own))) == 30      # qttt.h's own text declares what it did
    prog = ('#include "qttt.h"\nint main(void){'
            'int64_t (*b)(int64_t) = qttt_replay_bytes;\n'
            'int (*l)(int64_t, int64_t *) = qttt_replay_layout;\n'
            'int64_t (*c)(int64_t) = qttt_replay_append_scratch_bytes;\n'
            'int (*a)(void *, int64_t, int64_t, const void *, const double *, const uint8_t *, const uint8_t *, const float *,'
            ' const uint8_t *, void *, void *) = qttt_replay_append;\n'
            'int (*s)(const void *, int64_t, int64_t, uint64_t, uint32_t, const uint8_t *, int, float *, double *, uint8_t *,'
            ' float *, uint8_t *, int32_t *, uint8_t *, void *) = qttt_replay_sample;\n'
            'return b == 0 || l == 0 || c == 0 || a == 0 || s == 0 || QTTT_REPLAY_HEADER_BYTES != 64 || QTTT_ABI_VERSION != 6;}\n')
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-x", "c",
                          "-I" + os.path.join(ROOT, "include"), "-"], input=prog, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_the_package_exports_the_buffer_and_checks_capacity_before_it_asks_for_a_device():
    import qtttgym_amd
    from qtttgym_amd import ReplayBuffer
    assert "ReplayBuffer" in qtttgym_amd.__all__
    for bad in (0, -1, MAX + 1):
        with pytest.raises(ValueError):
            ReplayBuffer(bad)
    for method in ("add", "sample", "size", "views"):
        assert callable(getattr(ReplayBuffer, method))


# ---------------------------------------------------------------- the layout
ELEM = {"P": 8, "Q": 8, "pi": 288, "mask": 8, "v": 4, "done": 1}


@pytest.mark.parametrize("capacity", [1, 7, 8, 9, 37, 64, 65, 4096, 1000003, MAX])
def test_layout_is_aligned_ascending_without_overlap_and_the_size_agrees(capacity):
    off, total = M.layout(capacity)
    assert list(off) == list(_native.REPLAY_ARRAYS) == ["P", "Q", "pi", "mask", "v", "done"]
    end = 64                                                  # the header
    for name in _native.REPLAY_ARRAYS:
        assert off[name] % 64 == 0 and off[name] >= end, name     # aligned, ascending, behind what came before
        assert off[name] - end < 64                              # and no more than the padding apart
        end = off[name] + ELEM[name] * capacity
    assert end <= total < end + 64 and total % 64 == 0


def test_layout_and_scratch_errors():
    L = _native.lib()
    off = (ctypes.c_int64 * 6)(*[-7] * 6)
    for bad in (0, -1, MAX + 1, 1 << 62):
        assert L.qttt_replay_bytes(bad) == ERR_SIZE
        assert L.qttt_replay_layout(bad, off) == ERR_SIZE and L.qttt_replay_layout(bad, None) == ERR_SIZE
    assert list(off) == [-7] * 6                              # nothing written on an error
    assert L.qttt_replay_layout(5, None) == ERR_NULL
    for bad in (-1, MAX + 1):
        assert L.qttt_replay_append_scratch_bytes(bad) == ERR_SIZE
    # one word of `written`, seven of padding, then the levels: n, ceil(n / 256), ... down to the one total
    B = _native.REPLAY_SCAN_BLOCK
    assert B == 256
    for games, words in ((0, 0 + 0), (1, 1 + 1), (256, 256 + 1), (257, 257 + 2 + 1), (65536, 65536 + 256 + 1),
                         (65537, 65537 + 257 + 2 + 1), (MAX, MAX + (MAX >> 8) + (MAX >> 16) + (MAX >> 24) + 1)):
        assert L.qttt_replay_append_scratch_bytes(games) == 8 * (8 + words), games


# ---------------------------------------------------------------- argument errors
def _append(L, replay=0x10000, capacity=8, games=1, bufs=None, scratch=0x90000):
    """The entry with fake addresses (never dereferenced: every call of this file fails its checks first).
    bufs = states, pi, mask, done, v, length."""
    bufs = [0x20000 + 0x1000 * k for k in range(6)] if bufs is None else bufs
    return L.qttt_replay_append(replay, capacity, games, *bufs, scratch, None)


def test_append_return_codes_in_documented_order_without_device_work():
    L = _native.lib()
    nothing, odd = [None] * 6, [0x20001 + 0x1000 * k for k in range(6)]
    for kw in (dict(capacity=0), dict(capacity=-3), dict(capacity=MAX + 1), dict(games=-1), dict(games=MAX + 1)):
        assert _append(L, **kw) == ERR_SIZE, kw
        assert _append(L, replay=None, bufs=nothing, scratch=None, **kw) == ERR_SIZE, kw
        assert _append(L, replay=0x10001, bufs=odd, scratch=0x90001, **kw) == ERR_SIZE, kw
    assert _append(L, games=0, replay=None, bufs=nothing, scratch=None) == 0          # nothing to do, no pointer looked at
    assert _append(L, games=0, replay=0x10001, bufs=odd, scratch=0x90001) == 0
    assert _append(L, games=0, capacity=0) == ERR_SIZE                                  # (but the sizes still come first)
    assert _append(L, replay=None) == ERR_NULL and _append(L, scratch=None) == ERR_NULL
    for k in range(6):                                                                  # nulls before any alignment
        bufs = list(odd)
        bufs[k] = None
        assert _append(L, replay=0x10001, bufs=bufs, scratch=0x90001) == ERR_NULL, k
    # then alignment: replay 64 bytes, states 16, pi 8, v 4, scratch 8; mask, done and length take any address
    # (`good` itself is never passed: it would pass every check and launch)
    good = [0x20000, 0x21000, 0x22001, 0x23001, 0x24000, 0x25001]
    for replay in (0x10001, 0x10020):
        assert _append(L, replay=replay, bufs=good) == ERR_ACTION
    assert _append(L, bufs=good, scratch=0x90004) == ERR_ACTION
    for k, offs in ((0, (1, 8)), (1, (1, 4)), (4, (1, 2))):
        for off in offs:
            bufs = list(good)
            bufs[k] += off
            assert _append(L, bufs=bufs) == ERR_ACTION, (k, off)


def _sample(L, replay=0x10000, capacity=8, n=1, draw=0, sym=None, random_symmetry=0, outs=None, index=0x80000, sym_out=0x81001):
    """outs = s_out, pi_out, mask_out, v_out, done_out."""
    outs = [0x20000 + 0x1000 * k for k in range(5)] if outs is None else outs
    return L.qttt_replay_sample(replay, capacity, n, 5, draw, sym, random_symmetry, *outs, index, sym_out, None)


def test_sample_return_codes_in_documented_order_without_device_work():
    L = _native.lib()
    nothing, odd = [None] * 5, [0x20001 + 0x1000 * k for k in range(5)]
    for kw in (dict(capacity=0), dict(capacity=MAX + 1), dict(n=-1), dict(n=MAX + 1), dict(draw=1 << 31), dict(draw=(1 << 32) - 1)):
        assert _sample(L, **kw) == ERR_SIZE, kw
        assert _sample(L, replay=None, outs=nothing, index=None, sym_out=None, **kw) == ERR_SIZE, kw
        assert _sample(L, replay=0x10001, outs=odd, index=0x80001, **kw) == ERR_SIZE, kw
    assert _sample(L, n=0, replay=None, outs=nothing, index=None, sym_out=None) == 0   # nothing to do, no pointer looked at
    assert _sample(L, n=0, replay=0x10001, outs=odd, index=0x80001, draw=(1 << 31) - 1, random_symmetry=1) == 0
    assert _sample(L, n=0, draw=1 << 31) == ERR_SIZE                                    # (but the sizes still come first)
    assert _sample(L, replay=None) == ERR_NULL
    for k in range(5):                                                                  # nulls before any alignment
        outs = list(odd)
        outs[k] = None
        assert _sample(L, replay=0x10001, outs=outs, index=0x80001) == ERR_NULL, k
    # then alignment: replay 64 bytes, s_out and pi_out 16, mask_out, v_out and index_out 4; done_out, sym and sym_out
    # take any address, index_out and sym_out may be null (`good` itself is never passed)
    good = [0x20000, 0x21000, 0x22000, 0x23000, 0x24001]
    for replay in (0x10001, 0x10020):
        assert _sample(L, replay=replay, outs=good) == ERR_ACTION
    for off in (1, 2):
        assert _sample(L, outs=good, index=0x80000 + off) == ERR_ACTION
        assert _sample(L, outs=good, index=0x80000 + off, sym=0x70001, random_symmetry=1, sym_out=None) == ERR_ACTION
    for k, offs in ((0, (1, 4, 8)), (1, (1, 8)), (2, (1, 2)), (3, (1, 2))):
        for off in offs:
            outs = list(good)
            outs[k] += off
            assert _sample(L, outs=outs) == ERR_ACTION, (k, off)
            assert _sample(L, outs=outs, index=None, sym_out=None) == ERR_ACTION, (k, off)


# ---------------------------------------------------------------- the draw streams
def chi2_sf(x, dof):
    """P(X > x) for X chi-square with `dof` degrees of freedom, in closed form: the finite sums of the regularised
    incomplete gamma function Q(dof / 2, x / 2) for integer and half-integer first arguments."""
    h = x / 2.0
    if dof % 2 == 0:
        term, total = 1.0, 1.0
        for j in range(1, dof // 2):
            term *= h / j
            total += term
        return math.exp(-h) * total
    term, total = 1.0, 0.0                                    # sum over j = 0 .. (dof - 3) / 2 of h^(j + 1/2) / Gamma(j + 3/2)
    for j in range((dof - 1) // 2):
        term = math.sqrt(h) / math.gamma(1.5) if j == 0 else term * h / (j + 0.5)
        total += term
    return math.erfc(math.sqrt(h)) + math.exp(-h) * total


def chi2_upper_quantile(p, dof):
    """x with P(X > x) = p, by bisection on the survival function."""
    lo, hi = float(dof), 50.0 * dof
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if chi2_sf(mid, dof) > p else (lo, mid)
    return 0.5 * (lo + hi)


def test_the_chi_square_quantiles_are_the_distributions_own():
    # textbook values: P(X > 3.841) = 0.05 at 1 degree of freedom, 14.067 at 7, 50.998 at 36
    assert abs(chi2_upper_quantile(0.05, 1) - 3.8415) < 1e-3
    assert abs(chi2_upper_quantile(0.05, 7) - 14.0671) < 1e-3
    assert abs(chi2_upper_quantile(0.05, 36) - 50.9985) < 1e-3
    assert abs(chi2_sf(chi2_upper_quantile(1e-6, 36), 36) - 1e-6) < 1e-12
    assert abs(chi2_sf(chi2_upper_quantile(1e-6, 7), 7) - 1e-6) < 1e-12


def chi_square(counts, n):
    e = n / len(counts)
    return sum((c - e) ** 2 / e for c in counts)


@pytest.mark.parametrize("seed,draw", [(0, 0), (2026, 3), (2 ** 63 + 5, 2 ** 31 - 1)])
def test_the_slot_and_symmetry_streams_are_uniform(seed, draw):
    """F = 37 and 2^16 draws: a uniform stream exceeds the bound with probability 1e-6; a stuck bit, a short period or a
    biased multiply-high exceeds it by orders of magnitude."""
    n, F = 1 << 16, 37
    slots = M.slot_stream(seed, draw, n, F)
    assert min(slots) == 0 and max(slots) == F - 1
    stat = chi_square([slots.count(k) for k in range(F)], n)
    bound = chi2_upper_quantile(1e-6, F - 1)
    print("slots: chi-square %.2f, bound %.2f" % (stat, bound))
    assert stat < bound
    syms = M.symmetry_stream(seed, draw, n)
    assert min(syms) == 0 and max(syms) == 7
    stat = chi_square([syms.count(k) for k in range(8)], n)
    bound = chi2_upper_quantile(1e-6, 7)
    print("symmetries: chi-square %.2f, bound %.2f" % (stat, bound))
    assert stat < bound
    # the two streams of one call are different draws, and so are the streams of two calls
    assert M.slot_stream(seed, draw, 64, 1 << 40) != M.slot_stream(seed, draw ^ 1, 64, 1 << 40)
    assert [s >> 37 for s in M.slot_stream(seed, draw, 64, 1 << 40)] != syms[:64]


def test_the_model_ring_wraps_and_skips():
    import numpy as np
    rng = np.random.default_rng(1)
    G, stride = 5, 64
    ring = M.Ring(7)
    total = 0
    for rep in range(3):
        states = rng.integers(0, 256, (M.ROWS, 16 * stride), dtype=np.uint8)
        pi = rng.random((M.ROWS, G, 36))
        mask = rng.integers(0, 2, (M.ROWS, G, 36), dtype=np.uint8)
        done = rng.integers(0, 2, (M.ROWS, G), dtype=np.uint8)
        v = rng.random((M.ROWS, G)).astype(np.float32)
        length = np.array([3, 0, 12, 1, 10], np.uint8)              # 12 reads as 10
        n = ring.append(states, pi, mask, done, v, length)
        assert n == 24
        total += n
        assert ring.written == total and ring.filled == 7
        # the ring holds the last seven samples: rows 3..9 of the last game, sample number w in slot w % 7
        planes = states.view(np.uint64).reshape(M.ROWS, 2, stride)
        for t in range(3, 10):
            slot = (total - 10 + t) % 7
            assert ring.P[slot] == planes[t, 0, 4] and ring.Q[slot] == planes[t, 1, 4]
            assert ring.pi[slot].tolist() == pi[t, 4].view(np.uint64).tolist()
            assert ring.mask[slot] == sum(int(b) << a for a, b in enumerate(mask[t, 4]))
            assert ring.v[slot] == v[t, 4].view(np.uint32) and ring.done[slot] == done[t, 4]
