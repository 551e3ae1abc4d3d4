"""CPU tests of the search-value targets (include/qttt_selfplay_value.h, SelfPlay(value_mix= / td_lambda=)): the header and
the binding table; every argument error of the two entries, in order, without a device; the keywords' host-side checks; and
the properties of tests/selfplay_value_model.py's model on hand-built games.  No GPU."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "qttt_selfplay_value.h")
ERR_NULL, ERR_SIZE, ERR_ACTION = -1, -2, -3

import selfplay_value_model as M  # noqa: E402
from qtttgym_amd import _native  # noqa: E402

ROWS = M.ROWS


# ---------------------------------------------------------------- header, binding table, documents
def test_header_is_plain_c99_and_included_by_qttt_h_after_the_newest_header():
    src = open(os.path.join(ROOT, "include", "qttt.h")).read()
    assert src.index('#include "qttt_train_weighted.h"') < src.index('#include "qttt_selfplay_value.h"')
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-x", "c",
                          "-I" + os.path.join(ROOT, "include"), "-"],
                         input='#include "qttt.h"\nint main(void){'
                               'int (*f)(const void *, int64_t, int64_t, int, const uint8_t *, float *, const float *, void *)'
                               ' = qttt_selfplay_record_value;\n'
                               'int (*h)(int64_t, int, double, const uint8_t *, const uint8_t *, const uint8_t *,'
                               ' const uint8_t *, const float *, float *, void *) = qttt_selfplay_value_targets;\n'
                               'return f == 0 || h == 0 || QTTT_ABI_VERSION != 6 || QTTT_VALUE_MIX != 0 || QTTT_VALUE_TD != 1;}\n',
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_binding_header_exports_build_list_and_documents_agree():
    import __graft_entry__ as entry
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"^(?:int|int64_t)\s+(qttt_\w+)\s*\(", src, flags=re.M))
    assert names == set(_native.SELFPLAY_VALUE_SIGNATURES) == {"qttt_selfplay_record_value", "qttt_selfplay_value_targets"}
    assert HEADER in entry.HEADERS
    assert os.path.join(ROOT, "qtttgym_amd", "csrc", "qttt_selfplay_value_kernels.h") in entry.HEADERS
    L = _native.lib()
    raw = ctypes.CDLL(_native.LIB_PATH)
    for name, n_args in (("qttt_selfplay_record_value", 8), ("qttt_selfplay_value_targets", 10)):
        fn = getattr(L, name)
        assert getattr(raw, name)
        assert fn.argtypes == _native.SELFPLAY_VALUE_SIGNATURES[name][1] and len(fn.argtypes) == n_args
    assert L.qttt_selfplay_value_targets.argtypes[2] is ctypes.c_double
    assert L.qttt_abi_version() == _native.ABI_VERSION == 6             # additive entries: the ABI number stays
    assert (_native.VALUE_MIX, _native.VALUE_TD) == (M.MIX, M.TD) == (0, 1)
    for rule in ("BEFORE the ply's record kernel", "ascending action order", "There is no negation", "0 - x", "+0.0",
                 "bounded by 10", "lambda == 1"):
        assert rule in text, rule
    for doc in ("DESIGN.md", "README.md"):
        body = open(os.path.join(ROOT, doc)).read()
        for name in ("qttt_selfplay_record_value", "qttt_selfplay_value_targets", "td_lambda", "value_mix",
                     "qttt_selfplay_value.h"):
            assert name in body, (doc, name)


# ---------------------------------------------------------------- argument errors, with fake addresses never dereferenced
def _record(L, tree=0x1000, games=1, capacity=4, ply=0, length=0x2000, q=0x3000, v=0x4000):
    return L.qttt_selfplay_record_value(tree, games, capacity, ply, length, q, v, None)


def _targets(L, games=1, mode=1, lam=0.5, rows=0x1000, length=0x2000, done=0x3000, exact=0x4000, q=0x5000, v=0x6000):
    return L.qttt_selfplay_value_targets(games, mode, lam, rows, length, done, exact, q, v, None)


def test_record_value_return_codes_in_documented_order_without_device_work():
    L = _native.lib()
    required = ("tree", "length", "q", "v")
    nulls = {k: None for k in required}
    crooked = dict(tree=0x1008, q=0x3002, v=0x4001)
    sizes = (dict(games=-1), dict(capacity=0), dict(capacity=-1), dict(capacity=_native.TREE_MAX_CAPACITY + 1), dict(ply=10),
             dict(ply=1 << 20))
    for kw in sizes:
        assert _record(L, **kw) == ERR_SIZE, kw
        assert _record(L, **{**nulls, **kw}) == ERR_SIZE, kw                 # sizes before nulls
        assert _record(L, **{**crooked, **kw}) == ERR_SIZE, kw               # and before alignment
        assert _record(L, **{"games": 0, **kw}) == ERR_SIZE or kw == dict(games=-1), kw      # and before games == 0
    assert _record(L, games=0, **nulls) == 0                                 # nothing to do, no pointer looked at
    assert _record(L, games=0, **crooked) == 0
    for ply in (-1, -7, 0, 9):                                               # every ply in range passes the size check
        assert _record(L, ply=ply, tree=None) == ERR_NULL
    for k in required:
        assert _record(L, **{k: None}) == ERR_NULL, k
        assert _record(L, **{**crooked, k: None}) == ERR_NULL, k             # nulls before alignment
    for kw in (dict(tree=0x1008), dict(tree=0x1001), dict(q=0x3002), dict(q=0x3001), dict(v=0x4002), dict(v=0x4001)):
        assert _record(L, **kw) == ERR_ACTION, kw


def test_value_targets_return_codes_in_documented_order_without_device_work():
    L = _native.lib()
    required = ("length", "done", "q", "v")
    nulls = {k: None for k in required}
    crooked = dict(q=0x5002, v=0x6001)
    sizes = (dict(games=-1), dict(mode=2), dict(mode=-1), dict(lam=-0.001), dict(lam=1.001), dict(lam=float("nan")),
             dict(lam=float("inf")), dict(lam=-float("inf")))
    for kw in sizes:
        assert _targets(L, **kw) == ERR_SIZE, kw
        assert _targets(L, **{**nulls, **kw}) == ERR_SIZE, kw
        assert _targets(L, **{**crooked, **kw}) == ERR_SIZE, kw
        assert _targets(L, **{"games": 0, **kw}) == ERR_SIZE or kw == dict(games=-1), kw
    assert _targets(L, games=0, **nulls) == 0
    assert _targets(L, games=0, **crooked) == 0
    for mode in (0, 1):
        for lam in (0.0, 0.5, 1.0):                                          # the whole range passes the size check
            assert _targets(L, mode=mode, lam=lam, v=None) == ERR_NULL
    for k in required:
        assert _targets(L, **{k: None}) == ERR_NULL, k
        assert _targets(L, **{**crooked, k: None}) == ERR_NULL, k
        assert _targets(L, **{k: None, "rows": None, "exact": None}) == ERR_NULL, k
    for kw in (dict(q=0x5002), dict(q=0x5001), dict(v=0x6002), dict(v=0x6001)):
        assert _targets(L, **kw) == ERR_ACTION, kw
        assert _targets(L, **{"rows": None, "exact": None, **kw}) == ERR_ACTION, kw
    # rows and exact are nullable bytes: the next check is the launch itself, which this test does not reach (no device)


def test_the_host_header_under_the_sanitizers(tmp_path):
    """tools/value_host_check.cpp: the argument checks and one game's row arithmetic — the code the kernel's lanes run —
    over random batches in exactly-sized arrays, as a stand-alone program with ASan and UBSan.  CPU only."""
    exe = tmp_path / "value_host_check"
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "qtttgym_amd", "csrc"), os.path.join(ROOT, "tools", "value_host_check.cpp"),
                           "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "value_host_check: ok" in out.stdout, out.stdout + out.stderr


# ---------------------------------------------------------------- the keywords' host-side checks
def test_python_checks_the_keywords_before_it_asks_for_a_device():
    from qtttgym_amd import SelfPlay
    from qtttgym_amd.selfplay import SelfPlayBatch
    ok = dict(n_rollouts=2, value_targets=(1.0, -1.0))
    with pytest.raises(ValueError, match="at most one of value_mix and td_lambda"):
        SelfPlay(4, value_mix=0.5, td_lambda=0.8, **ok)
    for kw in ("value_mix", "td_lambda"):
        for targets in ((1.0, 0.0), (1.0, -0.5), (-1.0, 1.0)):
            with pytest.raises(ValueError, match=kw + r" needs value_targets=\(1\.0, -1\.0\): the searched value is the "
                                                      r"mover's, in \[-1, 1\], and the reference's \(1, 0\) is not zero-sum, "
                                                      r"so the mixed v would be on two scales"):
                SelfPlay(4, n_rollouts=2, value_targets=targets, **{kw: 0.5})
        with pytest.raises(ValueError, match=kw + " needs value_targets"):
            SelfPlay(4, n_rollouts=2, **{kw: 0.5})                           # the default targets are the reference's (1, 0)
        for bad in (-0.1, 1.5, float("nan"), float("inf"), "0.5", True, (0.5,)):
            with pytest.raises(ValueError, match=kw + r" must be a number in \[0, 1\]"):
                SelfPlay(4, **{kw: bad}, **ok)
    # the words are Reanalyser's own (qtttgym_amd/reanalyse.py), from "needs" on
    src = open(os.path.join(ROOT, "qtttgym_amd", "reanalyse.py")).read()
    flat = re.sub(r'"\s*\n\s*"', "", src)
    assert ("needs value_targets=(1.0, -1.0): the searched value is the mover's, in [-1, 1], and the reference's (1, 0) is "
            "not zero-sum, so the mixed v would be on two scales") in flat
    assert SelfPlay.check_value_args(None, None, (1.0, 0.0)) == (None, None)  # without the keywords any targets do
    assert SelfPlay.check_value_args(0.5, None, (1, -1)) == ("mix", 0.5)
    assert SelfPlay.check_value_args(None, 1, (1, -1)) == ("td", 1.0)
    assert SelfPlay.check_value_args(0, None, (1, -1)) == ("mix", 0.0)
    sig = inspect.signature(SelfPlay.__init__).parameters
    assert sig["value_mix"].default is None and sig["td_lambda"].default is None
    sig = inspect.signature(SelfPlayBatch.value_targets).parameters
    assert list(sig) == ["self", "mode", "lam", "rows", "exact"] and sig["rows"].default is None and sig["exact"].default is None
    assert "q" not in SelfPlayBatch._ROWS and "q" not in SelfPlayBatch._FIELDS
    assert "an augmented batch has no q" in " ".join(SelfPlayBatch.__doc__.split())
    doc = SelfPlay.__doc__
    assert "value_mix=L or td_lambda=L" in doc and "BEFORE its record" in doc
    example = open(os.path.join(ROOT, "examples", "selfplay_train.py")).read()
    assert "--value-mix" in example and "--td-lambda" in example


# ---------------------------------------------------------------- the model's own properties on hand-built games
def _game(L, v0, q, exact=None):
    v, done = M.outcome_game(L, v0)
    e = None if exact is None else np.asarray(exact, np.uint8).reshape(ROWS, 1)
    return dict(rows=None, length=np.array([L], np.uint8), done=done.reshape(ROWS, 1), exact=e,
                q=np.asarray(q, np.float32).reshape(ROWS, 1), v=v.reshape(ROWS, 1))


def _run(mode, lam, b):
    return M.value_targets(mode, lam, b["rows"], b["length"], b["done"], b["exact"], b["q"], b["v"])


def test_model_td_with_lambda_one_is_the_outcome_and_mix_with_zero_the_identity():
    rng = np.random.default_rng(5)
    for L in range(1, ROWS + 1):
        for v0 in (1.0, -1.0, 0.0):
            b = _game(L, v0, rng.standard_normal(ROWS))
            assert np.array_equal(M.bits(_run("td", 1.0, b)), M.bits(b["v"])), (L, v0)
            assert np.array_equal(M.bits(_run("mix", 0.0, b)), M.bits(b["v"])), (L, v0)
            assert np.array_equal(M.bits(_run(M.TD, 1.0, b)), M.bits(b["v"]))             # the modes by number too
    for sixteenths in (True, False):
        for kind in ("none", "zero", "late"):
            b = M.hand_batch(65, 3, sixteenths, kind, short_rows=True)
            for rows in (None, b["rows"]):
                got = M.value_targets("td", 1.0, rows, b["length"], b["done"], b["exact"], b["q"], b["v"])
                if kind != "late":                                   # an exact row holds another value than the outcome
                    assert np.array_equal(M.bits(got), M.bits(b["v"]))
                got = M.value_targets("mix", 0.0, rows, b["length"], b["done"], b["exact"], b["q"], b["v"])
                assert np.array_equal(M.bits(got), M.bits(b["v"]))


def test_model_one_step_target_mix_and_the_hand_computed_return():
    q = np.array([0.5, -0.25, 0.125, 0.75, 0, 0, 0, 0, 0, 0], np.float32)
    b = _game(4, 1.0, q)                                                     # v = 1, -1, 1, -1; row 3 is terminal
    one = _run("td", 0.0, b)[:, 0]
    assert one[:4].tolist() == [0.25, -0.125, 1.0, -1.0]                     # -q[1], -q[2], -v[3] (terminal), row 3 kept
    lam = 0.5
    g2 = -(-1.0)                                                             # b is the terminal outcome whatever lambda
    g1 = -((1 - lam) * 0.125 + lam * g2)
    g0 = -((1 - lam) * -0.25 + lam * g1)
    assert _run("td", lam, b)[:4, 0].tolist() == [np.float32(g0), np.float32(g1), np.float32(g2), -1.0]
    mix = _run("mix", 0.5, b)[:, 0]
    assert mix[:4].tolist() == [0.75, -0.625, 0.5625, -1.0]                  # the terminal row keeps its outcome
    assert np.array_equal(_run("mix", 1.0, b)[:3, 0], q[:3])
    assert not _run("td", 0.3, b)[4:].any() and not _run("mix", 0.3, b)[4:].any()       # rows at or past L


def test_model_an_exact_row_stops_the_recursion():
    q = np.array([0.5, -0.25, 0.125, 0.75, 0.375, 0, 0, 0, 0, 0], np.float32)
    exact = np.zeros(ROWS, np.uint8)
    exact[2] = 1
    b = _game(5, -1.0, q, exact)
    b["v"][2, 0] = 0.625                                                     # the truth of row 2
    for lam in (0.0, 0.5, 0.8, 1.0):
        got = _run("td", lam, b)[:, 0]
        assert got[2] == np.float32(0.625) and got[4] == b["v"][4, 0]
        assert got[1] == np.float32(-0.625)                                  # b = v[2] and g[2] = v[2]: -v[2] whatever lambda
        assert got[0] == np.float32(-((1 - lam) * -0.25 + lam * -0.625))
        tail = _game(5, -1.0, q)                                             # rows 3 and 4 do not know of the exact row
        assert got[3] == _run("td", lam, tail)[3, 0]
        other = dict(b, q=b["q"].copy())
        other["q"][3:, 0] += 1.0                                             # nothing behind the exact row reaches rows 0..2
        assert np.array_equal(_run("td", lam, other)[:3, 0], got[:3])
        mix = _run("mix", lam, b)[:, 0]
        assert mix[2] == np.float32(0.625)


def test_model_a_game_of_length_one_rows_zero_and_no_negative_zero():
    for mode in ("td", "mix"):
        for lam in (0.0, 0.5, 1.0):
            b = _game(1, 1.0, np.full(ROWS, 0.5))
            assert np.array_equal(M.bits(_run(mode, lam, b)), M.bits(b["v"]))            # one terminal row: nothing to do
            b = _game(6, 1.0, np.full(ROWS, 0.5))
            b["rows"] = np.array([0], np.uint8)
            assert np.array_equal(M.bits(_run(mode, lam, b)), M.bits(b["v"]))
            b["rows"] = np.array([1], np.uint8)                              # one row looked at, not terminal
            got = _run(mode, lam, b)
            assert np.array_equal(got[1:], b["v"][1:])
            assert got[0, 0] == (1.0 if mode == "td" else np.float32((1 - lam) * 1.0 + lam * 0.5))
    tiny = np.float32(1e-45)                                                 # the least f32: half of it rounds to zero
    b = _game(3, 0.0, np.array([-tiny, tiny, 0, 0, 0, 0, 0, 0, 0, 0]))
    assert tiny > 0 and np.signbit(np.float32(np.float64(tiny) * -0.5))      # what a plain rounding would store
    for mode in ("td", "mix"):
        got = _run(mode, 0.5, b)                                             # td: v[0] = -(0.5 q[1]); mix: v[0] = 0.5 q[0]
        assert not got[:3].any() and not np.signbit(got).any() and not np.isnan(got).any()
    assert M.search_value(np.zeros(36), np.zeros(36, np.int32), np.float32(-1.0)) == np.float32(-1.0)
    W = np.zeros(36)
    N = np.zeros(36, np.int32)
    W[3], N[3], W[20], N[20] = -1e-50, 4, 0.0, 4
    x = M.search_value(W, N, np.float32(1.0))
    assert x == 0 and not np.signbit(x)
    W[3], W[20] = 3.0, -1.5
    assert M.search_value(W, N, np.float32(1.0)) == np.float32(1.5 / 8)
