"""CPU tests of the exact targets of a self-play batch (include/qttt_selfplay_exact.h, SelfPlay(exact_targets=M)): the
header and the binding table; every argument error of the entry, in order, without a device; the keyword's host-side
checks; the invariants of tests/selfplay_exact_model.py's model on fixture boards; and the floor that keeps
tests/test_selfplay_exact_gpu.py from passing vacuously: what its inputs hold, shown by the model alone.  No GPU."""
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
HEADER = os.path.join(ROOT, "include", "qttt_selfplay_exact.h")
ERR_NULL, ERR_SIZE, ERR_ACTION = -1, -2, -3

import selfplay_exact_model as M  # noqa: E402
from qtttgym_amd import _native  # noqa: E402

ROWS = M.ROWS


# ---------------------------------------------------------------- header, binding table, documents
def test_header_is_plain_c99_and_included_by_qttt_h_after_the_exact_leaves():
    src = open(os.path.join(ROOT, "include", "qttt.h")).read()
    assert src.index('#include "qttt_tree_exact.h"') < src.index('#include "qttt_selfplay_exact.h"')
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-x", "c",
                          "-I" + os.path.join(ROOT, "include"), "-"],
                         input='#include "qttt.h"\nint main(void){'
                               'int (*f)(const void *, int64_t, int, int, const uint8_t *, const uint8_t *, const uint8_t *,'
                               ' const uint8_t *, double *, float *, uint8_t *, void *) = qttt_selfplay_exact_targets;\n'
                               'return f == 0 || QTTT_ABI_VERSION != 6 || QTTT_SELFPLAY_EXACT_MIN_PLY != 6'
                               ' || QTTT_SELFPLAY_EXACT_MAX_PLY != 9 || QTTT_SELFPLAY_EXACT_MIN_PLY != QTTT_TREE_EXACT_MIN_PLY'
                               ' || QTTT_SELFPLAY_EXACT_MAX_PLY != QTTT_SOLVE_MAX_PLY;}\n',
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_binding_header_exports_build_list_and_documents_agree():
    import __graft_entry__ as entry
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"^(?:int|int64_t)\s+(qttt_\w+)\s*\(", src, flags=re.M))
    assert names == set(_native.SELFPLAY_EXACT_SIGNATURES) == {"qttt_selfplay_exact_targets"}
    assert HEADER in entry.HEADERS
    L = _native.lib()
    fn = L.qttt_selfplay_exact_targets
    assert getattr(ctypes.CDLL(_native.LIB_PATH), "qttt_selfplay_exact_targets")
    assert fn.argtypes == _native.SELFPLAY_EXACT_SIGNATURES["qttt_selfplay_exact_targets"][1] and len(fn.argtypes) == 12
    assert L.qttt_abi_version() == _native.ABI_VERSION == 6             # an additive entry: the ABI number stays
    assert (_native.SELFPLAY_EXACT_MIN_PLY, _native.SELFPLAY_EXACT_MAX_PLY) == (M.MIN_PLY, M.MAX_PLY) == (6, 9)
    assert _native.SELFPLAY_EXACT_MIN_PLY == _native.TREE_EXACT_MIN_PLY and _native.SELFPLAY_EXACT_MAX_PLY == _native.SOLVE_MAX_PLY
    for rule in ("RELABELLED", "never -0.0", "1.0 / (double)k", "idempotent", "read only"):
        assert rule in text, rule
    for doc in ("DESIGN.md", "README.md"):
        body = open(os.path.join(ROOT, doc)).read()
        for name in ("qttt_selfplay_exact_targets", "exact_targets", "qttt_selfplay_exact.h"):
            assert name in body, (doc, name)
    assert "The batch's targets are not changed by it." not in open(os.path.join(ROOT, "qtttgym_amd", "selfplay.py")).read()


# ---------------------------------------------------------------- argument errors, with fake addresses never dereferenced
def _call(L, states=0x1000, games=1, min_ply=6, policy=1, rows=0x2000, length=0x3000, done=0x4000, mask=0x5000, pi=0x6000,
          v=0x7000, exact=0x8000):
    return L.qttt_selfplay_exact_targets(states, games, min_ply, policy, rows, length, done, mask, pi, v, exact, None)


REQUIRED = ("states", "length", "done", "mask", "pi", "v")


def test_return_codes_in_documented_order_without_device_work():
    L = _native.lib()
    nulls = {k: None for k in REQUIRED}
    crooked = dict(states=0x1008, pi=0x6004, v=0x7002)
    sizes = (dict(games=-1), dict(min_ply=5), dict(min_ply=10), dict(min_ply=0), dict(min_ply=-1), dict(policy=2),
             dict(policy=-1))
    for kw in sizes:
        assert _call(L, **kw) == ERR_SIZE, kw
        assert _call(L, **{**nulls, **kw}) == ERR_SIZE, kw                   # sizes before nulls
        assert _call(L, **{**crooked, **kw}) == ERR_SIZE, kw                 # and before alignment
        assert _call(L, **{"games": 0, **kw}) == ERR_SIZE or kw == dict(games=-1), kw      # and before games == 0
    assert _call(L, games=0, **nulls) == 0                                   # nothing to do, no pointer looked at
    assert _call(L, games=0, **crooked) == 0
    for min_ply in (6, 7, 8, 9):                                             # the whole range passes the size check
        for policy in (0, 1):
            assert _call(L, min_ply=min_ply, policy=policy, states=None) == ERR_NULL
    for k in REQUIRED:
        assert _call(L, **{k: None}) == ERR_NULL, k
        assert _call(L, **{**crooked, k: None}) == ERR_NULL, k              # nulls before alignment
        assert _call(L, **{k: None, "rows": None, "exact": None}) == ERR_NULL, k
    for kw in (dict(states=0x1008), dict(states=0x1001), dict(pi=0x6004), dict(pi=0x6001), dict(v=0x7002), dict(v=0x7001)):
        assert _call(L, **kw) == ERR_ACTION, kw
        assert _call(L, **{"rows": None, "exact": None, **kw}) == ERR_ACTION, kw
    # rows and exact are nullable and no buffer of bytes has an alignment: the next check is the launch itself, which this
    # test does not reach (no device), so only the order up to here is pinned


# ---------------------------------------------------------------- the keyword's host-side checks
def test_python_checks_exact_targets_before_it_asks_for_a_device():
    from qtttgym_amd import SelfPlay
    from qtttgym_amd.selfplay import SelfPlayBatch
    ok = dict(n_rollouts=2, value_targets=(1.0, -1.0))
    for bad in (5, 10, 0, -1, 6.5, True, "7", (7,), [6]):
        with pytest.raises(ValueError, match=r"exact_targets must be an integer in 6\.\.9"):
            SelfPlay(4, exact_targets=bad, **ok)
        with pytest.raises(ValueError, match=r"min_ply must be an integer in 6\.\.9"):
            SelfPlay.check_min_ply(bad, "min_ply")
    with pytest.raises(ValueError, match=r"min_ply must be an integer in 6\.\.9"):
        SelfPlay.check_min_ply(None, "min_ply")                               # SelfPlayBatch.exact_targets(None)
    for targets in ((1.0, 0.0), (1.0, -0.5), (-1.0, 1.0)):
        with pytest.raises(ValueError, match=r"exact_targets needs value_targets=\(1\.0, -1\.0\).*mover's.*not zero-sum"):
            SelfPlay(4, n_rollouts=2, value_targets=targets, exact_targets=6)
    with pytest.raises(ValueError, match="exact_targets needs value_targets"):
        SelfPlay(4, n_rollouts=2, exact_targets=6)                           # the default targets are the reference's (1, 0)
    sig = inspect.signature(SelfPlay.__init__).parameters
    assert sig["exact_targets"].default is None and sig["exact_policy"].default is True
    assert [SelfPlay.check_exact_targets(m, (1, -1)) for m in (6, 7, 8, 9)] == [6, 7, 8, 9]
    assert SelfPlay.check_exact_targets(None, (1.0, 0.0)) is None           # without the option any targets do
    # independent of exact_from, leaf_eval, root_policy and net: the other keywords' own checks are all that fire
    with pytest.raises(ValueError, match="exact_from needs a net"):
        SelfPlay(4, exact_targets=6, exact_from=6, **ok)
    sig = inspect.signature(SelfPlayBatch.exact_targets).parameters
    assert list(sig) == ["self", "min_ply", "policy", "rows"] and sig["policy"].default is True and sig["rows"].default is None
    doc = SelfPlay.__doc__
    assert "exact_targets=M" in doc and "The batch's targets are not changed by it." not in doc
    example = open(os.path.join(ROOT, "examples", "selfplay_train.py")).read()
    assert "--exact-targets" in example and "--exact-value-only" in example


# ---------------------------------------------------------------- the model's invariants on fixture boards
def _staged(name, G=None):
    """The fixture's boards with six to eight moves played as a staging batch: board i sits in row played[i]."""
    with np.load(os.path.join(M.GOLDEN, name)) as z:
        z = {k: z[k] for k in z.files}
    per = {t: np.flatnonzero(z["played"] == t) for t in range(4, 9)}
    G = G or min(len(v) for v in per.values() if len(v) >= 8)
    rows, value, q = [], np.full((ROWS, G), np.nan, np.float32), np.full((ROWS, G, 36), np.nan, np.float32)
    for t in range(ROWS):
        if t in per and len(per[t]) >= G:
            idx = per[t][:G]
            rows.append({k: z[k][idx] for k in M.ARRAYS})
            value[t], q[t] = z["value"][idx], z["q"][idx]
        else:
            rows.append({"board": np.zeros((G, 9), np.int8), "moves": np.full((G, 9, 2), 255, np.uint8),
                         "n_moves": np.zeros(G, np.uint8), "qmask": np.zeros((G, 4), np.uint16), "n_q": np.zeros(G, np.uint8)})
    rng = np.random.default_rng(11)
    return {"rows": rows, "length": np.full(G, 9, np.uint8), "done": np.zeros((ROWS, G), np.uint8),
            "mask": np.ones((ROWS, G, 36), np.uint8), "pi": rng.random((ROWS, G, 36)),
            "v": rng.choice(np.array([-1.0, 1.0], np.float32), (ROWS, G))}, value, q


@pytest.mark.parametrize("name", ["solve_positions.npz", "solve_deep.npz"])
def test_model_invariants_on_fixture_boards(name):
    b, value, q = _staged(name, G=32)
    args = (b["rows"], b["length"], b["done"], b["mask"], b["pi"], b["v"])
    played = M.played_per_row(b["rows"])
    seen = 0
    for m in (6, 7, 8):
        pi, v, exact = M.relabel(*args, m, True)
        assert not exact[played < m].any() and exact.any()
        hit = exact == 1
        seen += int(hit.sum())
        assert np.array_equal(M.bits(v[hit]), M.bits(value[hit]))                        # the fixture's own solution
        assert (v[hit] * 16 == np.round(v[hit] * 16)).all() and (np.abs(v[hit]) <= 1).all()
        assert not np.signbit(v[hit][v[hit] == 0]).any()
        best = q[hit] == value[hit][:, None]
        k = best.sum(1)
        assert (k >= 1).all() and np.array_equal(pi[hit] > 0, best)
        assert np.array_equal(pi[hit], np.where(best, 1.0 / k[:, None], 0.0)) and np.isfinite(q[hit][best]).all()
        assert np.array_equal(M.bits(pi[~hit]), M.bits(b["pi"][~hit])) and np.array_equal(M.bits(v[~hit]), M.bits(b["v"][~hit]))
        # a fixture leaf (a finished board) is never relabelled, whatever its row says
        leaves = np.isinf(q).all(2) & (played >= m)
        assert not exact[leaves].any()
        pi2, v2, exact2 = M.relabel(*args, m, False)
        assert np.array_equal(M.bits(pi2), M.bits(b["pi"])) and np.array_equal(M.bits(v2), M.bits(v))
        assert np.array_equal(exact2, exact)
        again = M.relabel(b["rows"], b["length"], b["done"], b["mask"], pi, v, m, True)      # idempotent
        assert all(np.array_equal(M.bits(x), M.bits(y)) for x, y in zip(again, (pi, v, exact)))
    assert seen > 0
    pi, v, exact = M.relabel(*args, 9, True)                                              # min_ply = 9: the identity
    assert not exact.any() and np.array_equal(M.bits(pi), M.bits(b["pi"])) and np.array_equal(M.bits(v), M.bits(b["v"]))
    short = b["length"].copy()
    short[::2] = 7
    done = b["done"].copy()
    done[8, 1] = 1
    pi, v, exact = M.relabel(b["rows"], short, done, b["mask"], b["pi"], b["v"], 6, True)
    assert not exact[7:, ::2].any() and not exact[8, 1] and exact[6, ::2].any() and exact[8, 3::2].any()


# ---------------------------------------------------------------- the floor of tests/test_selfplay_exact_gpu.py
def _facts(b, m):
    pi, v, exact = M.relabel(b["rows"], b["length"], b["done"], b["mask"], b["pi"], b["v"], m, True)
    return pi, v, exact, M.played_per_row(b["rows"])


def test_floor_the_recorded_plain_batches_are_not_vacuous():
    """The play(SEED) batches the GPU tests relabel (and assert to be these very bytes), by the model alone."""
    for (G, m), n in M.RELABELLED.items():                                                # the counts the GPU tests assert
        assert int(_facts(M.plain(G), m)[2].sum()) == n, (G, m)
    assert sum(n > 0 for n in M.RELABELLED.values()) >= 6 and all(M.RELABELLED[65, m] > 0 for m in (6, 7, 8))
    at = {G: _facts(M.plain(G), 6 if G == 3 else 7) for G in M.PLAIN_GAMES}
    pi, v, exact, played = at[3]
    assert 6 in played[exact == 1] and 7 in played[exact == 1]                           # G = 3 at min_ply 6; 8: below
    b = M.plain(65)
    pi, v, exact, played = at[65]
    hit = exact == 1
    assert (played[hit] == 7).any() and (played[hit] == 8).any() and not (played[hit] < 7).any()
    assert (M.bits(v[hit]) != M.bits(b["v"][hit])).any()                                  # a game outcome is replaced
    k = (pi[hit] > 0).sum(1)
    assert (k == 1).any() and (k > 1).any()
    live = (np.arange(ROWS)[:, None] < b["length"][None, :]) & (b["done"] == 0)
    assert (live & (played < 7)).any() and not exact[live & (played < 7)].any()          # a non-terminal row below min_ply
    # G = 65: 64-record workgroups, record r = t * 65 + g
    lists = np.bincount(np.flatnonzero(hit.reshape(-1)) // 64, minlength=11)
    assert (lists == 0).any() and (lists >= 2).any()
    assert at[1][2].shape == (ROWS, 1)
    assert (b["length"] >= 6).all() and (b["done"].sum(0) == 1).all() and set(np.unique(b["v"])) <= {-1.0, 0.0, 1.0}


def test_floor_the_fixture_batch_is_not_vacuous():
    """tests/selfplay_exact_model.fixture_batch(65), the GPU tests' staging batch of fixture boards."""
    b = M.fixture_batch(65)
    pi, v, exact, played = _facts(b, 6)
    hit = exact == 1
    assert sorted(set(played[hit].tolist())) == [6, 7, 8]
    frac = np.abs(v[hit] * 16) % 16 != 0
    assert frac.any() and (np.abs(v[hit] * 16) % 4 != 0).any()                            # fractional values, eighths among them
    k = (pi[hit] > 0).sum(1)
    assert (k == 1).any() and (k > 1).any()
    assert (M.bits(v[hit]) != M.bits(b["v"][hit])).any()
    live = (np.arange(ROWS)[:, None] < b["length"][None, :]) & (b["done"] == 0)
    assert (live & (played < 6) & (played > 0)).any() and not exact[played < 6].any()
    assert not exact[:, 16:64].any() and not exact[7:, 1].any() and not exact[7, 2] and exact[8, 2] == 1
    lists = np.bincount(np.flatnonzero(hit.reshape(-1)) // 64, minlength=11)
    assert (lists == 0).any() and (lists >= 2).any() and exact[:, 64].any()
    for m in (7, 8):
        assert _facts(b, m)[2].sum() > 0
