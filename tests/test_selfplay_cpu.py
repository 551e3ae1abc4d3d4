"""CPU tests of the self-play record (include/qttt_selfplay.h, qtttgym_amd.SelfPlay): the header, the binding table and
the argument errors, and the Python model of the record (tests/selfplay_model.py) against the numpy expressions the
reference runs (self_play.py:195-216) and on whole games of the tree model.  No GPU."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "qttt_selfplay.h")

from qtttgym_amd import SelfPlay, _native  # noqa: E402

ERR_NULL, ERR_SIZE, ERR_ACTION = -1, -2, -3


# ---------------------------------------------------------------- header, binding table
def test_header_is_plain_c99_and_included_by_qttt_h_last():
    src = open(os.path.join(ROOT, "include", "qttt.h")).read()
    assert src.index('#include "qttt_tree_compact.h"') < src.index('#include "qttt_selfplay.h"')
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-x", "c",
                          "-I" + os.path.join(ROOT, "include"), "-"],
                         input='#include "qttt.h"\nint main(void){int (*f)(const void *, int64_t, int64_t, int, uint32_t, '
                               'double, double, double, void *, double *, uint8_t *, uint8_t *, float *, uint8_t *, '
                               'uint8_t *, int8_t *, uint8_t *, void *) = qttt_selfplay_record;\n'
                               'return f == 0 || QTTT_SELFPLAY_ROWS != 10 || QTTT_ABI_VERSION != 6;}\n',
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_binding_header_exports_and_build_list_agree():
    import __graft_entry__ as entry
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = set(re.findall(r"^(?:int|int64_t)\s+(qttt_\w+)\s*\(", src, flags=re.M))
    assert names == set(_native.SELFPLAY_SIGNATURES) == {"qttt_selfplay_record"}
    assert not names & (set(_native.SIGNATURES) | set(_native.TREE_SIGNATURES) | set(_native.TREE_COMPACT_SIGNATURES))
    assert HEADER in entry.HEADERS
    assert ctypes.CDLL(_native.LIB_PATH).qttt_selfplay_record
    L = _native.lib()                                        # resolves every table, this one included
    assert L.qttt_selfplay_record.argtypes == _native.SELFPLAY_SIGNATURES["qttt_selfplay_record"][1]
    assert L.qttt_abi_version() == _native.ABI_VERSION == 6             # an additive entry: the ABI number stays
    assert _native.SELFPLAY_ROWS == 10 and re.search(r"#define QTTT_SELFPLAY_ROWS 10\b", src)
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        assert "qttt_selfplay_record" in open(os.path.join(ROOT, doc)).read(), doc


# ---------------------------------------------------------------- argument errors
def _record(L, tree=0x1000, games=1, capacity=8, ply=0, n_rollouts=4, alpha=1.0, v_first=1.0, v_second=0.0, bufs=None):
    """The entry with fake addresses (never dereferenced: every call of this file fails its checks first)."""
    bufs = [0x2000 + 0x100 * k for k in range(9)] if bufs is None else bufs
    return L.qttt_selfplay_record(tree, games, capacity, ply, n_rollouts, alpha, v_first, v_second, *bufs, None)


def test_return_codes_in_documented_order_without_device_work():
    L = _native.lib()
    nothing = [None] * 9
    inf, nan = float("inf"), float("nan")
    # sizes first, even with null or misaligned pointers
    for kw in (dict(games=-1), dict(capacity=0), dict(capacity=(1 << 30) + 1), dict(ply=-1), dict(ply=10),
               dict(n_rollouts=0), dict(alpha=0.0), dict(alpha=-1.0), dict(alpha=nan), dict(alpha=inf),
               dict(v_first=nan), dict(v_first=-inf), dict(v_second=inf), dict(v_second=nan)):
        assert _record(L, **kw) == ERR_SIZE, kw
        assert _record(L, tree=None, bufs=nothing, **kw) == ERR_SIZE, kw
        assert _record(L, tree=0x1001, bufs=[0x2001] * 9, **kw) == ERR_SIZE, kw
    # games == 0: nothing to do, no pointer looked at
    assert _record(L, games=0, tree=None, bufs=nothing) == 0
    assert _record(L, games=0, tree=0x1001, bufs=[0x2001] * 9, ply=9) == 0
    assert _record(L, games=0, n_rollouts=0) == ERR_SIZE     # (but the sizes still come first)
    # then null pointers, before any alignment: the tree and each of the nine buffers
    assert _record(L, tree=None) == ERR_NULL
    assert _record(L, tree=None, bufs=[0x2001] * 9) == ERR_NULL
    for k in range(9):
        bufs = [0x2001] * 9
        bufs[k] = None
        assert _record(L, bufs=bufs) == ERR_NULL, k
        assert _record(L, tree=0x1008, bufs=bufs) == ERR_NULL, k
    # then alignment: tree and states 16 bytes, pi 8, v 4; the byte buffers take any address
    odd = [0x2000, 0x3000, 0x4001, 0x4003, 0x5000, 0x6001, 0x6003, 0x6005, 0x6007]
    assert _record(L, tree=0x1008, bufs=odd) == ERR_ACTION
    for k, off in ((0, 8), (0, 1), (1, 4), (1, 1), (4, 2), (4, 1)):         # states, pi, v
        bufs = list(odd)
        bufs[k] += off
        assert _record(L, bufs=bufs) == ERR_ACTION, (k, off)


def test_selfplay_checks_its_arguments_before_it_asks_for_a_device():
    for kw in (dict(num_games=-1), dict(n_rollouts=0), dict(alpha=0.0), dict(alpha=float("nan")),
               dict(value_targets=(1.0, float("inf"))), dict(carry=5), dict(compact=True, carry=-1)):
        with pytest.raises(ValueError):
            SelfPlay(**{"num_games": 4, **kw})
    with pytest.raises(_native.QtttNativeError):             # there is no CPU path
        SelfPlay(4, device="cpu")


# ---------------------------------------------------------------- the model against the reference's expressions
def _reference_pi(N, legal, n_rollouts, alpha):
    """self_play.py:208-211, verbatim but for the names."""
    a = np.array(legal, dtype=int)
    pi = np.zeros(36)
    pi[a] = (np.array([N[x] for x in legal]) / n_rollouts) ** alpha
    with np.errstate(invalid="ignore", divide="ignore"):
        pi /= np.sum(pi, axis=-1)
    return pi


def _random_roots(count, seed):
    rng = np.random.default_rng(seed)
    for _ in range(count):
        k = int(rng.integers(1, 37))
        legal = sorted(rng.choice(36, k, replace=False).tolist())
        n_rollouts = int(rng.choice([1, 3, 8, 100, 1000, 4097]))
        N = np.zeros(36, dtype=np.int64)
        cuts = np.sort(rng.integers(0, n_rollouts + 1, k - 1)) if k > 1 else np.array([], dtype=np.int64)
        N[legal] = np.diff(np.concatenate([[0], cuts, [n_rollouts]]))          # sums to n_rollouts, zeros included
        if rng.random() < 0.25:
            N[legal] = rng.integers(0, n_rollouts + 1, k)                      # a re-rooted tree: any total
            if not N.any():
                N[legal[0]] = 1
        yield N, legal, n_rollouts


def test_model_pi_is_the_reference_expression():
    import selfplay_model
    worst = 0.0
    for N, legal, n_rollouts in _random_roots(400, 2026):
        pi = selfplay_model.pi_row(N, legal, n_rollouts, 1.0)
        ref = _reference_pi(N, legal, n_rollouts, 1.0)
        # any two summation orders of 36 non-negative doubles differ by less than 2 * 35 * 2^-53 ~ 8e-15, relatively
        np.testing.assert_allclose(pi, ref, rtol=1e-14, atol=0.0)
        assert (pi[[a for a in range(36) if a not in legal]] == 0).all()
        assert abs(pi.sum() - 1.0) <= 1e-14
        worst = max(worst, float(np.max(np.abs(pi - ref) / np.where(ref > 0, ref, 1.0))))
        half = selfplay_model.pi_row(N, legal, n_rollouts, 0.5)               # two host pows, each within an ulp or so
        np.testing.assert_allclose(half, _reference_pi(N, legal, n_rollouts, 0.5), rtol=1e-12, atol=0.0)
    print("largest relative deviation from numpy's sum order: %.3g" % worst)


def test_model_wave_sum_is_the_documented_tree():
    import selfplay_model
    rng = np.random.default_rng(5)
    x = rng.random(36)
    s = list(x) + [0.0] * 28
    for m in (1, 2, 4, 8, 16, 32):
        s = [s[i] + s[i ^ m] for i in range(64)]
        assert all(s[i] == s[i ^ m] for i in range(64))          # commutative: both partners hold the same double
    assert selfplay_model.wave_sum(x) == s[0]
    assert len(set(s)) == 1
    # it is a sum order of its own: on some inputs it differs from the left-to-right sum in the last place
    differs = sum(selfplay_model.wave_sum(r) != float(np.add.reduce(r)) or selfplay_model.wave_sum(r) != sum(r.tolist())
                  for r in rng.random((200, 36)))
    assert differs > 0


def test_model_unvisited_root_gives_the_reference_nan_row():
    import selfplay_model
    legal = [0, 3, 17, 35]
    pi = selfplay_model.pi_row(np.zeros(36, dtype=np.int64), legal, 8, 1.0)
    ref = _reference_pi(np.zeros(36, dtype=np.int64), legal, 8, 1.0)
    assert np.isnan(pi[legal]).all() and np.isnan(ref[legal]).all()
    rest = [a for a in range(36) if a not in legal]
    assert (pi[rest] == 0).all()             # (numpy's in-place division makes the whole row NaN; the record keeps 0 here)
    assert np.isnan(selfplay_model.pi_row(np.zeros(36, dtype=np.int64), legal, 8, 0.5)[legal]).all()


def _reference_v(winner, rows, v_first, v_second):
    """self_play.py:195-199, 215-216 with the two targets as parameters (the reference's are 1 and, in effect, 0)."""
    v_target = 0
    if winner == 1:
        v_target = v_first
    elif winner == 0:
        v_target = v_second
    out = []
    for _ in range(rows):
        out.append(v_target)
        v_target = -v_target
    return out


@pytest.mark.parametrize("targets", [(1.0, 0.0), (1.0, -1.0)])
def test_model_value_targets_for_every_outcome(targets):
    import selfplay_model
    for winner in (1, 0, -1):
        for rows in range(1, 11):
            v = selfplay_model.value_targets(winner, rows, *targets)
            assert v.dtype == np.float32 and v.shape == (rows,)
            assert np.array_equal(v, np.array(_reference_v(winner, rows, *targets), dtype=np.float32))
            assert not np.signbit(v[v == 0]).any()                 # no -0.0
    assert selfplay_model.value_targets(0, 4, 1.0, -1.0).tolist() == [-1.0, 1.0, -1.0, 1.0]
    assert selfplay_model.value_targets(0, 4, 1.0, 0.0).tolist() == [0.0, 0.0, 0.0, 0.0]       # the reference's quirk
    assert selfplay_model.value_targets(1, 3, 1.0, 0.0).tolist() == [1.0, -1.0, 1.0]


def test_model_whole_games_keep_the_batch_invariants():
    import oracle
    import selfplay_model
    G, R, S = 5, 6, 2
    out, env = selfplay_model.play(G, R, S, seed=3, v_first=1.0, v_second=-1.0)
    w, t, _, _ = oracle.node_info(env)
    assert t.all() and np.array_equal(out["winner"], w)
    length = out["length"].astype(int)
    assert ((length >= 6) & (length <= 10)).all()            # a win needs three marks of one player: five moves
    for g in range(G):
        n = int(length[g])
        assert out["done"][:, g].tolist() == [0] * (n - 1) + [1] + [0] * (10 - n)
        assert int(env.b["n_moves"][g]) == n - 1 or (int(env.b["n_moves"][g]) == 9 and n - 1 == 8)   # the autofill move
        assert (out["action36"][:n - 1, g] < 36).all() and out["action36"][n - 1, g] == 255
        assert np.array_equal(out["v"][:n, g], selfplay_model.value_targets(w[g], n, 1.0, -1.0))
        for k in ("pi", "mask", "v", "action36"):
            assert not out[k][n:, g].any(), k
        assert all(out["recs"][i][g] is not None for i in range(n)) and all(out["recs"][i][g] is None for i in range(n, 10))
        np.testing.assert_allclose(out["pi"][:n, g].sum(-1), 1.0, rtol=0, atol=1e-14)
        assert (out["pi"][:n, g][out["mask"][:n, g] == 0] == 0).all()
        assert (out["pi"][n - 1, g] == 1.0 / 36.0).all() and out["mask"][n - 1, g].all()
    assert (out["actions"] == 255).all()                     # ply 9: every game is over
