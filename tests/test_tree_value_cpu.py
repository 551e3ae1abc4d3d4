"""CPU tests of the value rollout (include/qttt_tree_value.h, TreeSearch(leaf_eval="value")): the header, the binding
table and the argument errors; the keyword's host-side checks; tests/value_tree_model.py's ValueTreeModel checked by
hand on small trees under the counting network; and the coverage floor: the root pool that tests/test_tree_value_gpu.py
searches drives the model through every branch the kernel has.  No GPU."""
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
HEADER = os.path.join(ROOT, "include", "qttt_tree_value.h")

import oracle  # noqa: E402
import tree_model  # noqa: E402
import value_tree_model as V  # noqa: E402
from nn_reference64 import counting_state_dict, forward64  # noqa: E402
from qtttgym_amd import _native  # noqa: E402

ERR_NULL, ERR_SIZE, ERR_ACTION = -1, -2, -3


# ---------------------------------------------------------------- header, binding table
def test_header_is_plain_c99_and_included_by_qttt_h_after_symmetry():
    src = open(os.path.join(ROOT, "include", "qttt.h")).read()
    assert src.index('#include "qttt_symmetry.h"') < src.index('#include "qttt_tree_value.h"')
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-x", "c",
                          "-I" + os.path.join(ROOT, "include"), "-"],
                         input='#include "qttt.h"\nint main(void){'
                               'int (*f)(void *, int64_t, int64_t, const void *, const void *, int, float *, float *, void *)'
                               ' = qttt_tree_value_rollout;\nreturn f == 0 || QTTT_ABI_VERSION != 6;}\n',
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_binding_header_exports_and_build_list_agree():
    import __graft_entry__ as entry
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"^(?:int|int64_t)\s+(qttt_\w+)\s*\(", src, flags=re.M))
    assert names == set(_native.TREE_VALUE_SIGNATURES) == {"qttt_tree_value_rollout"}
    assert not names & (set(_native.SIGNATURES) | set(_native.TREE_SIGNATURES) | set(_native.NN_SIGNATURES))
    assert HEADER in entry.HEADERS
    L = _native.lib()                                        # resolves every table, this one included
    for name in names:
        assert getattr(ctypes.CDLL(_native.LIB_PATH), name)
        assert getattr(L, name).argtypes == _native.TREE_VALUE_SIGNATURES[name][1]
    assert L.qttt_abi_version() == _native.ABI_VERSION == 6             # an additive entry: the ABI number stays
    for rule in ("The value rule", "leaf terminal", "The priors rule", "The non-finite rule"):
        assert rule in text, rule
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        assert "qttt_tree_value_rollout" in open(os.path.join(ROOT, doc)).read(), doc


# ---------------------------------------------------------------- argument errors
def _call(L, tree=0x1000, games=1, capacity=4, leaf=0x2000, weights=0x3000, precision=0, value=None, probs=None):
    """The entry with fake addresses (never dereferenced: every call of this file fails its checks first)."""
    return L.qttt_tree_value_rollout(tree, games, capacity, leaf, weights, precision, value, probs, None)


def test_return_codes_in_documented_order_without_device_work():
    L = _native.lib()
    for kw in (dict(games=-1), dict(capacity=0), dict(capacity=(1 << 30) + 1), dict(precision=2), dict(precision=-1)):
        assert _call(L, **kw) == ERR_SIZE, kw
        assert _call(L, tree=None, leaf=None, weights=None, **kw) == ERR_SIZE, kw            # sizes before nulls
        assert _call(L, tree=0x1001, weights=0x3001, value=0x4001, **kw) == ERR_SIZE, kw      # and before alignment
    assert _call(L, games=0, tree=None, leaf=None, weights=None) == 0      # nothing to do, no pointer looked at
    assert _call(L, games=0, tree=0x1001, weights=0x3001, value=0x4001, probs=0x5001, precision=1) == 0
    assert _call(L, games=0, precision=2) == ERR_SIZE                       # (but the sizes still come first)
    assert _call(L, games=0, capacity=0) == ERR_SIZE
    for kw in (dict(tree=None), dict(leaf=None), dict(weights=None)):
        assert _call(L, **kw) == ERR_NULL, kw
    assert _call(L, tree=None, weights=0x3001) == ERR_NULL                  # nulls before alignment
    assert _call(L, tree=0x1001, leaf=None) == ERR_NULL
    assert _call(L, tree=0x1008, weights=None, value=0x4002) == ERR_NULL
    for kw in (dict(tree=0x1008), dict(tree=0x1001), dict(weights=0x3008), dict(value=0x4002), dict(value=0x4001),
               dict(probs=0x5002), dict(value=0x4000, probs=0x5001)):
        assert _call(L, **kw) == ERR_ACTION, kw
        assert _call(L, precision=1, **kw) == ERR_ACTION, kw


def test_python_checks_leaf_eval_before_it_asks_for_a_device():
    from qtttgym_amd import SelfPlay, TreeSearch
    with pytest.raises(ValueError, match="net"):
        TreeSearch(4, capacity=8, leaf_eval="value", net=None)
    with pytest.raises(ValueError, match="leaf_eval"):
        TreeSearch(4, capacity=8, leaf_eval="values")
    with pytest.raises(ValueError, match="net"):
        SelfPlay(4, n_rollouts=2, leaf_eval="value")
    with pytest.raises(ValueError, match="leaf_eval"):
        SelfPlay(4, n_rollouts=2, leaf_eval="value head")
    assert TreeSearch.leaf_eval == "playouts"
    # a value search is bounded by the rollout index alone, whatever num_simulations says
    t = TreeSearch.__new__(TreeSearch)
    t.num_simulations, t.leaf_eval = 128, "value"
    assert t.max_rollouts == _native.TREE_MAX_ROLLOUTS
    t.leaf_eval = "playouts"
    assert t.max_rollouts == (1 << 31) // (128 * 16)


# ---------------------------------------------------------------- the model, by hand
NET = counting_state_dict()


def _value32(rec):
    """The counting network's value of one position: an integer, exact in f32."""
    import torch
    v = forward64(NET, torch.from_numpy(oracle.to_vector(oracle.OracleBoards.from_records([rec]))))[0]
    assert float(v[0]) == int(v[0])
    return float(v[0])


def _model(ob, capacity=None):
    m = V.ValueTreeModel(1, seed=3, board_offset=0, net=NET, capacity=capacity)
    m.reset(ob)
    return m


def _play(moves):
    """One board after the classical-free moves [(lo, hi), ...] (collapse bit 0 where a cycle closes)."""
    ob = oracle.OracleBoards(1)
    for lo, hi in moves:
        ob.step(np.array([[lo, hi]], dtype=np.uint8), np.zeros(1, dtype=np.uint8))
    return ob


def test_signs_alternate_from_minus_v_at_the_deepest_edge():
    """Tree 1, from the empty board: after every rollout the statistics of every edge are recomputed by hand from the
    recorded paths and the network's value of each leaf."""
    m = _model(oracle.OracleBoards(1))
    W, N = {}, {}                                            # by (node, action)
    deepest = 0
    for k in range(12):
        m.rollout()
        st = m.games[0]
        leaf = st["nodes"][st["leaf"]]
        assert not leaf.terminal
        v = _value32(leaf.rec)
        path = st["path"]
        deepest = max(deepest, len(path))
        for d, (i, a) in enumerate(path):
            edges_below = len(path) - 1 - d                  # the deepest edge has none below it and gets -v
            W[i, a] = W.get((i, a), 0.0) + (-v if edges_below % 2 == 0 else v)
            N[i, a] = N.get((i, a), 0) + 1
        for (i, a), w in W.items():
            assert st["nodes"][i].W[a] == w and st["nodes"][i].N[a] == N[i, a], (k, i, a)
        assert sum(sum(n.N) for n in st["nodes"]) == sum(N.values())
    assert deepest >= 2 and any(v != 0 for v in W.values())


@pytest.mark.parametrize("leaf_turn", [True, False])
@pytest.mark.parametrize("winner", [1, 0, -1])
def test_a_terminal_leaf_backs_up_the_reward(winner, leaf_turn):
    """Tree 2: a root, one edge, a terminal leaf made by hand with every winner under both leaf turns.  The network's
    value of the leaf (not 0, 1 or -1) must not appear."""
    m = _model(_play([(0, 1)] if leaf_turn else []))
    st = m.games[0]
    root = st["nodes"][0]
    assert root.turn != leaf_turn
    m.rollout()                                              # the root gets its priors
    m.select()                                               # expands one child: the leaf
    (i, a), = st["path"]
    leaf = st["nodes"][st["leaf"]]
    assert i == 0 and leaf.turn == leaf_turn and not leaf.terminal
    leaf.terminal, leaf.winner = True, winner                # a finished game, by decree
    assert abs(_value32(leaf.rec)) not in (0.0, 1.0)
    m.backup(np.array([_value32(leaf.rec)], dtype=np.float32), m.priors(oracle.OracleBoards.from_records([leaf.rec])))
    v = 0.0 if winner < 0 else (1.0 if (winner == 1) == leaf_turn else -1.0)       # for the player to move at the leaf
    assert root.W[a] == -v and root.N[a] == 1 and root.Ntot == 1
    assert leaf.P is None and leaf.probs is None             # a terminal leaf gets no priors
    assert (winner, leaf_turn) in m.ends["terminal"]


def test_a_leaf_receives_its_priors_in_the_rollout_that_reaches_it():
    """Tree 3, four plies in: the leaf of rollout k has no priors before the backup and the network's f32 row after it,
    so the next select that arrives there goes on below it; priors once given are never rewritten."""
    import policy_playout_model
    ob = oracle.OracleBoards(1)
    for t in range(4):
        ob.step(ob.sample_actions(11, t), None, 11, t)
    m = _model(ob)
    given = {}
    for k in range(10):
        leaves = m.select()
        st = m.games[0]
        leaf = st["nodes"][st["leaf"]]
        assert leaf.P is None and st["leaf"] not in given
        m.backup(m.playouts(leaves), m.priors(leaves))
        if leaf.terminal:
            assert leaf.P is None
            continue
        row = policy_playout_model.probs32(NET, leaves)[0]
        assert leaf.probs.dtype == np.float32 and leaf.probs.tobytes() == row.tobytes()
        assert leaf.P == {a: float(row[a]) for a in leaf.legal}
        given[st["leaf"]] = row.tobytes()
        for i, b in given.items():
            assert st["nodes"][i].probs.tobytes() == b
    d = m.dump()[0]
    assert all(n["P"] is None or isinstance(n["P"], np.ndarray) for n in d["nodes"])          # never "uniform"
    assert len(given) >= 5 and any(len(st["path"]) >= 2 for st in m.games)


# ---------------------------------------------------------------- the coverage floor
def test_the_root_pool_drives_the_model_through_every_branch():
    """The condition the GPU comparison rests on: over the roots that tests/test_tree_value_gpu.py searches (its G = 129
    pool, 40 rollouts, with its overflow capacity as well), the model ends rollouts on terminal leaves of all three
    winners under both leaf turns, on fresh leaves, and — in the small pool — on overflowed selects."""
    G = 129
    arrays = V.root_pool(G)
    plies = np.asarray(arrays["n_moves"]).astype(int)
    assert set(range(9)) <= set(plies.tolist()) and (plies >= 5).sum() > G // 2
    ob = oracle.boards_from_arrays(arrays["board"], arrays["moves"], arrays["n_moves"], arrays["qmask"], arrays["n_q"])
    terminal = oracle.node_info(ob)[1] != 0
    assert terminal.any() and not terminal.all()
    small = V.root_pool(65)
    assert all(np.array_equal(np.asarray(arrays[k])[:65], small[k]) for k in arrays)        # pools are prefixes
    ends = {}
    for capacity in (None, V.OVERFLOW_CAPACITY):
        m = V.ValueTreeModel(1, seed=5, board_offset=17, net=NET, capacity=capacity)
        m.reset(ob)
        for _ in range(40):
            m.rollout()
        ends[capacity] = m.ends
        assert m.ends["terminal"] == {(w, t) for w in (1, 0, -1) for t in (True, False)}, m.ends["terminal"]
        assert m.ends["fresh"] > 0
        assert any(len(st["path"]) >= 3 for st in m.games)
    assert ends[None]["overflowed"] == 0 and ends[V.OVERFLOW_CAPACITY]["overflowed"] > 0
