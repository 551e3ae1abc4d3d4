"""CPU tests of the exact leaves of the device search trees (include/qttt_tree_exact.h, TreeSearch(exact_from=M)): the
header and the binding table; every argument error of the two entries, in order, without a device; the invariants of
tests/exact_leaves_model.py's model on roots from tests/golden/solve_positions.npz; the floor that keeps the GPU tests
from passing vacuously (every search they compare solves at least one node); and the keyword's host-side checks.
No GPU."""
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
HEADER = os.path.join(ROOT, "include", "qttt_tree_exact.h")
ERR_NULL, ERR_SIZE, ERR_ACTION = -1, -2, -3

import exact_leaves_model as E  # noqa: E402
import nn_reference64 as R  # noqa: E402
import solve_model  # noqa: E402
from qtttgym_amd import _native  # noqa: E402

NETS = {"zero": R.zero_state_dict, "greedy": R.greedy_state_dict, "counting": R.counting_state_dict,
        "sharp": R.sharp_counting_state_dict}


# ---------------------------------------------------------------- header, binding table
def test_header_is_plain_c99_and_included_by_qttt_h_after_the_solver():
    src = open(os.path.join(ROOT, "include", "qttt.h")).read()
    assert src.index('#include "qttt_solve.h"') < src.index('#include "qttt_tree_exact.h"')
    assert "qttt_tree_exact.h" in open(os.path.join(ROOT, "include", "qttt_tree.h")).read()
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-x", "c",
                          "-I" + os.path.join(ROOT, "include"), "-"],
                         input='#include "qttt.h"\nint main(void){'
                               'int (*s)(void *, int64_t, int64_t, int, const void *, const void *, int, float *, uint8_t *,'
                               ' void *) = qttt_tree_solve_leaves;\n'
                               'int (*b)(void *, int64_t, int64_t, int, const void *, const float *, const float *, void *)'
                               ' = qttt_tree_backup_batch_exact;\n'
                               'return s == 0 || b == 0 || QTTT_ABI_VERSION != 6 || QTTT_TREE_EXACT_MIN_PLY != 6'
                               ' || QTTT_TREE_NODE_SOLVED != 16 || QTTT_TREE_NODE_VALUE_SHIFT != 16'
                               ' || QTTT_TREE_NODE_VALUE_MASK != 0x3F0000;}\n',
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_binding_header_exports_and_build_list_agree():
    import __graft_entry__ as entry
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"^(?:int|int64_t)\s+(qttt_\w+)\s*\(", src, flags=re.M))
    assert names == set(_native.TREE_EXACT_SIGNATURES) == {"qttt_tree_solve_leaves", "qttt_tree_backup_batch_exact"}
    assert HEADER in entry.HEADERS
    L = _native.lib()
    for name in names:
        assert getattr(ctypes.CDLL(_native.LIB_PATH), name)
        assert getattr(L, name).argtypes == _native.TREE_EXACT_SIGNATURES[name][1]
    assert L.qttt_abi_version() == _native.ABI_VERSION == 6             # additive entries: the ABI number stays
    assert _native.TREE_EXACT_MIN_PLY == E.EXACT_MIN_PLY == 6 and _native.SOLVE_MAX_PLY == E.EXACT_MAX_PLY == 9
    assert _native.TREE_NODE_SOLVED == E.NODE_SOLVED == 16 and _native.TREE_NODE_VALUE_MASK == E.NODE_VALUE_MASK
    assert _native.TREE_NODE_VALUE_SHIFT == E.NODE_VALUE_SHIFT == 16
    for rule in ("ELIGIBLE", "benign", "bit 4", "bits 16-21", "NO priors"):
        assert rule in text, rule
    for doc in ("DESIGN.md", "README.md"):
        assert "qttt_tree_solve_leaves" in open(os.path.join(ROOT, doc)).read(), doc


# ---------------------------------------------------------------- argument errors, with fake addresses never dereferenced
def _solve(L, tree=0x1000, games=1, capacity=4, leaves=2, paths=0x2000, leaf=0x3000, min_ply=6, value=0x4000, exact=0x5000):
    return L.qttt_tree_solve_leaves(tree, games, capacity, leaves, paths, leaf, min_ply, value, exact, None)


def _backup(L, tree=0x1000, games=1, capacity=4, leaves=2, paths=0x2000, value=0x4000, probs=0x5000):
    return L.qttt_tree_backup_batch_exact(tree, games, capacity, leaves, paths, value, probs, None)


def test_return_codes_in_documented_order_without_device_work():
    L = _native.lib()
    sizes = (dict(games=-1), dict(capacity=0), dict(capacity=(1 << 30) + 1), dict(leaves=0), dict(leaves=-1), dict(leaves=65))
    for kw in sizes + (dict(min_ply=5), dict(min_ply=10), dict(min_ply=0), dict(min_ply=-1)):
        assert _solve(L, **kw) == ERR_SIZE, kw
        assert _solve(L, **{"tree": None, "paths": None, "leaf": None, **kw}) == ERR_SIZE, kw         # sizes before nulls
        assert _solve(L, **{"tree": 0x1001, "paths": 0x2001, "value": 0x4001, **kw}) == ERR_SIZE, kw  # and before alignment
        assert _solve(L, **{"games": 0, **kw}) == ERR_SIZE or kw == dict(games=-1), kw                # and before games == 0
    for kw in sizes:
        assert _backup(L, **kw) == ERR_SIZE, kw
        assert _backup(L, **{"tree": None, "paths": None, "value": None, "probs": None, **kw}) == ERR_SIZE, kw
        assert _backup(L, **{"tree": 0x1001, "value": 0x4001, **kw}) == ERR_SIZE, kw
        assert _backup(L, **{"games": 0, **kw}) == ERR_SIZE or kw == dict(games=-1), kw
    assert _solve(L, games=0, tree=None, paths=None, leaf=None) == 0             # nothing to do, no pointer looked at
    assert _solve(L, games=0, tree=0x1001, paths=0x2001, leaf=0x3001, value=0x4001) == 0
    assert _backup(L, games=0, tree=None, paths=None, value=None, probs=None) == 0
    assert _backup(L, games=0, tree=0x1001, paths=0x2001, value=0x4001, probs=0x5001) == 0
    for min_ply in (6, 7, 8, 9):                                                 # the whole range passes the size check
        assert _solve(L, min_ply=min_ply, tree=None) == ERR_NULL
    for kw in (dict(tree=None), dict(paths=None), dict(leaf=None)):
        assert _solve(L, **kw) == ERR_NULL, kw
        assert _solve(L, **{"tree": 0x1001, "paths": 0x2008, "leaf": 0x3004, "value": 0x4002, **kw}) == ERR_NULL, kw
    for kw in (dict(tree=None), dict(paths=None), dict(value=None), dict(probs=None)):
        assert _backup(L, **kw) == ERR_NULL, kw
        assert _backup(L, **{"tree": 0x1001, "paths": 0x2008, "value": 0x4002, "probs": 0x5001, **kw}) == ERR_NULL, kw
    for kw in (dict(tree=0x1008), dict(tree=0x1001), dict(paths=0x2008), dict(paths=0x2004)):
        assert _solve(L, **kw) == ERR_ACTION, kw
        assert _backup(L, **kw) == ERR_ACTION, kw
    for kw in (dict(leaf=0x3008), dict(leaf=0x3001), dict(value=0x4002), dict(value=0x4001)):
        assert _solve(L, **kw) == ERR_ACTION, kw
    for kw in (dict(value=0x4002), dict(value=0x4001), dict(probs=0x5002), dict(probs=0x5001)):
        assert _backup(L, **kw) == ERR_ACTION, kw
    # leaf_value and leaf_exact are nullable, and leaf_exact has no alignment: the next check is the launch itself, which
    # this test does not reach (no device), so only the order up to here is pinned


# ---------------------------------------------------------------- the keyword's host-side checks
def test_python_checks_exact_from_before_it_asks_for_a_device():
    from qtttgym_amd import SelfPlay, TreeSearch
    net = object()                    # never looked at: every call fails before
    for cls, kw in ((TreeSearch, dict(capacity=8)), (SelfPlay, dict(n_rollouts=2))):
        with pytest.raises(ValueError, match="exact_from needs a net and leaf_eval"):
            cls(4, net=net, leaf_eval="playouts", exact_from=6, **kw)
        with pytest.raises(ValueError, match="exact_from needs a net and leaf_eval"):
            cls(4, net=net, exact_from=6, **kw)
        with pytest.raises(ValueError, match="exact_from needs a net"):
            cls(4, net=None, leaf_eval="value", exact_from=6, **kw)
        with pytest.raises(ValueError, match="exact_from needs a net"):
            cls(4, exact_from=7, **kw)
        for bad in (5, 10, 0, -1, 6.5, True):
            with pytest.raises(ValueError, match=r"exact_from must be None or an integer in 6\.\.9"):
                cls(4, net=net, leaf_eval="value", exact_from=bad, **kw)
        assert inspect.signature(cls.__init__).parameters["exact_from"].default is None
    assert TreeSearch.check_exact_from("value", net, None) is None and TreeSearch.check_exact_from("playouts", None, None) is None
    assert [TreeSearch.check_exact_from("value", net, m) for m in (6, 7, 8, 9)] == [6, 7, 8, 9]


# ---------------------------------------------------------------- the model
def test_flag_bits_are_the_header_s():
    assert E.flag_bits(-1.0) == 16 and E.flag_bits(0.0) == 16 | (16 << 16) and E.flag_bits(1.0) == 16 | (32 << 16)
    assert E.flag_bits(-0.0625) == 16 | (15 << 16) and E.flag_bits(0.5) == 16 | (24 << 16)
    with pytest.raises(AssertionError):
        E.flag_bits(0.03125)


def test_without_exact_from_the_model_is_the_leaf_parallel_model():
    import leaf_parallel_model as LP
    import tree_model
    ob = E.boards_of(E.roots(9)[0])
    for K in (1, 4):
        a = E.ExactLeavesModel(1, seed=E.SEED, board_offset=E.OFFSET, net=NETS["sharp"](), leaves=K)
        b = LP.LeafParallelModel(1, seed=E.SEED, board_offset=E.OFFSET, net=NETS["sharp"](), leaves=K)
        for m in (a, b):
            m.reset(ob)
            m.contemplate(12)
        assert [tree_model.game_view(d) for d in a.dump()] == [tree_model.game_view(d) for d in b.dump()]
        assert not a.solved_counts().any()


def test_a_solved_leaf_is_backed_up_with_its_exact_value_and_stays_a_leaf():
    """One five-move root under the zero network (value 0, uniform priors): after R rollouts with exact_from = 6 every
    visited child is solved, W / N of a single-child action is the negated exact value of that child, and the children
    have neither priors nor children of their own; without exact_from the same search backs other values up."""
    arrays, idx = E.roots(1, played=5)
    ob = E.boards_of(arrays)
    m = E.ExactLeavesModel(1, seed=E.SEED, board_offset=E.OFFSET, net=NETS["zero"](), exact_from=6)
    m.reset(ob)
    m.contemplate(30)
    st = m.games[0]
    root = st["nodes"][0]
    assert m.check_invariants() == len(st["solved"]) > 0 and m.met["reused"] > 0
    q = E.fixture()["q"][idx[0]]
    seen = 0
    for a in root.legal:
        kids = root.children[a]
        if kids and len(kids) == 1 and root.N[a]:
            assert kids[0] in st["solved"] and root.W[a] / root.N[a] == float(q[a]) == 0.0 - st["solved"][kids[0]]
            seen += 1
        for c in kids or ():
            assert st["nodes"][c].P is None and all(k is None for k in st["nodes"][c].children)
    assert seen
    plain = E.ExactLeavesModel(1, seed=E.SEED, board_offset=E.OFFSET, net=NETS["zero"]())
    plain.reset(ob)
    plain.contemplate(30)
    assert plain.games[0]["nodes"][0].W != root.W and not plain.solved_counts().any()


# ---------------------------------------------------------------- the floor of tests/test_tree_exact_gpu.py
@pytest.mark.parametrize("case", E.WHOLE_CASES, ids=lambda c: "%s-K%d-M%d-cap%d" % c)
def test_every_search_that_the_gpu_tests_compare_solves_nodes_and_keeps_the_invariants(case):
    """Every parametrisation with exact_from 6 or 7 reports solved nodes, in the first three games and beyond, reuses a
    solved node, and the pool as a whole meets two descents of one round on one eligible leaf and (capacity 8) overflow.
    exact_from = 9 solves nothing, by the rules of the game: the ninth move fills the board, so a position with nine moves
    played is terminal and never eligible — that case is the GPU tests' `unchanged results` case, asserted as such."""
    net, K, M, capacity = case
    probs_of = None
    if net == "counting":              # the device's expf stands behind its softmax: here uniform stand-ins, the floor only
        probs_of = lambda leaves: np.full((leaves.n, 36), 1 / 36, dtype=np.float32)  # noqa: E731
    m = E.searched(NETS[net](), K, M, capacity, probs_of=probs_of)
    counts = m.solved_counts()
    assert m.check_invariants() == counts.sum() == m.met["enumerated"]
    assert m.in_flight() == 0
    if M == 9:
        assert not counts.any() and m.met["eligible"] == 0
        return
    assert counts[:3].sum() > 0 and counts[3:].sum() > 0 and m.met["reused"] > 0
    assert (m.met["same_eligible_leaf"] > 0) == (K > 1)
    overflowed = np.array([st["overflow"] for st in m.games])
    assert overflowed.any() == (capacity == E.OVERFLOW_CAPACITY)


def test_a_solved_leaf_that_becomes_the_root_gets_priors_and_children():
    stages, act, bits = E.searched(NETS["sharp"](), 4, 7, E.CAPACITY, stages=True)
    for compact in (False, True):
        m = stages["second", compact]
        assert m.met["solved_root_expanded"] > 0 and m.check_invariants() > 0
        expanded = 0
        for st in m.games:
            root = st["nodes"][st["root"]]
            if st["root"] in st["solved"] and not root.terminal:
                assert root.P is not None
                expanded += any(c is not None for c in root.children)
        assert expanded > 0
    assert solve_model.played(stages["synced"].games[0]["nodes"][stages["synced"].games[0]["root"]].rec.tobytes()) >= 5
