"""CPU tests of the proven interior nodes of the device search trees (include/qttt_tree_prove.h, TreeSearch(exact_from=M,
prove=True)): the header and the binding table; every argument error of the two entries, in order, without a device; the
keyword's host-side checks; the invariants of tests/prove_model.py's model (every solved node holds tests/solve_model.py's
value of its position, a solved node below its root has no priors, nothing differs from the search without the prove step
until a descent first ends on a proven node); and the floor that keeps tests/test_tree_prove_gpu.py from passing
vacuously.  No GPU."""
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
HEADER = os.path.join(ROOT, "include", "qttt_tree_prove.h")
ERR_NULL, ERR_SIZE, ERR_ACTION = -1, -2, -3

import nn_reference64 as R  # noqa: E402
import prove_model as PM  # noqa: E402
import tree_model  # noqa: E402
from qtttgym_amd import _native  # noqa: E402

NETS = {"zero": R.zero_state_dict, "greedy": R.greedy_state_dict, "counting": R.counting_state_dict,
        "sharp": R.sharp_counting_state_dict}


def _searched(case, **kw):
    net, K, M, capacity = case
    probs_of = None
    if net == "counting":              # the device's expf stands behind its softmax: here uniform stand-ins, the floor only
        probs_of = lambda leaves: np.full((leaves.n, 36), 1 / 36, dtype=np.float32)  # noqa: E731
    return PM.searched(NETS[net](), K, M, capacity, probs_of=probs_of, **kw)


# ---------------------------------------------------------------- header, binding table
def test_header_is_plain_c99_and_included_by_qttt_h_after_the_exact_leaves():
    src = open(os.path.join(ROOT, "include", "qttt.h")).read()
    assert src.index('#include "qttt_tree_exact.h"') < src.index('#include "qttt_tree_prove.h"')
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-x", "c",
                          "-I" + os.path.join(ROOT, "include"), "-"],
                         input='#include "qttt.h"\nint main(void){'
                               'int (*p)(void *, int64_t, int64_t, int, const void *, int32_t *, void *) = qttt_tree_prove;\n'
                               'int (*r)(const void *, int64_t, int64_t, float *, uint8_t *, float *, uint8_t *, void *)'
                               ' = qttt_tree_root_exact;\n'
                               'return p == 0 || r == 0 || QTTT_ABI_VERSION != 6;}\n',
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_binding_header_exports_and_build_list_agree():
    import __graft_entry__ as entry
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"^(?:int|int64_t)\s+(qttt_\w+)\s*\(", src, flags=re.M))
    assert names == set(_native.TREE_PROVE_SIGNATURES) == {"qttt_tree_prove", "qttt_tree_root_exact"}
    assert HEADER in entry.HEADERS
    assert os.path.join(ROOT, "qtttgym_amd", "csrc", "qttt_tree_prove_kernels.h") in entry.HEADERS
    L = _native.lib()
    for name in names:
        assert getattr(ctypes.CDLL(_native.LIB_PATH), name)
        assert getattr(L, name).argtypes == _native.TREE_PROVE_SIGNATURES[name][1]
    assert len(L.qttt_tree_prove.argtypes) == 7 and len(L.qttt_tree_root_exact.argtypes) == 8
    assert L.qttt_abi_version() == _native.ABI_VERSION == 6             # additive entries: the ABI number stays
    for rule in ("SKIPPED", "WALKED", "PROVABLE", "ENDS", "CLEARED", "UNTOUCHED", "keeps its priors", "sum is even",
                 "never -0.0", "leaf_exact[r] = 0", "for the first"):
        assert rule in text, rule
    for doc in ("DESIGN.md", "README.md"):
        assert "qttt_tree_prove" in open(os.path.join(ROOT, doc)).read(), doc


# ---------------------------------------------------------------- argument errors, with fake addresses never dereferenced
def _prove(L, tree=0x1000, games=1, capacity=4, leaves=2, paths=0x2000, proved=0x3000):
    return L.qttt_tree_prove(tree, games, capacity, leaves, paths, proved, None)


def _root(L, tree=0x1000, games=1, capacity=4, q=0x2000, proven=0x3000, value=0x4000, solved=0x5000):
    return L.qttt_tree_root_exact(tree, games, capacity, q, proven, value, solved, None)


def test_return_codes_in_documented_order_without_device_work():
    L = _native.lib()
    sizes = (dict(games=-1), dict(capacity=0), dict(capacity=-1), dict(capacity=(1 << 30) + 1))
    for kw in sizes + (dict(leaves=0), dict(leaves=-1), dict(leaves=65)):
        assert _prove(L, **kw) == ERR_SIZE, kw
        assert _prove(L, **{"tree": None, "paths": None, **kw}) == ERR_SIZE, kw                     # sizes before nulls
        assert _prove(L, **{"tree": 0x1001, "paths": 0x2001, "proved": 0x3001, **kw}) == ERR_SIZE, kw   # and before alignment
        assert _prove(L, **{"games": 0, **kw}) == ERR_SIZE or kw == dict(games=-1), kw              # and before games == 0
    for kw in sizes:
        assert _root(L, **kw) == ERR_SIZE, kw
        assert _root(L, **{"tree": None, **kw}) == ERR_SIZE, kw
        assert _root(L, **{"tree": 0x1001, "q": 0x2001, "value": 0x4001, **kw}) == ERR_SIZE, kw
        assert _root(L, **{"games": 0, **kw}) == ERR_SIZE or kw == dict(games=-1), kw
    assert _prove(L, games=0, tree=None, paths=None) == 0                        # nothing to do, no pointer looked at
    assert _prove(L, games=0, tree=0x1001, paths=0x2001, proved=0x3001) == 0
    assert _root(L, games=0, tree=None) == 0
    assert _root(L, games=0, tree=0x1001, q=0x2001, value=0x4001) == 0
    for kw in (dict(tree=None), dict(paths=None)):
        assert _prove(L, **kw) == ERR_NULL, kw
        assert _prove(L, **{"tree": 0x1001, "paths": 0x2008, "proved": 0x3002, **kw}) == ERR_NULL, kw   # nulls before alignment
    assert _root(L, tree=None) == ERR_NULL
    assert _root(L, tree=None, q=0x2001, value=0x4002) == ERR_NULL
    for kw in (dict(tree=0x1008), dict(tree=0x1001), dict(paths=0x2008), dict(paths=0x2004), dict(proved=0x3002),
               dict(proved=0x3001)):
        assert _prove(L, **kw) == ERR_ACTION, kw
    for kw in (dict(tree=0x1008), dict(tree=0x1001), dict(q=0x2002), dict(q=0x2001), dict(value=0x4002), dict(value=0x4001)):
        assert _root(L, **kw) == ERR_ACTION, kw
    # proved and the four outputs are nullable, proven and solved have no alignment: the next check is the launch itself,
    # which this test does not reach (no device), so only the order up to here is pinned


# ---------------------------------------------------------------- the keyword's host-side checks
def test_python_checks_prove_before_it_asks_for_a_device():
    from qtttgym_amd import SelfPlay, TreeSearch
    net = object()                    # never looked at: every call fails before
    for cls, kw in ((TreeSearch, dict(capacity=8)), (SelfPlay, dict(n_rollouts=2))):
        with pytest.raises(ValueError, match="prove=True needs exact_from"):
            cls(4, net=net, leaf_eval="value", prove=True, **kw)
        with pytest.raises(ValueError, match="prove=True needs exact_from"):
            cls(4, prove=True, **kw)
        with pytest.raises(ValueError, match="exact_from needs a net"):
            cls(4, net=net, exact_from=7, prove=True, **kw)
        for bad in (1, 0, None, "yes"):
            with pytest.raises(ValueError, match="prove must be True or False"):
                cls(4, net=net, leaf_eval="value", exact_from=7, prove=bad, **kw)
        assert inspect.signature(cls.__init__).parameters["prove"].default is False
    assert TreeSearch.prove is False
    assert [TreeSearch.check_prove(m, True) for m in (6, 7, 8, 9)] == [True] * 4         # 9 is allowed
    assert TreeSearch.check_prove(None, False) is False and TreeSearch.check_prove(7, False) is False
    assert inspect.signature(TreeSearch.choose).parameters["exact"].default is False
    assert set(TreeSearch._EXACT_ROWS) == {"proven", "q_exact", "root_solved", "root_value_exact"}
    assert not set(TreeSearch._EXACT_ROWS) & (set(TreeSearch._ROOT_ROWS) | set(TreeSearch._GUMBEL_ROWS))


# ---------------------------------------------------------------- the model
def test_without_prove_the_model_is_the_exact_leaves_model():
    import exact_leaves_model as E
    ob = E.boards_of(PM.roots(9)[0])
    for K in (1, 4):
        a = PM.ProveLeavesModel(1, seed=PM.SEED, board_offset=PM.OFFSET, net=NETS["zero"](), leaves=K, exact_from=8, prove=False)
        b = E.ExactLeavesModel(1, seed=PM.SEED, board_offset=PM.OFFSET, net=NETS["zero"](), leaves=K, exact_from=8)
        for m in (a, b):
            m.reset(ob)
            m.contemplate(PM.ROLLOUTS)
        assert [tree_model.game_view(d) for d in a.dump()] == [tree_model.game_view(d) for d in b.dump()]
        assert a.solved_flags() == b.solved_flags() and not any(st["proven"] for st in a.games)


def test_a_hand_built_position_is_proven_by_the_header_s_formula():
    """One node with three legal actions: a terminal child, a solved child and a collapse with a solved and a terminal
    child.  16 Q = -16 V(c), or minus half the sum; 16 V = the maximum."""
    m = PM.ProveLeavesModel(1, net=NETS["zero"](), leaves=1, exact_from=9)

    class N:
        def __init__(self, terminal=False, winner=-1, turn=True):
            self.terminal, self.winner, self.turn, self.legal, self.children, self.P = terminal, winner, turn, [], [None] * 36, None

    x, lost, solved, c0, c1 = N(), N(True, 1, False), N(), N(), N(True, -1)     # `lost`: the mover there (False) lost
    x.legal = [2, 5, 7]
    x.children[2], x.children[5], x.children[7] = [1], [2], [3, 4]
    st = {"nodes": [x, lost, solved, c0, c1], "solved": {2: 0.25, 3: -0.5}}
    assert PM.terminal_value(1, False) == -1.0
    assert m.sixteenths(st, 0) == (16, True)                                   # max(16, -4, -(-8 + 0) / 2 = 4)
    st["solved"] = {2: 0.25}
    assert m.sixteenths(st, 0) is None                                         # a child of the collapse is still open
    st["solved"] = {2: 0.25, 3: -0.5}
    x.legal = [5, 7]
    assert m.sixteenths(st, 0) == (4, True)
    x.legal = [5]
    assert m.sixteenths(st, 0) == (-4, False)
    x.legal = [5, 9]
    assert m.sixteenths(st, 0) is None                                         # an action that was never expanded
    x.legal, x.terminal = [5], True
    assert m.sixteenths(st, 0) is None
    x.legal, x.terminal = [], False
    assert m.sixteenths(st, 0) is None


@pytest.mark.parametrize("K", [1, 4])
def test_nothing_differs_from_the_search_without_the_prove_step_until_a_descent_ends_on_a_proven_node(K):
    """Round by round: W, N, Ntot, the child words and the priors rows (those the device keeps under a cleared flag
    included) equal the model's without the prove step up to and including the round in which a descent first ends on a
    proven interior node (that round's descents were made before anything was backed up differently); only the solved
    nodes and the has-priors flags of proven nodes differ.  After it the two searches part."""
    import exact_leaves_model as E
    ob = E.boards_of(PM.roots(PM.G_MAX)[0])
    a, b = (PM.ProveLeavesModel(1, seed=PM.SEED, board_offset=PM.OFFSET, net=NETS["zero"](), leaves=K, exact_from=8, prove=p)
            for p in (True, False))
    for m in (a, b):
        m.reset(ob)

    def view(m):
        out = []
        for st in m.games:
            for i, n in enumerate(st["nodes"]):
                row = n.probs if n.probs is not None else st["kept"].get(i)
                out.append((n.Ntot, n.N, n.W, n.children, None if row is None else row.tobytes()))
        return out

    same = parted = 0
    for k in PM.schedule(PM.ROLLOUTS, K):
        for m in (a, b):
            m.round_of(k)
        if a.met["rounds_before_first_end_on_proven"] is None or a.met["rounds"] - 1 <= a.met["rounds_before_first_end_on_proven"]:
            # the round that first ends on a proven node backs that record up with the node's exact value: W may differ there
            if a.met["ended_on_proven"] == 0:
                assert view(a) == view(b), a.met["rounds"]
                same += 1
        else:
            parted += view(a) != view(b)
    assert same >= 3 and parted > 0 and a.met["ended_on_proven"] > 0 and b.met["ended_on_proven"] == 0
    assert sum(len(st["proven"]) for st in a.games) > 0 and not any(st["proven"] for st in b.games)


# ---------------------------------------------------------------- the floor of tests/test_tree_prove_gpu.py
@pytest.mark.parametrize("case", PM.WHOLE_CASES, ids=lambda c: "%s-K%d-M%d-cap%d" % c)
def test_every_search_that_the_gpu_tests_compare_keeps_the_invariants_and_meets_its_floor(case):
    """Every search: every solved node holds the Solver's value of its position and a solved node below its root has no
    priors (check_invariants), nothing is in flight, the pool overflows iff it holds 8 nodes, some root is unproven.
    FLOOR_CASES, each: a node below the root is proven, two levels are proven in one record's walk, a node is proven
    through a collapse, a later descent ends on a proven node with fewer than exact_from moves played, some root is
    proven.  prove_model.py says why the cases with exact_from 6 and 7 cannot meet that floor; they are held to what their
    rules allow: a proven root at 6, and at 7 where the model finds any proof at all."""
    net, K, M, capacity = case
    m = _searched(case)
    assert m.check_invariants() == m.solved_counts().sum() > 0 and m.in_flight() == 0
    met = m.met
    roots = np.array([st["root"] in st["solved"] for st in m.games])
    overflowed = np.array([st["overflow"] for st in m.games])
    assert overflowed.any() == (capacity == PM.OVERFLOW_CAPACITY) and not roots.all()
    proofs = met["proved_below_root"] + met["proved_root"]
    assert proofs == sum(len(st["proven"]) for st in m.games) > 0
    if case in PM.FLOOR_CASES:
        assert met["proved_below_root"] > 0 and met["two_levels_in_one_walk"] > 0 and met["proved_through_collapse"] > 0
        assert met["ended_on_proven_early"] > 0 and roots.any()
        assert met["rederived"] > 0
    elif M == 6:
        assert met["proved_below_root"] == 0 and roots.any()
    elif M == 9:
        assert met["two_levels_stored"] > 0 and met["ended_on_proven_early"] > 0       # terminal children alone
    if capacity == PM.OVERFLOW_CAPACITY and M == 8:
        assert met["proved_below_root"] > 0 and met["ended_on_proven"] > 0             # proofs in a pool that overflows


def test_a_proven_child_that_becomes_the_root_gets_priors_and_keeps_its_children():
    stages, act, bits = _searched(("zero", 4, 8, PM.CAPACITY), stages=True)
    synced = stages["synced"]
    onto = [g for g, st in enumerate(synced.games) if st["root"] in st["proven"] and st["nodes"][st["root"]].P is None]
    assert len(onto) > 0
    for compact in (False, True):
        m = stages["second", compact]
        assert m.check_invariants() > 0
        for g in onto:
            st = m.games[g]
            root = st["nodes"][st["root"]]
            assert root.P is not None and any(c is not None for c in root.children) and st["root"] in st["solved"]
            assert st["root"] not in st["kept"]
    ex = stages["second", False].root_exact()
    assert ex["root_solved"][onto].all() and ex["proven"][onto].any(1).all()
    assert np.isnan(ex["q_exact"][~ex["proven"]]).all() and np.isnan(ex["root_value_exact"][~ex["root_solved"]]).all()


def test_root_exact_and_the_exact_choice_on_the_model():
    m = _searched(("zero", 4, 8, PM.CAPACITY))
    ex = m.root_exact()
    ordinary = np.array([tree_model.choose(st["nodes"][st["root"]]) for st in m.games], dtype=np.uint8)
    choice = m.choose_exact(ordinary)
    solver = PM.solve_model.Solver()
    n = 0
    for g, st in enumerate(m.games):
        root = st["nodes"][st["root"]]
        sol = solver.solve(root.rec)
        for a in np.flatnonzero(ex["proven"][g]):
            q = ex["q_exact"][g, a]
            assert q == np.float32(sol["q"][a]) and (q != 0 or not np.signbit(q)), (g, a)
        if ex["root_solved"][g]:
            assert ex["root_value_exact"][g] == np.float32(sol["value"]) and choice[g] == sol["best"]
            n += 1
        else:
            assert choice[g] == ordinary[g]
    assert 0 < n < len(m.games)
