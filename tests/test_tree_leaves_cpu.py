"""CPU tests of the leaf-parallel rounds (include/qttt_tree_leaves.h, TreeSearch(leaf_eval="value", leaves=K)):
tests/leaf_parallel_model.py's LeafParallelModel checked by hand on small trees; the model at K = 1 against ValueTreeModel
on whole trees; the coverage floor: the roots and round counts that tests/test_tree_leaves_gpu.py searches drive the model
through everything a round can meet; the header and the binding table; and the keyword checks that need no device.
No GPU."""
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
HEADER = os.path.join(ROOT, "include", "qttt_tree_leaves.h")

import leaf_parallel_model as LP  # noqa: E402
import oracle  # noqa: E402
import tree_model  # noqa: E402
import value_tree_model as V  # noqa: E402
from nn_reference64 import sharp_counting_state_dict, zero_state_dict  # noqa: E402
from qtttgym_amd import _native  # noqa: E402


# ---------------------------------------------------------------- header, binding table
def test_header_is_plain_c99_and_included_by_qttt_h_after_the_value_rollout():
    src = open(os.path.join(ROOT, "include", "qttt.h")).read()
    assert src.index('#include "qttt_tree_value.h"') < src.index('#include "qttt_tree_leaves.h"')
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-x", "c",
                          "-I" + os.path.join(ROOT, "include"), "-"],
                         input='#include "qttt.h"\nint main(void){'
                               'int (*s)(void *, int64_t, int64_t, uint64_t, uint32_t, int, int64_t, double, double, void *,'
                               ' void *, void *) = qttt_tree_select_batch;\n'
                               'int (*b)(void *, int64_t, int64_t, int, const void *, const float *, const float *, void *)'
                               ' = qttt_tree_backup_batch;\nint64_t (*p)(int64_t, int) = qttt_tree_paths_bytes;\n'
                               'return s == 0 || b == 0 || p == 0 || QTTT_ABI_VERSION != 6 || QTTT_TREE_MAX_LEAVES != 64'
                               ' || QTTT_TREE_PATH_BYTES != 64;}\n',
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_binding_header_exports_and_build_list_agree():
    import __graft_entry__ as entry
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"^(?:int|int64_t)\s+(qttt_\w+)\s*\(", src, flags=re.M))
    assert names == set(_native.TREE_LEAVES_SIGNATURES) == {"qttt_tree_paths_bytes", "qttt_tree_select_batch",
                                                            "qttt_tree_backup_batch"}
    assert HEADER in entry.HEADERS
    L = _native.lib()
    for name in names:
        assert getattr(ctypes.CDLL(_native.LIB_PATH), name)
        assert getattr(L, name).argtypes == _native.TREE_LEAVES_SIGNATURES[name][1]
    assert L.qttt_abi_version() == _native.ABI_VERSION == 6             # additive entries: the ABI number stays
    assert _native.TREE_MAX_LEAVES == LP.MAX_LEAVES == 64 and _native.TREE_PATH_BYTES == LP.PATH_DTYPE.itemsize == 64
    for rule in ("The in-flight invariant", "NO OTHER TREE ENTRY", "The select rule", "The backup rule"):
        assert rule in text, rule
    for doc in ("DESIGN.md", "README.md"):
        assert "qttt_tree_select_batch" in open(os.path.join(ROOT, doc)).read(), doc


# ---------------------------------------------------------------- the keyword's host-side checks
def test_python_checks_leaves_and_virtual_loss_before_it_asks_for_a_device():
    from qtttgym_amd import SelfPlay, TreeSearch
    net = object()                    # never looked at: every call fails before
    for cls, kw in ((TreeSearch, dict(capacity=8)), (SelfPlay, dict(n_rollouts=2))):
        for leaves in (0, -1, 65):
            with pytest.raises(ValueError, match="leaves"):
                cls(4, net=net, leaf_eval="value", leaves=leaves, **kw)
        with pytest.raises(ValueError, match="leaf_eval"):
            cls(4, net=net, leaves=2, **kw)
        with pytest.raises(ValueError, match="leaf_eval"):
            cls(4, leaves=2, **kw)
        for vl in (-0.5, float("inf"), float("nan")):
            with pytest.raises(ValueError, match="virtual_loss"):
                cls(4, net=net, leaf_eval="value", leaves=2, virtual_loss=vl, **kw)
    import inspect
    for cls in (TreeSearch, SelfPlay):
        p = inspect.signature(cls.__init__).parameters
        assert p["leaves"].default == 1 and p["virtual_loss"].default == 1.0


# ---------------------------------------------------------------- the model, by hand
def _model(net, K, c_puct=1.0, vloss=1.0, capacity=None):
    m = LP.LeafParallelModel(1, seed=3, board_offset=0, c_puct=c_puct, net=net, capacity=capacity, leaves=K, virtual_loss=vloss)
    m.reset(oracle.OracleBoards(1))
    m.contemplate(1)                  # the single rollout: the root gets its priors
    return m


@pytest.mark.parametrize("vloss, diverted", [(1.0, True), (0.25, True), (0.0, False)])
def test_virtual_loss_alone_diverts_the_second_descent(vloss, diverted):
    """c_puct = 0 under the zero network: every score is q = 0, so descent 0 takes the lowest action; for descent 1 that
    action has q = -virtual_loss / 1, and nothing else tells the actions apart."""
    m = _model(zero_state_dict(), 2, c_puct=0.0, vloss=vloss)
    m.select_batch(2, vloss)
    (r0, r1), = m.round
    root = m.games[0]["nodes"][0]
    assert r0["path"] == [(0, root.legal[0])]
    assert r1["path"] == [(0, root.legal[1] if diverted else root.legal[0])]
    assert (r0["leaf"] != r1["leaf"]) == diverted and m.met["diverted"] == int(diverted)
    words = m.raw_words()[0][0]
    assert words[1] == 2 << 24 and sorted(w for w in words[0] if w) == ([1 << 24, 1 << 24] if diverted else [2 << 24])
    assert root.W == [0.0] * 36 and root.N == [0] * 36             # W and the counts proper are not perturbed


def _dominant_prior_round(vloss):
    """The zero network's tree after two rollouts, then by decree a root prior of 0.9 on one unvisited action."""
    m = _model(zero_state_dict(), 2, vloss=vloss)
    m.round_of(1)
    root = m.games[0]["nodes"][0]
    star = root.legal[7]
    assert root.Ntot == 1 and root.N[star] == 0
    root.P = {a: 0.9 if a == star else 0.1 / (len(root.legal) - 1) for a in root.legal}
    m.select_batch(2, vloss)
    return m, root, star


def test_without_virtual_loss_a_dominant_prior_is_not_diverted_and_both_descents_back_up():
    m, root, star = _dominant_prior_round(0.0)
    (r0, r1), = m.round
    assert r0["path"] == r1["path"] == [(0, star)] and r0["leaf"] == r1["leaf"] and m.met["same_open_leaf"] == 1
    # by hand: descent 1 sees Ne = 1, Ntot_e = 2 on the starred action
    assert m._score_in_flight(root, star, 1, 1, 0.0) == 0.9 * 2 ** 0.5 / 2 > 0.1 / 35 * 2 ** 0.5
    leaf = m.games[0]["nodes"][r0["leaf"]]
    assert leaf.P is None and m.in_flight() == 4 and m.raw_words()[0][0][0][star] == 2 << 24
    rows = np.zeros((2, 36), dtype=np.float32)
    rows[0, leaf.legal], rows[1, leaf.legal] = 0.25, 0.75
    m.backup_batch(np.array([0.5, 0.125], dtype=np.float32), rows)
    assert root.W[star] == -0.5 - 0.125 and root.N[star] == 2 and root.Ntot == 3
    assert leaf.probs.tobytes() == rows[0].tobytes()                 # the second descent keeps the first's priors
    assert m.in_flight() == 0 and m.round is None and m.k == 4
    assert all(w < 1 << 24 for n in m.raw_words()[0] for w in n[0] + [n[1]])


def test_enough_virtual_loss_diverts_even_a_dominant_prior():
    m, root, star = _dominant_prior_round(8.0)
    (r0, r1), = m.round
    assert r0["path"] == [(0, star)] and r1["path"][0][1] != star and m.met["diverted"] == 1
    # by hand: q = -8 / 1 on the starred action, against an exploration term below 1 everywhere
    assert m._score_in_flight(root, star, 1, 1, 8.0) == -8.0 + 0.9 * 2 ** 0.5 / 2


def test_in_flight_counts_are_zero_after_every_backup_and_a_round_is_k_rollouts():
    net = sharp_counting_state_dict()
    m = LP.LeafParallelModel(1, seed=5, board_offset=17, net=net, leaves=5)
    arrays = LP.root_pool(12)
    m.reset(oracle.boards_from_arrays(arrays["board"], arrays["moves"], arrays["n_moves"], arrays["qmask"], arrays["n_q"]))
    m.contemplate(1 + 5 + 3)
    assert m.k == 9 and m.in_flight() == 0 and not m.fresh
    leaves = m.select_batch(5, 1.0)
    assert leaves.n == 12 * 5
    recs = m.records()
    assert recs.shape == (12, 5) and m.in_flight() == 2 * int(recs["depth"].sum()) > 0
    for g, st in enumerate(m.games):
        assert st["path"] == [] and st["leaf"] == st["root"]         # as a compaction leaves them
        root = st["nodes"][st["root"]]
        if not root.terminal and root.legal:
            assert m.raw_words()[g][st["root"]][1] >> 24 == 5        # every descent passes the root
    m.backup_batch(m.playouts(leaves), m.priors(leaves))
    assert m.k == 14 and m.in_flight() == 0
    open_roots = [st["nodes"][st["root"]] for st in m.games if not st["nodes"][st["root"]].terminal]
    assert open_roots and all(r.Ntot == 13 for r in open_roots)


# ---------------------------------------------------------------- K = 1 is the value rollout
@pytest.mark.parametrize("capacity", [None, V.OVERFLOW_CAPACITY])
def test_rounds_of_one_are_the_value_rollout_on_whole_trees(capacity):
    net = sharp_counting_state_dict()
    arrays = LP.root_pool(65)
    ob = oracle.boards_from_arrays(arrays["board"], arrays["moves"], arrays["n_moves"], arrays["qmask"], arrays["n_q"])
    a = V.ValueTreeModel(1, seed=5, board_offset=17, net=net, capacity=capacity)
    b = LP.LeafParallelModel(1, seed=5, board_offset=17, net=net, capacity=capacity, leaves=1)
    a.reset(ob)
    b.reset(ob)
    for k in range(24):
        a.rollout()
        b.round_of(1)                 # from the very first rollout on: a root without priors is its own leaf
        if k in (0, 1, 11, 23):
            for da, db in zip(a.dump(), b.dump()):
                va, vb = tree_model.game_view(da), tree_model.game_view(db)
                assert (va[0], va[1], va[4]) == (vb[0], vb[1], vb[4]) and da["overflow"] == db["overflow"]
    assert a.k == b.k == 24 and b.ends == a.ends and b.met["diverted"] == 0


# ---------------------------------------------------------------- the coverage floor
def test_the_searches_of_the_gpu_tests_meet_everything_a_round_can_meet():
    """Over the roots (the 65-game pool), the leaf counts and the schedule that tests/test_tree_leaves_gpu.py runs, in
    its ample pool and in its 12-node pool, the model meets each of: two descents of a round sharing an edge below the
    root; two ending on the same open leaf; a terminal leaf inside a round; a collapse pair expanded inside a round whose
    sibling a later descent of the round enters; and, in the small pool, descents after an overflowed one."""
    ample, small = {}, {}
    for net in (sharp_counting_state_dict,):
        for K in (2, 5, 8):
            for capacity, total in ((None, ample), (V.OVERFLOW_CAPACITY, small)):
                stages, _, _ = LP.model_stages(net(), K, capacity, 65)
                for key in (("second", False), ("second", True)):
                    m = stages[key]
                    assert m.in_flight() == 0 and m.k == LP.first_rollouts(K) + LP.second_rollouts(K)
                    for what, n in m.met.items():
                        total[what] = total.get(what, 0) + n
    for what in ("shared_edge_below_root", "same_open_leaf", "terminal_in_round", "sibling_entered", "diverted"):
        assert ample[what] > 0, (what, ample)
    assert ample["descents_after_overflow"] == 0 and small["descents_after_overflow"] > 0, (ample, small)
