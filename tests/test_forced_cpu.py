"""CPU tests of forced playouts and policy target pruning (include/qttt_tree_forced.h, TreeSearch(forced_playouts=k),
SelfPlay(prune_targets=True)): the header and the binding table; the predicate and F(c) at hand-computed points; the
properties of tests/forced_model.py's model on the searches that tests/test_forced_gpu.py runs on the device, the model
alone under its own network; the host header under the sanitizers; the keywords' host-side checks.  No GPU."""
import ctypes
import functools
import inspect
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
HEADER = os.path.join(ROOT, "include", "qttt_tree_forced.h")
ERR_NULL, ERR_SIZE, ERR_ACTION = -1, -2, -3
NAMES = {"qttt_tree_select_batch_forced", "qttt_tree_root_forced", "qttt_selfplay_record_pruned",
         "qttt_selfplay_record_stream_pruned"}

import forced_model as M  # noqa: E402
import gumbel_cases  # noqa: E402
import selfplay_model  # noqa: E402
from qtttgym_amd import _native  # noqa: E402

# the searches of the model alone: every leaves and both noise settings at G = 3, the lone wave, and the overflowing pool
# cut to its first nine games (the model is a few thousand oracle calls per game)
CPU_CASES = tuple(c for c in M.CASES if c[0] == 3) + ((1, 3, True, None), (9, 3, True, M.OVERFLOW_CAPACITY))


@functools.lru_cache(maxsize=None)
def _searched(case, forced_k=M.K_FORCED, plain=False):
    net = gumbel_cases.net_state_dict("random")
    return M.model_search(case, net, forced_k, M.PlainRoundsModel if plain else M.ForcedModel)


# ---------------------------------------------------------------- header, binding table, documents
def test_header_is_plain_c99_and_included_by_qttt_h_after_the_newest_header():
    src = open(os.path.join(ROOT, "include", "qttt.h")).read()
    assert src.index('#include "qttt_selfplay_value.h"') < src.index('#include "qttt_tree_forced.h"')
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-x", "c",
                          "-I" + os.path.join(ROOT, "include"), "-"],
                         input='#include "qttt.h"\nint main(void){'
                               'int (*f)(void *, int64_t, int64_t, uint64_t, uint32_t, int, int64_t, double, double, void *,'
                               ' void *, double, void *) = qttt_tree_select_batch_forced;\n'
                               'int (*h)(const void *, int64_t, int64_t, double, double, uint8_t *, int32_t *, void *)'
                               ' = qttt_tree_root_forced;\n'
                               'int (*r)(const void *, int64_t, int64_t, int, uint32_t, double, double, double, void *, double *,'
                               ' uint8_t *, uint8_t *, float *, uint8_t *, uint8_t *, int8_t *, uint8_t *, uint64_t, int64_t,'
                               ' double, int, double, double, void *) = qttt_selfplay_record_pruned;\n'
                               'int (*s)(const void *, int64_t, int64_t, uint32_t, double, double, double, void *, double *,'
                               ' uint8_t *, uint8_t *, float *, uint8_t *, uint8_t *, int8_t *, uint8_t *, uint64_t, int64_t,'
                               ' double, int, uint32_t, double, double, void *) = qttt_selfplay_record_stream_pruned;\n'
                               'return f == 0 || h == 0 || r == 0 || s == 0 || QTTT_ABI_VERSION != 6;}\n',
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_binding_header_exports_build_list_and_documents_agree():
    import __graft_entry__ as entry
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"^(?:int|int64_t)\s+(qttt_\w+)\s*\(", src, flags=re.M))
    assert names == set(_native.TREE_FORCED_SIGNATURES) == NAMES
    others = [getattr(_native, t) for t in dir(_native) if t.endswith("SIGNATURES") and t != "TREE_FORCED_SIGNATURES"]
    assert not any(names & set(o) for o in others)
    assert HEADER in entry.HEADERS
    for f in ("qttt_tree_forced_kernels.h", "qttt_tree_forced_host.h"):
        assert os.path.join(ROOT, "qtttgym_amd", "csrc", f) in entry.HEADERS
    L = _native.lib()
    raw = ctypes.CDLL(_native.LIB_PATH)
    for name, n_args in (("qttt_tree_select_batch_forced", 13), ("qttt_tree_root_forced", 8),
                         ("qttt_selfplay_record_pruned", 24), ("qttt_selfplay_record_stream_pruned", 24)):
        fn = getattr(L, name)
        assert getattr(raw, name)
        assert fn.argtypes == _native.TREE_FORCED_SIGNATURES[name][1] and len(fn.argtypes) == n_args, name
    sampled = _native.TREE_EXPLORE_SIGNATURES["qttt_selfplay_record_sampled"][1]
    assert _native.TREE_FORCED_SIGNATURES["qttt_selfplay_record_pruned"][1][:len(sampled) - 1] == sampled[:-1]
    assert L.qttt_abi_version() == _native.ABI_VERSION == 6             # additive entries: the ABI number stays
    for rule in ("n * n == (k P) S exactly is NOT forced", "ties to the lowest action", "Q(c) = W(c) / N(c) held fixed",
                 "N(c) - d(c) <= 1", "bisection", "sample_plies = 0 plays the plain move", "The rule stores nothing"):
        assert rule in text, rule
    for doc in ("DESIGN.md", "README.md"):
        body = open(os.path.join(ROOT, doc)).read()
        for name in ("qttt_tree_select_batch_forced", "qttt_selfplay_record_pruned", "forced_playouts", "prune_targets",
                     "qttt_tree_forced.h"):
            assert name in body, (doc, name)


# ---------------------------------------------------------------- the predicate and F(c) by hand
def test_the_predicate_and_F_at_hand_computed_points():
    # k P S = 2 * 0.5 * 16 = 16: n = 4 has n * n == k P S exactly: not forced, and F = n
    assert M.threshold(2.0, 0.5, 16) == 16.0
    assert not M.is_forced(4, 2.0, 0.5, 16) and M.F_of(2.0, 0.5, 16) == 4
    assert M.is_forced(3, 2.0, 0.5, 16) and M.is_forced(1, 2.0, 0.5, 16) and not M.is_forced(5, 2.0, 0.5, 16)
    assert not M.is_forced(0, 2.0, 0.5, 16)                              # an unvisited action is never forced
    # k P S = 2 * 0.25 * 10 = 5: 2 * 2 < 5 <= 3 * 3
    assert M.is_forced(2, 2.0, 0.25, 10) and not M.is_forced(3, 2.0, 0.25, 10) and M.F_of(2.0, 0.25, 10) == 3
    # k = 0 forces nothing and F = 0; so does a prior of 0
    assert not M.is_forced(1, 0.0, 1.0, 100) and M.F_of(0.0, 1.0, 100) == 0
    assert not M.is_forced(1, 2.0, 0.0, 100) and M.F_of(2.0, 0.0, 100) == 0
    # the largest counts: 2 * 1 * 2^23 = 4096^2
    assert not M.is_forced(4096, 2.0, 1.0, 1 << 23) and M.is_forced(4095, 2.0, 1.0, 1 << 23) and M.F_of(2.0, 1.0, 1 << 23) == 4096
    # the products are rounded one by one, in the order written: (2 * 0.1) * 5 is exactly 1.0 in doubles
    assert M.threshold(2.0, 0.1, 5) == (2.0 * 0.1) * 5.0 == 1.0 and not M.is_forced(1, 2.0, 0.1, 5) and M.F_of(2.0, 0.1, 5) == 1
    # and (2 * 0.1) * 3 is a little more than 0.6: F = 1, and one visit is not forced
    assert M.F_of(2.0, 0.1, 3) == 1 and not M.is_forced(1, 2.0, 0.1, 3)
    assert M.F_of(2.0, 0.7, 36) == 8 and M.is_forced(7, 2.0, 0.7, 36) and not M.is_forced(8, 2.0, 0.7, 36)      # 50.4
    assert M.F_of(math.inf, 1.0, 1) is None and M.F_of(math.nan, 1.0, 1) == 0
    for S in range(0, 60):
        for p in (0.0, 1 / 36, 0.2, 0.5, 1.0):
            F = M.F_of(2.0, p, S)
            assert F * F >= M.threshold(2.0, p, S) and (F == 0 or (F - 1) * (F - 1) < M.threshold(2.0, p, S))
            for n in range(0, 12):
                assert M.is_forced(n, 2.0, p, S) == (0 < n < F)           # forced: the visited actions below F


class _Node:
    terminal = False

    def __init__(self, N, W, P, Ntot=None):
        self.legal = list(range(len(N)))
        self.N, self.W = list(N) + [0] * (36 - len(N)), list(W) + [0.0] * (36 - len(N))
        self.P = None if P is None else dict(enumerate(P))
        self.Ntot = sum(N) if Ntot is None else Ntot


def test_the_prune_on_hand_built_roots():
    # c* = action 0 (20 visits, Q = 0.5).  Action 1 looked bad (Q = -1, one forced visit): it loses it.  Action 2 is as good
    # as c* (Q = 0.5, large prior): its score without any visit taken is above score(c*): it keeps all.  Action 3: unvisited.
    n = _Node([20, 1, 4, 0], [10.0, -1.0, 2.0, 0.0], [0.4, 0.1, 0.45, 0.05])
    sq = math.sqrt(25.0)
    best = 0.5 + 1.0 * (0.4 * sq / 21)
    assert M.pruned_visits(n, 2.0, 1.0)[:4] == [20, 0, 4, 0]
    assert 0.5 + 1.0 * (0.45 * sq / (1 + 3)) >= best                     # action 2 with one visit taken: not below c*
    assert M.F_of(2.0, 0.1, 25) == 3 and -1.0 + 0.1 * sq / 1 < best       # action 1 with its visit taken: below
    assert M.pruned_visits(n, 0.0, 1.0)[:4] == [20, 1, 4, 0]              # k = 0 prunes nothing
    # a bad action with many forced visits gives back min(N, F) of them, and what is left stays when it is more than one
    n = _Node([30, 6], [15.0, -6.0], [0.5, 0.5])
    assert M.F_of(2.0, 0.5, 36) == 6 and M.pruned_visits(n, 2.0, 1.0)[:2] == [30, 0]
    n = _Node([30, 9], [15.0, -9.0], [0.5, 0.5])
    assert M.F_of(2.0, 0.5, 39) == 7 and M.pruned_visits(n, 2.0, 1.0)[:2] == [30, 2]
    # the most visited action with the lowest index is c*: a tie keeps both counts when neither is below the other
    n = _Node([5, 5], [1.0, 1.0], [0.5, 0.5])
    assert M.pruned_visits(n, 2.0, 1.0)[:2] == [5, 5]
    # a root without priors prunes nothing; a root without visits neither
    assert M.pruned_visits(_Node([3, 2], [0.0, -2.0], None), 2.0, 1.0)[:2] == [3, 2]
    assert M.pruned_visits(_Node([0, 0], [0.0, 0.0], [0.5, 0.5]), 2.0, 1.0)[:2] == [0, 0]
    assert M.forced_actions(_Node([3, 2], [0.0, -2.0], None), 2.0) == []
    assert M.forced_actions(_Node([9, 1, 0], [0.0, 0.0, 0.0], [0.3, 0.6, 0.1]), 2.0) == [1]       # 1 < 12, 81 > 6, unvisited
    assert M.forced_actions(_Node([9, 1, 0], [0.0, 0.0, 0.0], [0.3, 0.6, 0.1]), 2.0, {0: 0, 1: 4, 2: 1}) == [2]  # in flight: n = 9, 5, 1


# ---------------------------------------------------------------- the model alone on the GPU tests' searches
def test_the_cases_are_the_issues():
    assert {c[0] for c in M.CASES} == {1, 3, 130} and {c[1] for c in M.CASES} == {1, 3, 8}
    assert {c[2] for c in M.CASES} == {False, True} and sum(c[3] is not None for c in M.CASES) == 1
    assert (M.K_FORCED, M.ROLLOUTS, M.NOISE, M.OVERFLOW_CAPACITY) == (2.0, 24, (0.25, 0.3), 12)
    assert all(c in M.CASES or c[0] in (1, 9) for c in CPU_CASES)


@pytest.mark.parametrize("case", CPU_CASES, ids=str)
def test_k_zero_is_the_plain_in_flight_search_visit_for_visit(case):
    zero, plain = _searched(case, 0.0), _searched(case, 0.0, True)
    assert zero.forced_taken == 0
    for stage in ("first", "games"):
        for a, b in zip(getattr(zero, stage) if stage == "first" else zero.games,
                        getattr(plain, stage) if stage == "first" else plain.games):
            assert len(a["nodes"]) == len(b["nodes"]) and a["root"] == b["root"]
            for x, y in zip(a["nodes"], b["nodes"]):
                assert x.N == y.N and x.W == y.W and x.Ntot == y.Ntot and x.children == y.children
    for root in zero.roots():                                             # and the plain pi row bit for bit
        if root.legal and not root.terminal:
            got = M.pruned_pi_row(root, 0.0, zero.c_puct, M.ROLLOUTS)
            want = selfplay_model.pi_row(root.N, root.legal, M.ROLLOUTS)
            assert np.array_equal(got.view(np.int64), want.view(np.int64))


@pytest.mark.parametrize("case", CPU_CASES, ids=str)
def test_the_pruned_row_keeps_the_best_action_and_invents_nothing(case):
    m = _searched(case)
    pruned_something = forced_something = 0
    for stage in (m.first, m.games):
        for st in stage:
            root = st["nodes"][st["root"]]
            if root.terminal or not root.legal or root.P is None:
                continue
            N1 = M.pruned_visits(root, M.K_FORCED, m.c_puct)
            star = max(root.legal, key=lambda a: root.N[a])
            assert N1[star] == root.N[star]                               # c* keeps its visits
            assert all(N1[a] <= root.N[a] for a in range(36))
            assert all(N1[a] == 0 for a in range(36) if root.N[a] == 0)   # the support lies inside the plain row's
            assert sum(N1) >= root.N[star] > 0
            assert all(N1[a] != 1 for a in range(36) if N1[a] != root.N[a])      # no single visit left by a subtraction
            plain, pruned = selfplay_model.pi_row(root.N, root.legal, M.ROLLOUTS), M.pruned_pi_row(root, M.K_FORCED, m.c_puct, M.ROLLOUTS)
            assert not (pruned[plain == 0.0] != 0.0).any() and abs(pruned.sum() - 1.0) < 1e-12
            pruned_something += N1 != list(root.N)
            forced_something += bool(M.forced_actions(root, M.K_FORCED))
    assert m.forced_taken > 0                                             # the rule did decide descents
    assert case[0] < 3 or not case[2] or pruned_something > 0              # under noise the prune took visits away


def test_forcing_spreads_the_visits_of_a_noised_root():
    """What the rule is for: under the same noise more root actions get a second look than under the plain search."""
    case = (3, 3, True, None)
    forced, plain = _searched(case), _searched(case, 0.0, True)
    twice = lambda m: sum(sum(1 for a in st["nodes"][st["root"]].legal if st["nodes"][st["root"]].N[a] >= 2) for st in m.first)  # noqa: E731
    assert twice(forced) >= twice(plain)


# ---------------------------------------------------------------- the host header under the sanitizers
def test_the_host_header_under_the_sanitizers(tmp_path):
    """tools/forced_host_check.cpp: the argument checks and one action's arithmetic — the code the kernels' lanes run — as a
    stand-alone program with ASan and UBSan.  CPU only."""
    exe = tmp_path / "forced_host_check"
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "qtttgym_amd", "csrc"), os.path.join(ROOT, "tools", "forced_host_check.cpp"),
                           "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "forced_host_check: ok" in out.stdout, out.stdout + out.stderr


# ---------------------------------------------------------------- argument errors of the C entries, without a device
def test_return_codes_in_documented_order_without_device_work():
    """Fake addresses, never dereferenced: every call fails its checks first (or has no games)."""
    L = _native.lib()
    nan, inf = float("nan"), float("inf")

    def select(tree=0x1000, games=1, capacity=4, idx0=0, leaves=2, offset=0, vloss=1.0, paths=0x2000, leaf=0x3000, k=2.0):
        return L.qttt_tree_select_batch_forced(tree, games, capacity, 0, idx0, leaves, offset, 1.0, vloss, paths, leaf, k, None)

    def root(tree=0x1000, games=1, capacity=4, k=2.0, c=1.0, forced=0x2000, pruned=0x3000):
        return L.qttt_tree_root_forced(tree, games, capacity, k, c, forced, pruned, None)

    def record(stream=False, tree=0x1000, games=1, ply=0, n=8, alpha=1.0, temp=1.0, plies=2, draw=0, k=2.0, c=1.0, **ptr):
        p = {f: 0x10000 * (i + 2) for i, f in enumerate(selfplay_fields)}
        p.update(ptr)
        head = (tree, games, 4) + (() if stream else (ply,)) + (n, alpha, 1.0, -1.0) + tuple(p[f] for f in selfplay_fields)
        tail = (0, 0, temp, plies) + ((draw,) if stream else ()) + (k, c, None)
        return (L.qttt_selfplay_record_stream_pruned if stream else L.qttt_selfplay_record_pruned)(*head, *tail)

    selfplay_fields = ("states", "pi", "mask", "done", "v", "action36", "length", "winner", "actions")
    sizes = (dict(games=-1), dict(capacity=0), dict(capacity=_native.TREE_MAX_CAPACITY + 1))
    for kw in sizes + (dict(offset=-1), dict(leaves=0), dict(leaves=65), dict(idx0=(1 << 24) - 1), dict(vloss=-1.0),
                       dict(vloss=nan), dict(k=-0.5), dict(k=nan), dict(k=inf)):
        assert select(**kw) == ERR_SIZE, kw
        assert select(**{"tree": None, "paths": None, "leaf": None, **kw}) == ERR_SIZE, kw          # sizes before nulls
        assert select(**{"tree": 0x1008, "paths": 0x2008, **kw}) == ERR_SIZE, kw                    # and before alignment
    assert select(games=0, tree=None, paths=None, leaf=None) == 0
    for kw in (dict(tree=None), dict(paths=None), dict(leaf=None)):
        assert select(**kw) == ERR_NULL, kw
        assert select(**{"tree": 0x1008, "paths": 0x2008, **kw}) == ERR_NULL, kw                    # nulls before alignment
    for kw in (dict(tree=0x1008), dict(paths=0x2008)):
        assert select(**kw) == ERR_ACTION, kw
    for kw in sizes + (dict(k=-1.0), dict(k=nan), dict(k=inf), dict(c=nan), dict(c=inf)):
        assert root(**kw) == ERR_SIZE and root(**{"tree": None, **kw}) == ERR_SIZE, kw
    assert root(games=0, tree=None) == 0 and root(tree=None) == ERR_NULL
    assert root(tree=0x1008) == ERR_ACTION and root(pruned=0x3002) == ERR_ACTION
    for stream in (False, True):
        bad = (dict(games=-1), dict(n=0), dict(alpha=0.0), dict(alpha=nan), dict(temp=0.0), dict(temp=inf), dict(plies=-1),
               dict(plies=11), dict(k=-1.0), dict(k=nan), dict(k=inf), dict(c=nan), dict(c=-inf))
        bad += (dict(draw=_native.SELFPLAY_MAX_MOVE_DRAWS),) if stream else (dict(ply=-1), dict(ply=10))
        for kw in bad:
            assert record(stream, **kw) == ERR_SIZE, (stream, kw)
            assert record(stream, **{"tree": None, "pi": None, **kw}) == ERR_SIZE, (stream, kw)
        assert record(stream, games=0, tree=None, pi=None) == 0
        assert record(stream, plies=0, tree=None) == ERR_NULL               # sample_plies = 0 passes the size check
        for f in ("tree",) + selfplay_fields:
            assert record(stream, **{f: None}) == ERR_NULL, (stream, f)
        assert record(stream, tree=0x1008) == record(stream, states=0x20008) == ERR_ACTION
        assert record(stream, pi=0x30004) == record(stream, v=0x60002) == ERR_ACTION


# ---------------------------------------------------------------- the keywords' host-side checks
def test_python_checks_the_keywords_before_it_asks_for_a_device():
    from qtttgym_amd import SelfPlay, TreeSearch
    net = object()                                                       # never looked at before the keywords are checked
    assert inspect.signature(TreeSearch.__init__).parameters["forced_playouts"].default is None
    sig = inspect.signature(SelfPlay.__init__).parameters
    assert sig["forced_playouts"].default is None and sig["prune_targets"].default is None
    assert TreeSearch.forced_playouts is None
    for bad in (-0.5, float("nan"), float("inf"), "2", True, (2.0,)):
        with pytest.raises(ValueError, match="forced_playouts must be None or a finite number >= 0"):
            TreeSearch(4, 64, net=net, leaf_eval="value", forced_playouts=bad)
        with pytest.raises(ValueError, match="forced_playouts must be None or a finite number >= 0"):
            SelfPlay(4, net=net, leaf_eval="value", forced_playouts=bad)
    for kw in (dict(), dict(net=net), dict(leaf_eval="value")):
        with pytest.raises(ValueError, match='forced_playouts needs a net and leaf_eval="value"'):
            TreeSearch(4, 64, forced_playouts=2.0, **kw)
    with pytest.raises(ValueError, match='forced_playouts needs a net and leaf_eval="value"'):
        SelfPlay(4, net=net, forced_playouts=2.0)
    for cls, args in ((TreeSearch, (4, 64)), (SelfPlay, (4,))):
        with pytest.raises(ValueError, match='forced_playouts is a rule of the PUCT root'):
            cls(*args, net=net, leaf_eval="value", root_policy="gumbel", forced_playouts=2.0)
    with pytest.raises(ValueError, match="prune_targets=True needs forced_playouts"):
        SelfPlay(4, prune_targets=True)
    with pytest.raises(ValueError, match="prune_targets=True needs forced_playouts"):
        SelfPlay(4, net=net, leaf_eval="value", prune_targets=True)
    with pytest.raises(ValueError, match="prune_targets must be True or False"):
        SelfPlay(4, net=net, leaf_eval="value", forced_playouts=2.0, prune_targets=1)
    assert TreeSearch.check_forced_playouts("playouts", None, "puct", None) is None
    assert TreeSearch.check_forced_playouts("value", net, "puct", 2) == 2.0
    assert TreeSearch.check_forced_playouts("value", net, "puct", 0) == 0.0
    assert SelfPlay.check_prune_targets(None, None) is False and SelfPlay.check_prune_targets(None, False) is False
    assert SelfPlay.check_prune_targets(2.0, None) is True and SelfPlay.check_prune_targets(2.0, False) is False
    assert SelfPlay.check_prune_targets(0.0, True) is True
    assert "forced_playouts" in sys.modules[TreeSearch.__module__].__doc__ and "forced_playouts" in TreeSearch.__init__.__doc__
    assert "prune_targets" in SelfPlay.__doc__
    for example, flags in (("selfplay_train.py", ("--forced-playouts", "--no-prune-targets")), ("tree_tournament.py", ("--forced-playouts",))):
        body = open(os.path.join(ROOT, "examples", example)).read()
        for flag in flags:
            assert flag in body, (example, flag)
