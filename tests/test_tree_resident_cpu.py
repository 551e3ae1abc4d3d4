"""CPU tests of the resident search (include/qttt_tree_resident.h, TreeSearch(resident=), SelfPlay(resident=)): the header,
the exported symbols and the binding table; every argument error of the entry, in order, without a device; the tile and the
round plan by hand; the constructors' refusals; the stand-alone host program.  No GPU."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
INCLUDE = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "qtttgym_amd", "csrc")
ERR_NULL, ERR_SIZE, ERR_ACTION = -1, -2, -3
NAMES = {"qttt_tree_search_resident", "qttt_tree_resident_games_per_group", "qttt_tree_resident_plan"}

from qtttgym_amd import _native  # noqa: E402


# ---------------------------------------------------------------- header, binding table, documents
def test_the_header_is_plain_c99_and_ends_qttt_hs_include_chain():
    src = open(os.path.join(INCLUDE, "qttt.h")).read()
    assert src.index('#include "qttt_selfplay_cap.h"') < src.index('#include "qttt_tree_resident.h"')
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-x", "c", "-I" + INCLUDE, "-"],
                         input='#include "qttt.h"\nint main(void){'
                               'int (*s)(void *, int64_t, int64_t, uint64_t, uint32_t, int, uint32_t, int64_t, double, double,'
                               ' double, const void *, int, void *) = qttt_tree_search_resident;\n'
                               'int (*t)(int, int) = qttt_tree_resident_games_per_group;\n'
                               'int (*p)(int, uint32_t, int32_t *, int) = qttt_tree_resident_plan;\n'
                               'return s == 0 || t == 0 || p == 0 || QTTT_ABI_VERSION != 6;}\n',
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_binding_header_exports_build_list_and_documents_agree():
    import __graft_entry__ as entry
    path = os.path.join(INCLUDE, "qttt_tree_resident.h")
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    names = set(re.findall(r"^(?:int|int64_t)\s+(qttt_\w+)\s*\(", src, flags=re.M))
    assert names == set(_native.TREE_RESIDENT_SIGNATURES) == NAMES
    others = [getattr(_native, t) for t in dir(_native) if t.endswith("SIGNATURES") and t != "TREE_RESIDENT_SIGNATURES"]
    assert not any(names & set(o) for o in others)
    assert path in entry.HEADERS
    for f in ("qttt_tree_resident_kernels.h", "qttt_tree_resident_host.h"):
        assert os.path.join(CSRC, f) in entry.HEADERS
    L = _native.lib()
    raw = ctypes.CDLL(_native.LIB_PATH)
    for name, n_args in (("qttt_tree_search_resident", 14), ("qttt_tree_resident_games_per_group", 2),
                         ("qttt_tree_resident_plan", 4)):
        assert getattr(raw, name)
        sig = _native.TREE_RESIDENT_SIGNATURES[name][1]
        assert getattr(L, name).argtypes == sig and len(sig) == n_args, name
    # the argument order of the subset select up to forced_k, with `rollouts` after `leaves`
    subset = _native.TREE_SUBSET_SIGNATURES["qttt_tree_select_batch_subset"][1]
    mine = _native.TREE_RESIDENT_SIGNATURES["qttt_tree_search_resident"][1]
    assert mine[:6] == subset[:6] and mine[7:11] == subset[6:10]
    assert L.qttt_abi_version() == _native.ABI_VERSION == 6             # additive entries: the ABI number stays
    text = open(path).read()
    for rule in ("ROUNDS OF K WHILE K ROLLOUTS REMAIN, THEN ONE ROUND OF THE", "forced_k < 0 is the", "no workspace argument",
                 "64 / K", "128 / K", "rollout_idx0 + rollouts > QTTT_TREE_MAX_ROLLOUTS"):
        assert rule in text, rule
    for doc in ("DESIGN.md", "README.md"):
        body = open(os.path.join(ROOT, doc)).read()
        for name in ("qttt_tree_search_resident", "qttt_tree_resident.h", "resident=True", "rounds_per_launch"):
            assert name in body, (doc, name)
    # the kernel's source names no body of its own: the three parts are the existing launches' device functions
    kernel = open(os.path.join(CSRC, "qttt_tree_resident_kernels.h")).read()
    for fn in ("tree_select_batch_game(", "tree_backup_batch_game<false>(", "nn_encode_row<PREC>(", "nn_hidden<PREC>(",
               "nn_head<PREC>(", "nn_softmax_stats(", "nn_prob("):
        assert fn in kernel, fn
    assert "atomic" not in re.sub(r"//.*", "", kernel) and "return;" not in re.sub(r"//.*", "", kernel)


# ---------------------------------------------------------------- argument errors of the C entry, without a device
def test_return_codes_in_documented_order_without_device_work():
    """Fake addresses, never dereferenced: every call fails its checks first (or has nothing to do)."""
    L = _native.lib()
    nan, inf = float("nan"), float("inf")

    def search(tree=0x1000, games=2, capacity=4, idx0=0, leaves=2, rollouts=3, offset=0, vloss=1.0, k=-1.0, weights=0x2000,
               precision=_native.NN_F32):
        return L.qttt_tree_search_resident(tree, games, capacity, 0, idx0, leaves, rollouts, offset, 1.0, vloss, k, weights,
                                           precision, None)

    for kw in (dict(games=-1), dict(capacity=0), dict(capacity=_native.TREE_MAX_CAPACITY + 1), dict(offset=-1), dict(leaves=0),
               dict(leaves=65), dict(idx0=(1 << 24) - 2), dict(idx0=1, rollouts=(1 << 24)), dict(vloss=-1.0), dict(vloss=nan),
               dict(vloss=inf), dict(k=nan), dict(k=inf), dict(k=-inf), dict(precision=2), dict(precision=-1)):
        assert search(**kw) == ERR_SIZE, kw
        assert search(**{"tree": None, "weights": None, **kw}) == ERR_SIZE, kw                # sizes before nulls
        assert search(**{"tree": 0x1008, "weights": 0x2004, **kw}) == ERR_SIZE, kw            # and before alignment
    assert search(idx0=(1 << 24) - 3, tree=None) == ERR_NULL             # idx0 + rollouts == the bound: allowed
    for k in (-1.0, -0.5, 0.0, 2.0):                                     # any finite k: negative is the plain root
        assert search(k=k, tree=None) == ERR_NULL
    for p in (_native.NN_F32, _native.NN_BF16):
        assert search(precision=p, weights=None) == ERR_NULL
    # nothing to do: no device work, whatever the pointers
    assert search(games=0, tree=None, weights=None) == 0 and search(rollouts=0, tree=None, weights=None) == 0
    assert search(rollouts=0, tree=0x1008, weights=0x2004) == 0
    for kw in (dict(tree=None), dict(weights=None)):
        assert search(**kw) == ERR_NULL, kw
        assert search(**{"tree": 0x1008, "weights": 0x2004, **kw}) == ERR_NULL, kw            # nulls before alignment
    for kw in (dict(tree=0x1008), dict(weights=0x2008), dict(weights=0x2004)):
        assert search(**kw) == ERR_ACTION, kw


# ---------------------------------------------------------------- the tile and the plan
def test_games_per_group_is_the_network_tile_over_the_leaves():
    T = _native.lib().qttt_tree_resident_games_per_group
    want = {1: (64, 128), 3: (21, 42), 8: (8, 16), 64: (1, 2)}
    for K, (f32, bf16) in want.items():
        assert T(K, _native.NN_F32) == f32 and T(K, _native.NN_BF16) == bf16, K
    for K in range(1, 65):
        assert T(K, _native.NN_F32) == 64 // K >= 1 and T(K, _native.NN_BF16) == 128 // K
    for K, p in ((0, 0), (65, 0), (-1, 1), (8, 2), (8, -1)):
        assert T(K, p) == ERR_SIZE, (K, p)


def _plan(K, R, cap=64):
    out = (ctypes.c_int32 * max(cap, 1))(*([-7] * max(cap, 1)))
    n = _native.lib().qttt_tree_resident_plan(K, R, ctypes.cast(out, ctypes.c_void_p) if cap else None, cap)
    return n, list(out)[:min(max(n, 0), cap)], list(out)


def test_the_plan_by_hand():
    assert _plan(8, 31) == (4, [8, 8, 8, 7], [8, 8, 8, 7] + [-7] * 60)
    assert _plan(8, 32)[:2] == (4, [8, 8, 8, 8]) and _plan(8, 33)[:2] == (5, [8, 8, 8, 8, 1])
    assert _plan(8, 5)[:2] == (1, [5]) and _plan(64, 63)[:2] == (1, [63])          # rollouts < K: one short round
    assert _plan(1, 3)[:2] == (3, [1, 1, 1]) and _plan(3, 0)[:2] == (0, [])
    # cap: the count is the whole launch's, the array gets the first cap sizes, and none at all without one
    assert _plan(8, 31, cap=2) == (4, [8, 8], [8, 8])
    assert _plan(8, 31, cap=0)[0] == 4
    P = _native.lib().qttt_tree_resident_plan
    assert P(0, 5, None, 0) == P(65, 5, None, 0) == P(8, (1 << 24) + 1, None, 0) == P(8, 5, None, -1) == ERR_SIZE
    assert P(8, 5, None, 1) == ERR_NULL and P(0, 5, None, 1) == ERR_SIZE           # sizes before nulls
    assert P(8, 1 << 24, None, 0) == 1 << 21


def test_the_plans_sum_is_the_rollouts_for_every_k_and_budget():
    for K in range(1, 65):
        for R in range(0, 201):
            n, rounds, _ = _plan(K, R, cap=200)
            assert n == -(-R // K) == len(rounds) and sum(rounds) == R, (K, R)
            assert all(r == K for r in rounds[:-1]) and (not rounds or 1 <= rounds[-1] <= K), (K, R)


# ---------------------------------------------------------------- the keywords' host-side checks
def test_python_refuses_what_the_fused_launch_cannot_run_before_it_asks_for_a_device():
    from qtttgym_amd import SelfPlay, TreeSearch
    net = object()                                                       # never looked at before the keywords are checked
    for cls in (TreeSearch, SelfPlay):
        sig = inspect.signature(cls.__init__).parameters
        assert sig["resident"].default is False and sig["rounds_per_launch"].default == 64
    ok = dict(net=net, leaf_eval="value", resident=True)
    for make in (lambda **kw: TreeSearch(4, capacity=64, **kw), lambda **kw: SelfPlay(4, n_rollouts=12, **kw)):
        with pytest.raises(ValueError, match='resident=True with leaf_eval="playouts"'):
            make(resident=True)
        with pytest.raises(ValueError, match='resident=True with leaf_eval="playouts"'):
            make(resident=True, net=net)
        with pytest.raises(ValueError, match='resident=True with root_policy="gumbel"'):
            make(root_policy="gumbel", **ok)
        with pytest.raises(ValueError, match="resident=True with exact_from"):
            make(exact_from=7, **ok)
        with pytest.raises(ValueError, match="resident=True with exact_from"):
            make(exact_from=7, prove=True, **ok)
        with pytest.raises(ValueError, match="resident=True with eval_symmetries"):
            make(eval_symmetries="all", **ok)
        for bad in (0, -1, 2.0, True, "4", None):
            with pytest.raises(ValueError, match="rounds_per_launch must be an integer >= 1"):
                make(rounds_per_launch=bad, **ok)
        for bad in (1, "yes", None):
            with pytest.raises(ValueError, match="resident must be True or False"):
                make(net=net, leaf_eval="value", resident=bad)
    with pytest.raises(ValueError, match="resident=True with playout_cap"):
        SelfPlay(4, n_rollouts=12, playout_cap=(0.5, 4), **ok)
    check = TreeSearch.check_resident
    assert check(True, 3, "value", net, "puct", None, False, None) == (True, 3)
    assert check(False, 64, "playouts", None, "gumbel", 7, True, (0,)) == (False, 64)       # off: nothing is looked at
    with pytest.raises(ValueError, match="resident=True with prove"):
        check(True, 64, "value", net, "puct", None, True, None)
    # contemplate(games=...) is refused by the pair's name (a tree is needed for nothing else here)
    t = TreeSearch.__new__(TreeSearch)
    t.resident, t._bound, t.rollout_idx, t.leaf_eval, t.capacity = True, 1, 0, "value", 64
    with pytest.raises(ValueError, match=r"resident=True with contemplate\(games=\.\.\.\)"):
        t.contemplate(2, games=[True])
    assert "resident" in SelfPlay.__doc__ and "resident" in TreeSearch.contemplate.__doc__
    assert "resident=True" in sys.modules[TreeSearch.__module__].__doc__
    for example in ("selfplay_train.py", "tree_tournament.py"):
        assert "--resident" in open(os.path.join(ROOT, "examples", example)).read()
    sp = SelfPlay.__new__(SelfPlay)
    for k in ("num_simulations", "c_puct", "net", "leaf_eval", "leaves", "virtual_loss", "eval_symmetries", "root_policy",
              "max_considered", "c_visit", "c_scale", "exact_from", "prove", "forced_playouts"):
        setattr(sp, k, None)
    sp.resident, sp.rounds_per_launch = True, 5
    kw = sp.search_kwargs()
    assert kw["resident"] is True and kw["rounds_per_launch"] == 5       # what a Reanalyser's recorder and trees are built with


# ---------------------------------------------------------------- the host program
def test_the_host_program_builds_and_runs_clean_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "resident_host_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-I" + INCLUDE, "-I" + CSRC, os.path.join(ROOT, "tools", "resident_host_check.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "resident_host_check: ok" in run.stdout, run.stdout + run.stderr
