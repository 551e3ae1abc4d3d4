"""CPU tests of playout cap randomisation (include/qttt_tree_subset.h, include/qttt_selfplay_cap.h,
TreeSearch.contemplate(games=), SelfPlay(playout_cap=)): the headers and the binding table; every argument error of the
new entries, in order, without a device; the constructors' refusals; the host's draw against hand-computed hash values and
its mean; the row-sign rule on hand-built staging rows.  No GPU."""
import ctypes
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
INCLUDE = os.path.join(ROOT, "include")
ERR_NULL, ERR_SIZE, ERR_ACTION = -1, -2, -3
SUBSET_NAMES = {"qttt_tree_select_batch_subset", "qttt_tree_backup_batch_subset", "qttt_tree_root_noise_subset"}
CAP_NAMES = {"qttt_selfplay_record_capped", "qttt_selfplay_harvest_capped"}

import cap_model as M  # noqa: E402
from qtttgym_amd import _host, _native  # noqa: E402


# ---------------------------------------------------------------- headers, binding table, documents
def test_headers_are_plain_c99_and_end_qttt_hs_include_chain():
    src = open(os.path.join(INCLUDE, "qttt.h")).read()
    assert src.index('#include "qttt_tree_forced.h"') < src.index('#include "qttt_tree_subset.h"') \
        < src.index('#include "qttt_selfplay_cap.h"')
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-x", "c", "-I" + INCLUDE, "-"],
                         input='#include "qttt.h"\nint main(void){'
                               'int (*s)(void *, int64_t, int64_t, uint64_t, uint32_t, int, int64_t, double, double, double,'
                               ' const int32_t *, int64_t, void *, void *, void *) = qttt_tree_select_batch_subset;\n'
                               'int (*b)(void *, int64_t, int64_t, int, const int32_t *, int64_t, const void *, const float *,'
                               ' const float *, void *) = qttt_tree_backup_batch_subset;\n'
                               'int (*n)(void *, int64_t, int64_t, uint64_t, uint32_t, int64_t, double, double, const int32_t *,'
                               ' int64_t, double *, uint8_t *, void *) = qttt_tree_root_noise_subset;\n'
                               'int (*r)(const void *, int64_t, int64_t, uint32_t, double, double, double, void *, double *,'
                               ' uint8_t *, uint8_t *, float *, uint8_t *, uint8_t *, int8_t *, uint8_t *, uint64_t, int64_t,'
                               ' double, int, uint32_t, double, double, const uint8_t *, void *) = qttt_selfplay_record_capped;\n'
                               'int (*h)(const void *, int64_t, int64_t, double, double, void *, double *, uint8_t *, uint8_t *,'
                               ' float *, uint8_t *, uint8_t *, int8_t *, uint8_t *, uint8_t *, uint8_t *, int64_t *, int64_t *,'
                               ' void *) = qttt_selfplay_harvest_capped;\n'
                               'return s == 0 || b == 0 || n == 0 || r == 0 || h == 0 || QTTT_ABI_VERSION != 6'
                               ' || QTTT_SELFPLAY_CAP_BASE != 0xA0000000u;}\n',
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_binding_headers_exports_build_list_and_documents_agree():
    import __graft_entry__ as entry
    for header, table, want in (("qttt_tree_subset.h", "TREE_SUBSET_SIGNATURES", SUBSET_NAMES),
                                ("qttt_selfplay_cap.h", "SELFPLAY_CAP_SIGNATURES", CAP_NAMES)):
        path = os.path.join(INCLUDE, header)
        src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
        names = set(re.findall(r"^(?:int|int64_t)\s+(qttt_\w+)\s*\(", src, flags=re.M))
        assert names == set(getattr(_native, table)) == want
        others = [getattr(_native, t) for t in dir(_native) if t.endswith("SIGNATURES") and t != table]
        assert not any(names & set(o) for o in others)
        assert path in entry.HEADERS
    for f in ("qttt_tree_subset_kernels.h", "qttt_tree_subset_host.h", "qttt_selfplay_cap_kernels.h"):
        assert os.path.join(ROOT, "qtttgym_amd", "csrc", f) in entry.HEADERS
    L = _native.lib()
    raw = ctypes.CDLL(_native.LIB_PATH)
    tables = dict(_native.TREE_SUBSET_SIGNATURES, **_native.SELFPLAY_CAP_SIGNATURES)
    for name, n_args in (("qttt_tree_select_batch_subset", 15), ("qttt_tree_backup_batch_subset", 10),
                         ("qttt_tree_root_noise_subset", 13), ("qttt_selfplay_record_capped", 25),
                         ("qttt_selfplay_harvest_capped", 19)):
        assert getattr(raw, name)
        assert getattr(L, name).argtypes == tables[name][1] and len(tables[name][1]) == n_args, name
    pruned = _native.TREE_FORCED_SIGNATURES["qttt_selfplay_record_stream_pruned"][1]
    assert _native.SELFPLAY_CAP_SIGNATURES["qttt_selfplay_record_capped"][1][:len(pruned) - 1] == pruned[:-1]
    assert L.qttt_abi_version() == _native.ABI_VERSION == 6             # additive entries: the ABI number stays
    # the draw's index range collides with no other: above the select's, below the noise's
    assert _native.TREE_SELECT_BASE + _native.TREE_MAX_ROLLOUTS <= _native.SELFPLAY_CAP_BASE
    assert _native.SELFPLAY_CAP_BASE + _native.SELFPLAY_MAX_CAP_DRAWS <= _native.TREE_NOISE_BASE
    text = open(os.path.join(INCLUDE, "qttt_tree_subset.h")).read() + open(os.path.join(INCLUDE, "qttt_selfplay_cap.h")).read()
    for rule in ("ASCENDING, DISTINCT", "row w * K + j", "NOT TOUCHED", "forced_k < 0 is the plain PUCT", "actions[g] ONLY",
                 "length[g] does not advance", "FIRST player", "QTTT_SELFPLAY_CAP_BASE + i"):
        assert rule in text, rule
    for doc in ("DESIGN.md", "README.md"):
        body = open(os.path.join(ROOT, doc)).read()
        for name in ("qttt_tree_select_batch_subset", "qttt_selfplay_record_capped", "playout_cap", "qttt_tree_subset.h",
                     "qttt_selfplay_cap.h"):
            assert name in body, (doc, name)


# ---------------------------------------------------------------- argument errors of the C entries, without a device
FIELDS = ("states", "pi", "mask", "done", "v", "action36", "length", "winner", "actions")


def test_return_codes_in_documented_order_without_device_work():
    """Fake addresses, never dereferenced: every call fails its checks first (or has nothing to do)."""
    L = _native.lib()
    nan, inf = float("nan"), float("inf")
    sizes = (dict(games=-1), dict(capacity=0), dict(capacity=_native.TREE_MAX_CAPACITY + 1), dict(n_ids=-1), dict(n_ids=3))

    def select(tree=0x1000, games=2, capacity=4, idx0=0, leaves=2, offset=0, vloss=1.0, k=-1.0, ids=0x4000, n_ids=1,
               paths=0x2000, leaf=0x3000):
        return L.qttt_tree_select_batch_subset(tree, games, capacity, 0, idx0, leaves, offset, 1.0, vloss, k, ids, n_ids, paths,
                                               leaf, None)

    def backup(tree=0x1000, games=2, capacity=4, leaves=2, ids=0x4000, n_ids=1, paths=0x2000, value=0x3000, probs=0x5000):
        return L.qttt_tree_backup_batch_subset(tree, games, capacity, leaves, ids, n_ids, paths, value, probs, None)

    def noise(tree=0x1000, games=2, capacity=4, idx=0, offset=0, eps=0.25, alpha=0.3, ids=0x4000, n_ids=1, out=0x2000,
              applied=0x3000):
        return L.qttt_tree_root_noise_subset(tree, games, capacity, 0, idx, offset, eps, alpha, ids, n_ids, out, applied, None)

    for kw in sizes + (dict(offset=-1), dict(leaves=0), dict(leaves=65), dict(idx0=(1 << 24) - 1), dict(vloss=-1.0),
                       dict(vloss=nan), dict(k=nan), dict(k=inf), dict(k=-inf)):
        assert select(**kw) == ERR_SIZE, kw
        assert select(**{"tree": None, "paths": None, "leaf": None, "ids": None, **kw}) == ERR_SIZE, kw      # sizes before nulls
        assert select(**{"tree": 0x1008, "ids": 0x4002, **kw}) == ERR_SIZE, kw                                # and alignment
    for k in (-1.0, -0.5, 0.0, 2.0):                                     # any finite k: negative is the plain root
        assert select(k=k, tree=None) == ERR_NULL
    assert select(games=0, n_ids=0, tree=None, ids=None) == 0 and select(n_ids=0, tree=None, ids=None, paths=None, leaf=None) == 0
    for kw in (dict(tree=None), dict(paths=None), dict(leaf=None), dict(ids=None)):
        assert select(**kw) == ERR_NULL, kw
        assert select(**{"tree": 0x1008, "paths": 0x2008, "ids": 0x4002, **kw}) == ERR_NULL, kw               # nulls before alignment
    for kw in (dict(tree=0x1008), dict(paths=0x2008), dict(ids=0x4002)):
        assert select(**kw) == ERR_ACTION, kw

    for kw in sizes + (dict(leaves=0), dict(leaves=65)):
        assert backup(**kw) == ERR_SIZE and backup(**{"tree": None, "ids": None, **kw}) == ERR_SIZE, kw
        assert backup(**{"tree": 0x1008, **kw}) == ERR_SIZE, kw
    assert backup(games=0, n_ids=0, tree=None) == 0 and backup(n_ids=0, tree=None, ids=None, value=None) == 0
    for kw in (dict(tree=None), dict(paths=None), dict(value=None), dict(probs=None), dict(ids=None)):
        assert backup(**kw) == ERR_NULL, kw
        assert backup(**{"tree": 0x1008, "ids": 0x4002, **kw}) == ERR_NULL, kw
    for kw in (dict(tree=0x1008), dict(paths=0x2008), dict(value=0x3002), dict(probs=0x5002), dict(ids=0x4002)):
        assert backup(**kw) == ERR_ACTION, kw

    for kw in sizes + (dict(offset=-1), dict(idx=_native.TREE_MAX_NOISE), dict(eps=-0.1), dict(eps=1.5), dict(eps=nan),
                       dict(alpha=0.0), dict(alpha=nan), dict(alpha=inf)):
        assert noise(**kw) == ERR_SIZE and noise(**{"tree": None, "ids": None, **kw}) == ERR_SIZE, kw
        assert noise(**{"tree": 0x1008, **kw}) == ERR_SIZE, kw
    assert noise(games=0, n_ids=0, tree=None) == 0 and noise(n_ids=0, tree=None, ids=None) == 0
    assert noise(tree=None) == noise(ids=None) == ERR_NULL and noise(tree=0x1008, ids=None) == ERR_NULL
    assert noise(out=None, applied=None, tree=0x1008) == ERR_ACTION      # the two outputs are optional
    assert noise(tree=0x1008) == noise(out=0x2004) == noise(ids=0x4002) == ERR_ACTION

    def record(tree=0x1000, games=1, n=8, alpha=1.0, temp=1.0, plies=2, draw=0, k=2.0, c=1.0, full=0x90000, **ptr):
        p = {f: 0x10000 * (i + 2) for i, f in enumerate(FIELDS)}
        p.update(ptr)
        return L.qttt_selfplay_record_capped(tree, games, 4, n, alpha, 1.0, -1.0, *(p[f] for f in FIELDS), 0, 0, temp, plies,
                                             draw, k, c, full, None)

    def harvest(tree=0x1000, games=1, capacity=4, v1=1.0, **ptr):
        names = FIELDS + ("harvest_len", "finished", "games_done", "tally")
        p = {f: 0x10000 * (i + 2) for i, f in enumerate(names)}
        p.update(ptr)
        return L.qttt_selfplay_harvest_capped(tree, games, capacity, v1, -1.0, *(p[f] for f in names), None)

    for kw in (dict(games=-1), dict(n=0), dict(alpha=0.0), dict(alpha=nan), dict(temp=0.0), dict(temp=inf), dict(plies=-1),
               dict(plies=11), dict(k=nan), dict(k=inf), dict(k=-inf), dict(c=nan), dict(c=-inf),
               dict(draw=_native.SELFPLAY_MAX_MOVE_DRAWS)):
        assert record(**kw) == ERR_SIZE, kw
        assert record(**{"tree": None, "pi": None, "full": None, **kw}) == ERR_SIZE, kw
    assert record(k=-1.0, c=nan, tree=None) == ERR_NULL                  # without pruning c_puct is not looked at
    assert record(games=0, tree=None, pi=None, full=None) == 0
    assert record(plies=0, tree=None) == ERR_NULL
    for f in ("tree", "full") + FIELDS:
        assert record(**{f: None}) == ERR_NULL, f
        assert record(**{f: None, "k": -1.0}) == ERR_NULL, f
        assert record(**{"tree": 0x1008, "pi": 0x30004, f: None}) == ERR_NULL, f                              # nulls before alignment
    assert record(tree=0x1008) == record(states=0x20008) == record(pi=0x30004) == record(v=0x60002) == ERR_ACTION
    for kw in (dict(games=-1), dict(capacity=0), dict(v1=nan), dict(v1=inf)):
        assert harvest(**kw) == ERR_SIZE and harvest(**{"tree": None, **kw}) == ERR_SIZE, kw
    assert harvest(games=0, tree=None) == 0
    for f in ("tree",) + FIELDS + ("harvest_len", "finished", "games_done", "tally"):
        assert harvest(**{f: None}) == ERR_NULL, f
    assert harvest(tree=0x1008) == harvest(states=0x20008) == harvest(pi=0x30004) == harvest(v=0x60002) == ERR_ACTION
    assert harvest(games_done=0xD0004) == harvest(tally=0xE0004) == ERR_ACTION


# ---------------------------------------------------------------- the keywords' host-side checks
def test_python_checks_the_keywords_before_it_asks_for_a_device():
    from qtttgym_amd import SelfPlay, TreeSearch
    net = object()                                                       # never looked at before the keywords are checked
    assert inspect.signature(SelfPlay.__init__).parameters["playout_cap"].default is None
    sig = inspect.signature(TreeSearch.contemplate).parameters
    assert sig["games"].default is None and sig["forced"].default is None
    assert inspect.signature(TreeSearch.add_root_noise).parameters["games"].default is None
    ok = dict(net=net, leaf_eval="value", n_rollouts=12)
    for bad in (0.5, (0.5,), (0.5, 4, 1), "abc", 3):
        with pytest.raises(ValueError, match=r"playout_cap must be None or \(p, n_fast\)"):
            SelfPlay(4, playout_cap=bad, **ok)
    for bad in (0.0, -0.1, 1.5, float("nan"), "1", True):
        with pytest.raises(ValueError, match=r"p must be a number in \(0, 1\]"):
            SelfPlay(4, playout_cap=(bad, 4), **ok)
    for bad in (0, 13, 4.0, True, "4"):
        with pytest.raises(ValueError, match="n_fast must be an integer in 1..n_rollouts"):
            SelfPlay(4, playout_cap=(0.5, bad), **ok)
    for kw in (dict(n_rollouts=12), dict(net=net, n_rollouts=12), dict(leaf_eval="value", n_rollouts=12)):
        with pytest.raises(ValueError, match='playout_cap needs a net and leaf_eval="value"'):
            SelfPlay(4, playout_cap=(0.5, 4), **kw)
    for kw in (dict(root_policy="gumbel"), dict(exact_from=7), dict(exact_from=7, prove=True)):
        with pytest.raises(ValueError, match="index their records by game"):
            SelfPlay(4, playout_cap=(0.5, 4), **ok, **kw)
    with pytest.raises(ValueError, match="TD\\(lambda\\) chains consecutive plies"):
        SelfPlay(4, playout_cap=(0.5, 4), td_lambda=0.5, value_targets=(1.0, -1.0), **ok)
    check = SelfPlay.check_playout_cap
    assert check(None, 12, "playouts", None, "puct", None, False, None) is None
    assert check((1, 12), 12, "value", net, "puct", None, False, None) == (1.0, 12)
    assert check((0.25, 1), 12, "value", net, "puct", None, False, None) == (0.25, 1)
    # the subset search's own refusals say why (a tree is needed for nothing else here)
    t = TreeSearch.__new__(TreeSearch)
    t.leaf_eval = "value"
    for kw in (dict(root_policy="gumbel"), dict(exact_from=7), dict(prove=True)):
        for k, v in kw.items():
            setattr(t, k, v)
        with pytest.raises(ValueError, match="index their records by game"):
            t._check_subset_search()
        for k in kw:
            delattr(t, k)
    t.leaf_eval = "playouts"
    with pytest.raises(ValueError, match='needs leaf_eval="value"'):
        t._check_subset_search()
    assert "playout_cap" in SelfPlay.__doc__ and "games" in TreeSearch.contemplate.__doc__
    assert "games=" in sys.modules[TreeSearch.__module__].__doc__
    assert "--playout-cap" in open(os.path.join(ROOT, "examples", "selfplay_train.py")).read()


# ---------------------------------------------------------------- the host's draw
def test_the_draw_at_hand_computed_hash_values():
    h = _native.lib().qttt_hash
    base = _native.SELFPLAY_CAP_BASE
    assert base == 0xA0000000
    for seed, off, ply in ((15, 0, 0), (15, 17, 3), (2 ** 63 + 5, (1 << 32) - 2, 9), (1, 1 << 40, (1 << 28) - 1)):
        want = np.array([h(seed, off + g, base + ply) for g in range(6)], dtype=np.uint64)
        assert np.array_equal(_host.counter_hash(seed, off, 6, base + ply), want)          # the restated hash, u64 for u64
        for p in (0.25, 0.5, 1.0):
            by_hand = np.array([(int(x) >> 11) * 2.0 ** -53 < p for x in want], dtype=np.uint8)
            assert np.array_equal(_host.cap_full_mask(seed, off, 6, ply, p), by_hand)
            assert np.array_equal(M.full_mask(seed, off, 6, ply, p), by_hand)
    # u = (h >> 11) * 2^-53 lies in [0, 1): p = 1 takes every game, and the comparison is strict
    assert _host.cap_full_mask(3, 0, 4096, 5, 1.0).all()
    x = int(h(15, 0, base))
    u = (x >> 11) * 2.0 ** -53
    assert 0.0 <= u < 1.0 and not _host.cap_full_mask(15, 0, 1, 0, u)[0] and _host.cap_full_mask(15, 0, 1, 0, math.nextafter(u, 1.0))[0]
    # different plies and different seeds are different draws
    a, b, c = (_host.cap_full_mask(s, 0, 4096, i, 0.5) for s, i in ((15, 0), (15, 1), (16, 0)))
    assert 0.4 < (a != b).mean() < 0.6 and 0.4 < (a != c).mean() < 0.6


@pytest.mark.parametrize("p", [0.25, 0.5, 0.9])
def test_the_draws_mean_over_65536_games(p):
    n = 1 << 16
    mean = _host.cap_full_mask(2026, 0, n, 7, p).mean()
    assert abs(mean - p) <= 4.0 * math.sqrt(p * (1.0 - p) / n), mean     # four binomial standard deviations


# ---------------------------------------------------------------- the row-sign rule
def _P(moves):
    return np.uint64(moves) << np.uint64(40)


def test_the_row_sign_rule_on_hand_built_staging_rows():
    # every ply recorded: row r has r moves played, and the signs are the row's parity, the existing kernels' bits
    every = np.array([_P(r) for r in range(6)], dtype=np.uint64)
    assert M.moves_played(every).tolist() == list(range(6))
    v = M.backfill(every, 1.0)
    assert v.tolist() == [1.0, -1.0, 1.0, -1.0, 1.0, -1.0] and v.dtype == np.float32
    assert np.array_equal(v.view(np.uint32), np.array([(-1.0) ** r for r in range(6)], dtype=np.float32).view(np.uint32))
    # plies 1, 2 and 5 were fast: the rows hold the states after 0, 3, 4 and 6 (terminal) moves
    rows = np.array([_P(0), _P(3), _P(4), _P(6)], dtype=np.uint64)
    assert M.backfill(rows, 1.0).tolist() == [1.0, -1.0, 1.0, 1.0]
    assert M.backfill(rows, -1.0).tolist() == [-1.0, 1.0, -1.0, -1.0]    # the second player won: value_targets (1, -1)
    # the reference's (1, 0) targets: a lost game trains towards 0, and a zero is +0.0 in every row
    z = M.backfill(rows, 0.0)
    assert np.array_equal(z.view(np.uint32), np.zeros(4, dtype=np.uint32))
    # a game whose plies were all fast: its terminal row alone, after seven moves the second player is to move
    assert M.backfill(np.array([_P(7)], dtype=np.uint64), 1.0).tolist() == [-1.0]
    # the other fields of the word do not matter: the done bit, the classical mask, the nibbles
    busy = rows | np.uint64(1 << 63) | np.uint64(0x1FF << 54) | np.uint64(0xFFFFFFFF)
    assert np.array_equal(M.backfill(busy, 1.0), M.backfill(rows, 1.0))


def test_the_subsets_are_the_issues():
    s = M.subsets(130)
    assert s["none"] == [] and s["all"] == list(range(130)) and s["last"] == [129]
    assert s["every other"] == list(range(0, 130, 2)) and s["one per workgroup"] == list(range(1, 130, 4))
    assert len({g // 4 for g in s["one per workgroup"]}) == len(s["one per workgroup"]) == 33
    assert M.subsets(1)["one per workgroup"] == [0] and M.subsets(3)["one per workgroup"] == [1]
    for G in (1, 3, 130):
        for ids in M.subsets(G).values():
            assert ids == sorted(set(ids)) and all(0 <= g < G for g in ids)
