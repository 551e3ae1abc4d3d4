"""The resident search (include/qttt_tree_resident.h, TreeSearch(resident=), SelfPlay(resident=)) on the MI355X, bit for bit
against the launches it replaces: a twin TreeSearch with identical bytes, seed and settings and resident=False runs the same
schedule through qttt_tree_select_batch[_forced] -> qttt_evaluate -> qttt_tree_backup_batch, and the WHOLE tree buffer is
compared after every contemplate(): game headers, node headers, slots, priors.  Every row's network result is a function of
that row alone and of a fixed accumulation order, so there is no tolerance anywhere and no case is left out.

Sizes: G in {1, 3, T + 1, 130} with T = qttt_tree_resident_games_per_group (a partial tile, a tile boundary, several tiles),
leaves in {1, 3, 8, 64} (64: one or two games per workgroup and waves without a game, the barrier case), f32 and bf16; every
K at G = T + 1 and every G at K = 8.  Roots 0..7 plies deep, terminal roots and roots with one legal move among them."""
import pytest
import torch

import cap_model as M
import gumbel_cases as C
from tree_harness import DEV, env_from_arrays

from qtttgym_amd import PolicyValueNet, ReplayBuffer, SelfPlay, TreeSearch, VecEnv, _native
from qtttgym_amd.actions import action36_to_pairs

pytestmark = pytest.mark.gpu
SEED, OFFSET, NOISE = 5, 17, (0.25, 0.3)
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
_NETS = {}


def _net(prec):
    if prec not in _NETS:
        _NETS[prec] = PolicyValueNet(C.net_state_dict("random"), device=DEV, dtype=DTYPES[prec])
    return _NETS[prec]


def _tile(K, prec):
    return int(_native.lib().qttt_tree_resident_games_per_group(K, _net(prec).precision))


def _tree(G, K, capacity, prec, resident, **kw):
    t = TreeSearch(G, capacity=capacity, net=_net(prec), seed=SEED, board_offset=OFFSET, device=DEV, leaf_eval="value",
                   leaves=K, resident=resident, **kw)
    t.tree.zero_()                                               # torch.empty's bytes: the twins start from identical ones
    t.reset(env_from_arrays(C.positions(G)))                     # roots 0..7 plies deep
    return t


def _pair(G, K, capacity, prec, **kw):
    res = {k: kw.pop(k) for k in ("rounds_per_launch",) if k in kw}
    return _tree(G, K, capacity, prec, False, **kw), _tree(G, K, capacity, prec, True, **res, **kw)


def _reference(t, r):
    """The oracle's schedule on the twin: contemplate itself where it runs rounds (leaves > 1 or forced_playouts); for
    leaves == 1 without forcing, the single rollout while the tree is fresh, then _round(1) repeated."""
    if t.leaves > 1 or t.forced_playouts is not None:
        t.contemplate(r)
        return
    assert t.rollout_idx + r <= t.max_rollouts and t._bound + 2 * r <= t.capacity
    if r and t._fresh:
        t._rollout()
        t._fresh = False
        r -= 1
        t._bound += 2
    for _ in range(r):
        t._round(1)
        t._bound += 2


def _assert_same(a, b, what):
    assert a.rollout_idx == b.rollout_idx and a._bound == b._bound and a._fresh == b._fresh, what
    if not torch.equal(a.tree, b.tree):
        G, cap = a.num_games, a.capacity
        for va, vb, part in zip(M.game_views(a.tree, G, cap), M.game_views(b.tree, G, cap), ("header", "nodes", "priors")):
            bad = torch.nonzero((va != vb).reshape(G, -1).any(1)).reshape(-1)[:8].tolist()
            assert not bad, (what, part, "games", bad)
        raise AssertionError((what, "bytes outside the games' views differ"))


def _budgets(K):
    """Rollouts that leave, after the single rollout of a fresh tree, no, one and several full rounds, with and without a
    remainder: at K = 8 they are 1, 2, 9, 17, 24, 31."""
    return sorted({1, 2, K + 1, 2 * K + 1, 3 * K, 4 * K - 1})


SIZES = [("T+1", K) for K in (1, 3, 8, 64)] + [(G, 8) for G in (1, 3, 130)]


# ---------------------------------------------------------------- 1. every budget, every size, both precisions
@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("G,K", SIZES, ids=lambda x: str(x))
def test_a_resident_search_leaves_the_bytes_of_the_rounds_it_replaces(G, K, prec):
    T = _tile(K, prec)
    assert T == (64 if prec == "f32" else 128) // K
    G = T + 1 if G == "T+1" else G
    assert _budgets(8) == [1, 2, 9, 17, 24, 31]
    for r in _budgets(K):
        second = K + 1                                           # on the searched tree: one full round and a remainder of 1
        a, b = _pair(G, K, 2 + 2 * (r + second), prec)
        assert torch.equal(a.tree, b.tree)
        for n in (r, second):
            _reference(a, n)
            b.contemplate(n)
            _assert_same(a, b, (G, K, prec, r, n))
        sa, sb = a.root_stats(), b.root_stats()
        assert all(torch.equal(sa[k], sb[k]) for k in sa)
        assert torch.equal(a.choose(), b.choose())
    assert int(sb["Ntot"].max()) > 0 and not bool(sb["overflow"].any())
    if G >= 130:                                                 # terminal roots are among them: no descent leaves such a root
        assert bool((sb["Ntot"] == 0).any()) and not bool((sb["Ntot"] == 0).all())


# ---------------------------------------------------------------- 2. a move, sync, compact and a second search
@pytest.mark.parametrize("prec,K,forced", [("f32", 8, None), ("bf16", 3, 2.0), ("f32", 1, None)], ids=str)
def test_through_a_move_sync_compact_and_a_second_search_on_the_reused_subtrees(prec, K, forced):
    G, r = 130, 2 * K + 2
    a, b = _pair(G, K, 2 + 2 * r + 1 + 2 * r + 4, prec, forced_playouts=forced)
    env_a, env_b = env_from_arrays(C.positions(G)), env_from_arrays(C.positions(G))
    for stage in range(2):
        _reference(a, r)
        b.contemplate(r)
        _assert_same(a, b, (stage, "search"))
        if stage == 0:
            acts = b.choose()
            assert torch.equal(acts, a.choose())
            for t, env in ((a, env_a), (b, env_b)):
                env.step_raw(action36_to_pairs(acts).contiguous())       # 255 at a terminal root: a noop
                t.sync(env)
                t.compact()
            _assert_same(a, b, "after sync and compact")
            assert bool((b.nodes_used() > 1).any())              # subtrees were kept: the second search reuses them


# ---------------------------------------------------------------- 3. a pool that overflows
@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_in_a_pool_of_12_nodes_that_overflows(prec):
    G, K, capacity, r = 130, 3, 12, 10
    a, b = _pair(G, K, capacity, prec)
    for t in (a, b):
        t._rollout()                                             # the single rollout, without the host's node bound
        t._fresh = False
    n_rounds = int(_native.lib().qttt_tree_resident_plan(K, r, None, 0))
    assert n_rounds == 4
    for k in (3, 3, 3, 1):
        a._round(k)
    b._resident_rounds(r)
    assert a.rollout_idx == b.rollout_idx == 1 + r and torch.equal(a.tree, b.tree)
    sa, sb = a.root_stats(), b.root_stats()
    assert torch.equal(sa["overflow"], sb["overflow"]) and torch.equal(sa["nodes_used"], sb["nodes_used"])
    assert bool(sb["overflow"].any()) and not bool(sb["overflow"].all()) and int(sb["nodes_used"].max()) <= capacity


# ---------------------------------------------------------------- 4. composition: root noise and forced playouts
@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("forced", [None, 0.0, 2.0], ids=str)
def test_root_noise_and_forced_playouts_compose(forced, prec):
    G, K, r = 130, 8, 25
    a, b = _pair(G, K, 2 + 2 * (1 + r), prec, forced_playouts=forced)
    for t in (a, b):
        if t is a:
            _reference(t, 1)
        else:
            t.contemplate(1)
        t.add_root_noise(*NOISE)
    _assert_same(a, b, "noised")
    _reference(a, r)
    b.contemplate(r)
    _assert_same(a, b, ("searched", forced))
    sa, sb = a.root_stats(), b.root_stats()
    assert set(sa) == set(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    if forced is not None:
        assert torch.equal(sa["forced"], sb["forced"]) and torch.equal(sa["n_pruned"], sb["n_pruned"])
        if forced > 0:
            assert bool((sb["n_pruned"] != sb["N"]).any())       # the forcing did something at these roots


# ---------------------------------------------------------------- 5. launch splitting
@pytest.mark.parametrize("prec,K", [("f32", 8), ("bf16", 3)], ids=str)
def test_rounds_per_launch_changes_no_byte(prec, K, monkeypatch):
    G, r = 2 * _tile(K, prec) + 1, 1 + 4 * K + 2                 # four full rounds and a remainder of 2
    a = _tree(G, K, 2 + 2 * r, prec, False)
    a.contemplate(r)
    for per, launches in ((1, 5), (2, 3), (64, 1)):
        b = _tree(G, K, 2 + 2 * r, prec, True, rounds_per_launch=per)
        log = []
        orig = TreeSearch._call
        monkeypatch.setattr(TreeSearch, "_call", lambda self, entry, *x, _o=orig, _l=log: (_l.append((entry, x)), _o(self, entry, *x))[1])
        b.contemplate(r)
        monkeypatch.undo()
        _assert_same(a, b, per)
        calls = [x for e, x in log if e == "qttt_tree_search_resident"]
        assert len(calls) == launches and [e for e, _ in log][:2] == ["qttt_tree_select", "qttt_tree_value_rollout"]
        assert len(log) == 2 + launches                          # the single rollout's two launches, then the fused ones
        assert sum(x[6] for x in calls) == r - 1 and all(x[6] % K == 0 for x in calls[:-1])
        assert [x[4] for x in calls] == [1 + sum(y[6] for y in calls[:i]) for i in range(len(calls))]      # the draw indices


# ---------------------------------------------------------------- 6. the default is the call sequence it always was
def test_resident_false_is_the_call_sequence_without_the_keyword(monkeypatch):
    calls = {}
    for name, extra in (("omitted", {}), ("false", dict(resident=False, rounds_per_launch=3)), ("true", dict(resident=True))):
        t = TreeSearch(6, capacity=80, net=_net("f32"), seed=SEED, board_offset=OFFSET, device=DEV, leaf_eval="value", leaves=3,
                       forced_playouts=2.0, **extra)
        t.tree.zero_()
        env = env_from_arrays(C.positions(6))
        log = calls[name] = []
        for obj in (TreeSearch, VecEnv):
            orig = obj._call
            monkeypatch.setattr(obj, "_call", lambda self, entry, *a, _o=orig, _l=log: (_l.append(entry), _o(self, entry, *a))[1])
        t.reset(env)
        t.contemplate(1)
        t.add_root_noise(*NOISE)
        t.contemplate(11)
        acts = t.choose()
        env.step_raw(action36_to_pairs(acts).contiguous())
        t.sync(env)
        t.compact()
        t.contemplate(12)
        monkeypatch.undo()
        calls[name + " bytes"] = t.tree.clone()
        assert not t._rounds if name == "true" else t._rounds    # the resident search allocates no round buffers
    assert calls["omitted"] == calls["false"] and len(calls["false"]) > 20
    assert not any("resident" in c for c in calls["false"])
    assert calls["true"].count("qttt_tree_search_resident") == 2
    assert not any(c in calls["true"] for c in ("qttt_tree_select_batch", "qttt_tree_select_batch_forced", "qttt_evaluate",
                                                "qttt_tree_backup_batch"))
    assert torch.equal(calls["omitted bytes"], calls["false bytes"]) and torch.equal(calls["true bytes"], calls["false bytes"])


# ---------------------------------------------------------------- 7. self-play
def _selfplay(resident, **kw):
    base = dict(n_rollouts=12, net=_net("f32"), seed=7, device=DEV, leaf_eval="value", leaves=4, value_targets=(1.0, -1.0))
    base.update(kw)
    return SelfPlay(8, resident=resident, **base)


@pytest.mark.parametrize("kw", [dict(), dict(forced_playouts=2.0, root_noise=NOISE, sample_plies=2, compact=True)], ids=str)
def test_selfplay_play_and_stream_are_what_they_were(kw):
    out = {}
    for resident in (False, True):
        sp = _selfplay(resident, **kw)
        batch = sp.play(seed=11)
        tree_after_play = sp.tree.root_stats()              # (the pools are torch.empty's: unused bytes are not compared)
        ring = ReplayBuffer(64, device=DEV, seed=3)
        stats = sp.stream(ring, 14, seed=5)
        out[resident] = (batch, tree_after_play, ring.views(), stats, sp._stream["batch"], sp.tree.root_stats())
    (b0, t0, r0, s0, g0, u0), (b1, t1, r1, s1, g1, u1) = out[False], out[True]
    for f in M.FIELDS:
        assert torch.equal(getattr(b0, f), getattr(b1, f)), ("batch", f)
        assert torch.equal(getattr(g0, f), getattr(g1, f)), ("staging", f)
    assert set(t0) == set(t1) and all(torch.equal(t0[k], t1[k]) and torch.equal(u0[k], u1[k]) for k in t0)
    assert set(r0) == set(r1)
    for k in r0:
        assert torch.equal(r0[k], r1[k]), ("ring", k)
    for k in ("games", "samples", "winners"):
        x, y = getattr(s0, k), getattr(s1, k)
        assert torch.equal(torch.as_tensor(x), torch.as_tensor(y)), ("stats", k)
    assert int(torch.as_tensor(s1.samples)) > 0 and int(b1.length.sum()) > 8
