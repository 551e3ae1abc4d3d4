"""The host side of the search, without a device: search_plan() against the tests' own models of the schedule
(prove_model.schedule, LeafParallelModel.contemplate), TreeSearch.contemplate and contemplate_groups on a tree that was never
opened, with _rollout and _round stubbed to log, and the refusals of the search keywords by both constructors, whose texts
are written out as they stood before the constructors shared one check."""
import pytest
import torch

import prove_model
from leaf_parallel_model import LeafParallelModel, ValueTreeModel

from qtttgym_amd import SelfPlay, TreeSearch
from qtttgym_amd.tree import search_plan

KS = (1, 2, 3, 64)


def _cases():
    return [(r, K, fresh) for K in KS for r in range(3 * K + 2) for fresh in (True, False)]


# ---------------------------------------------------------------- the plan
def test_the_plan_is_the_models_schedule():
    for r, K, fresh in _cases():
        singles, sizes = search_plan(r, K, fresh)
        assert [1] * singles + sizes == prove_model.schedule(r, K, fresh), (r, K, fresh)
        assert singles + sum(sizes) == r and singles == (1 if r and fresh else 0)
        assert search_plan(r, K, fresh, rounds=False) == (r, [])


def test_the_plan_is_the_leaf_parallel_models(monkeypatch):
    monkeypatch.setattr(ValueTreeModel, "rollout", lambda self: self.log.append("rollout"))
    for r, K, fresh in _cases():
        m = LeafParallelModel.__new__(LeafParallelModel)
        m._games, m._queued, m.leaves, m.fresh, m.log = [], 0, K, fresh, []
        m.round_of = m.log.append
        m.contemplate(r)
        singles, sizes = search_plan(r, K, fresh, rounds=K > 1)       # the model's leaves == 1 is the search without rounds
        assert m.log == ["rollout"] * singles + sizes, (r, K, fresh)
        assert m.fresh == (fresh and not (K > 1 and r > 0))


class _Unopened:
    """A TreeSearch that was never opened on a device; _rollout and _round log (the rollout index they see, what they are
    asked) and advance the rollout index as the real ones do."""

    def __init__(self, leaves, fresh=True, capacity=10 ** 6, **attrs):
        t = self.t = TreeSearch.__new__(TreeSearch)
        t.leaves, t.leaf_eval, t.capacity, t.num_games, t.device = leaves, "value", capacity, 8, torch.device("cpu")
        t.rollout_idx, t._bound, t._fresh, self.log = 7, 1, fresh, []
        for k, v in attrs.items():
            setattr(t, k, v)

        def rollout():
            self.log.append((t.rollout_idx, "rollout"))
            t.rollout_idx += 1

        def one_round(k, g=None, ids=None, forced=None):
            self.log.append((t.rollout_idx, k) + (() if ids is None else (ids[1], forced)))
            t.rollout_idx += k

        t._rollout, t._round = rollout, one_round


@pytest.mark.parametrize("single_round", [False, True])
def test_contemplate_runs_the_plan_with_singles_of_either_kind(single_round):
    for r, K, fresh in _cases():
        for forced in (None, 2.0):
            u = _Unopened(K, fresh, eval_symmetries=(0,) if single_round else None, forced_playouts=forced)
            u.t.contemplate(r)
            singles, sizes = search_plan(r, K, fresh, rounds=K > 1 or forced is not None)
            steps = [1 if single_round else "rollout"] * singles + sizes
            starts = [7 + sum(1 if s == "rollout" else s for s in steps[:i]) for i in range(len(steps))]
            assert u.log == list(zip(starts, steps)), (r, K, fresh, forced)
            assert u.t.rollout_idx == 7 + r and u.t._bound == 1 + 2 * r
            assert u.t._fresh == (fresh and not (singles == 1 and (K > 1 or forced is not None)))


# ---------------------------------------------------------------- the group search
def _ids(*games):
    return torch.tensor(games, dtype=torch.int32), len(games)


def test_the_groups_start_at_the_same_rollout_index_and_the_counters_advance_once():
    u = _Unopened(2, fresh=False, forced_playouts=2.0)
    u.t.contemplate_groups(5, [(_ids(0, 3), 1, False), (_ids(1, 2, 5), 4, None)])
    assert u.log == [(7, 1, 2, False), (7, 2, 3, 2.0), (9, 2, 3, 2.0)]
    assert u.t.rollout_idx == 7 + 5 and u.t._bound == 1 + 10 and u.t._fresh is False
    fresh = _Unopened(2, fresh=True, forced_playouts=2.0)       # a listed root may lack priors: a plain round of one first
    fresh.t.contemplate_groups(5, [(_ids(1, 2, 5), 4, None)])
    assert fresh.log == [(7, 1, 3, False), (8, 2, 3, 2.0), (10, 1, 3, 2.0)]
    assert fresh.t.rollout_idx == 12 and fresh.t._bound == 11 and fresh.t._fresh is True     # the other games stay fresh
    one = _Unopened(2, fresh=False)                             # contemplate(games=) is the group search of one group
    one.t.contemplate(3, games=_ids(4), forced=False)
    assert one.log == [(7, 2, 1, False), (9, 1, 1, False)] and one.t.rollout_idx == 10 and one.t._bound == 7


def test_the_group_search_checks_every_bound_before_the_first_launch():
    a, b = _ids(0, 3), _ids(1, 2, 5)
    u = _Unopened(2, fresh=False)
    with pytest.raises(ValueError, match="a group's rollouts must be in 0..5"):
        u.t.contemplate_groups(5, [(a, 1, False), (b, 6, None)])
    with pytest.raises(ValueError, match="a group's rollouts must be in 0..5"):
        u.t.contemplate_groups(5, [(a, -1, False)])
    small = _Unopened(2, fresh=False, capacity=10)
    with pytest.raises(ValueError, match="5 rollouts could use 11 nodes, more than capacity 10"):
        small.t.contemplate_groups(5, [(a, 1, False), (b, 4, None)])
    late = _Unopened(2, fresh=False)
    late.t.rollout_idx = start = late.t.max_rollouts - 4
    with pytest.raises(ValueError, match="draw indices"):
        late.t.contemplate_groups(5, [(a, 1, False), (b, 4, None)])
    for x, idx in ((u, 7), (small, 7), (late, start)):
        assert x.log == [] and x.t.rollout_idx == idx and x.t._bound == 1
    for kw in (dict(root_policy="gumbel"), dict(exact_from=7), dict(prove=True)):
        with pytest.raises(ValueError, match="index their records by game"):
            _Unopened(2, fresh=False, **kw).t.contemplate_groups(5, [(a, 1, False)])
    with pytest.raises(ValueError, match=r"resident=True with contemplate\(games=\.\.\.\)"):
        _Unopened(2, fresh=False, resident=True).t.contemplate_groups(5, [(a, 1, False)])


# ---------------------------------------------------------------- the constructors' refusals, word for word
NET = object()                          # never looked at before the keywords are checked
VALUE = dict(net=NET, leaf_eval="value")
_FUSED = ": the fused launch runs the PUCT (or forced) select, one plain evaluation and the plain backup, nothing between them"
REFUSALS = [
    (dict(leaf_eval="values"), "leaf_eval must be one of ('playouts', 'value')"),
    (dict(leaf_eval="value"), 'leaf_eval="value" needs a net'),
    (dict(leaves=0, **VALUE), "leaves must be in 1..64"),
    (dict(leaves=65, **VALUE), "leaves must be in 1..64"),
    (dict(leaves=2, net=NET), 'leaves > 1 needs leaf_eval="value"'),
    (dict(virtual_loss=-1.0, **VALUE), "virtual_loss must be finite and >= 0"),
    (dict(virtual_loss=float("inf"), **VALUE), "virtual_loss must be finite and >= 0"),
    (dict(root_policy="ucb", **VALUE), "root_policy must be one of ('puct', 'gumbel')"),
    (dict(root_policy="gumbel", net=NET), 'root_policy="gumbel" needs a net and leaf_eval="value"'),
    (dict(max_considered=0, **VALUE), "max_considered must be in 1..36"),
    (dict(max_considered=37, **VALUE), "max_considered must be in 1..36"),
    (dict(c_visit=-1.0, **VALUE), "c_visit must be finite and >= 0"),
    (dict(c_scale=float("inf"), **VALUE), "c_scale must be finite"),
    (dict(eval_symmetries="all", net=NET), 'eval_symmetries needs leaf_eval="value"'),
    (dict(eval_symmetries=(8,), **VALUE), "a symmetry is 0..7, got 8"),
    (dict(exact_from=7, net=NET),
     'exact_from needs a net and leaf_eval="value": exact leaves replace the value head\'s estimate'),
    (dict(exact_from=5, **VALUE), "exact_from must be None or an integer in 6..9 (moves played)"),
    (dict(exact_from=True, **VALUE), "exact_from must be None or an integer in 6..9 (moves played)"),
    (dict(prove=1, exact_from=7, **VALUE), "prove must be True or False"),
    (dict(prove=True, **VALUE),
     "prove=True needs exact_from: the plain backup would hand a proven node its priors back"),
    (dict(forced_playouts=-1.0, **VALUE), "forced_playouts must be None or a finite number >= 0"),
    (dict(forced_playouts=True, **VALUE), "forced_playouts must be None or a finite number >= 0"),
    (dict(forced_playouts=2.0, net=NET),
     'forced_playouts needs a net and leaf_eval="value": the forced rounds are leaf-parallel rounds'),
    (dict(forced_playouts=2.0, root_policy="gumbel", **VALUE),
     'forced_playouts is a rule of the PUCT root: root_policy="gumbel" replaces that root'),
    (dict(resident="yes", **VALUE), "resident must be True or False"),
    (dict(rounds_per_launch=0, **VALUE), "rounds_per_launch must be an integer >= 1"),
    (dict(rounds_per_launch=2.0, resident=True, **VALUE), "rounds_per_launch must be an integer >= 1"),
    (dict(resident=True, net=NET), 'resident=True with leaf_eval="playouts" (or without a net): the fused launch evaluates '
                                   'the leaves with the value head, it plays no playouts'),
    (dict(resident=True, root_policy="gumbel", **VALUE), 'resident=True with root_policy="gumbel"' + _FUSED),
    (dict(resident=True, exact_from=7, **VALUE), "resident=True with exact_from" + _FUSED),
    (dict(resident=True, eval_symmetries="all", **VALUE), "resident=True with eval_symmetries" + _FUSED),
]
_BY_GAME = ("is not available with root_policy=\"gumbel\", exact_from or prove: their kernels index their records by game, "
            "not by a subset's dense rows")
SELFPLAY_REFUSALS = [
    (dict(playout_cap=(0.5, 4), resident=True, **VALUE),
     "resident=True with playout_cap: the cap's two groups are searched in subset rounds, which the fused launch does not run"),
    (dict(playout_cap=(0.5, 4), net=NET),
     'playout_cap needs a net and leaf_eval="value": the two groups are searched in subset rounds'),
    (dict(playout_cap=(0.5, 4), leaf_eval="value"),
     'playout_cap needs a net and leaf_eval="value": the two groups are searched in subset rounds'),
    (dict(playout_cap=(0.5, 4), root_policy="gumbel", **VALUE), "playout_cap " + _BY_GAME),
    (dict(playout_cap=(0.5, 4), exact_from=7, **VALUE), "playout_cap " + _BY_GAME),
    (dict(playout_cap=(0.5, 4), exact_from=7, prove=True, **VALUE), "playout_cap " + _BY_GAME),
    (dict(prune_targets=True, **VALUE), "prune_targets=True needs forced_playouts: it subtracts the visits that forcing added"),
]


@pytest.mark.parametrize("make", [lambda **kw: TreeSearch(4, capacity=64, **kw), lambda **kw: SelfPlay(4, n_rollouts=12, **kw)],
                         ids=["TreeSearch", "SelfPlay"])
def test_a_bad_search_keyword_is_refused_in_the_same_words_by_both_constructors(make):
    for kw, text in REFUSALS:
        with pytest.raises(ValueError) as e:
            make(**kw)
        assert str(e.value) == text, kw


def test_selfplays_own_refusals_and_the_subset_searchs_keep_their_words():
    for kw, text in SELFPLAY_REFUSALS:
        with pytest.raises(ValueError) as e:
            SelfPlay(4, n_rollouts=12, **kw)
        assert str(e.value) == text, kw
    t = TreeSearch.__new__(TreeSearch)
    t.leaf_eval, t.root_policy = "value", "gumbel"
    with pytest.raises(ValueError) as e:
        t._check_subset_search()
    assert str(e.value) == "a subset search (games=...) " + _BY_GAME.replace("a subset's", "the subset's")
    assert TreeSearch.subset_refused("puct", None, False) is False and TreeSearch.subset_refused("puct", 7, False) is True


def test_search_kwargs_is_the_trees_own_list_of_keys():
    sp = SelfPlay.__new__(SelfPlay)
    for i, k in enumerate(TreeSearch.SEARCH_KEYS):
        setattr(sp, k, i)
    assert sp.search_kwargs() == {k: i for i, k in enumerate(TreeSearch.SEARCH_KEYS)}
    import inspect
    assert set(TreeSearch.SEARCH_KEYS) < set(inspect.signature(TreeSearch.__init__).parameters)
    assert set(TreeSearch.SEARCH_KEYS) < set(inspect.signature(SelfPlay.__init__).parameters)
