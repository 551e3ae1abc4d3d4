"""Root exploration on the MI355X (include/qttt_tree_explore.h): qttt_tree_root_noise and qttt_selfplay_record_sampled
against the numpy model (tests/explore_model.py) at G = 1, 3 and 65 (a partial last workgroup), what the noise may and
may not touch in the tree, the search, the compaction and the self-play loop that go on from it, and the example.

The model's decisions equal the device's because tests/test_explore_cpu.py asserts, for exactly the cases used here
(explore_model.NOISE_CASES, NOISE_PARAMS, PLAY), that no decision is closer than 1e-9; what is left between the two is
the device library's log / cos / pow against numpy's, a few ulps: rtol = 1e-9 on the noise (a wrong draw, index or
decision changes it at order 1) and one f32 ulp on the mixed priors."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import explore_model as E
import nn_reference64 as R
import oracle
import tree_layout
from tree_harness import DEV, assert_stats_equal, boards, env_from_arrays, rollout, search, stats, two_plies_in
from value_tree_model import ValueTreeModel, root_pool

from qtttgym_amd import PolicyValueNet, SelfPlay, TreeSearch, VecEnv

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = 10
GS = [1, 3, 65]
KEYS = ("pi", "mask", "done", "v", "action36", "length", "winner", "actions")
FIELDS = KEYS + ("states",)


# ---------------------------------------------------------------- roots, networks
@functools.lru_cache(maxsize=None)
def _open_roots():
    """65 roots 0..8 plies deep that are not terminal and have a legal action (value_tree_model.root_pool's, the
    finished games left out): (import arrays, the lists of legal actions)."""
    arrays = root_pool(160)
    _, terminal, legal, _ = oracle.node_info(boards(arrays))
    keep = np.nonzero((terminal == 0) & (legal != 0))[0][:E.G_MAX]
    assert len(keep) == E.G_MAX
    arrays = {k: np.asarray(v)[keep] for k, v in arrays.items()}
    lists = [[a for a in range(36) if (int(m) >> a) & 1] for m in legal[keep]]
    assert {len(x) for x in lists} >= {36, 21, 3}          # full, mid-game and nearly full boards
    return arrays, lists


def _prefix(arrays, G, first=0):
    return {k: np.asarray(v)[first:first + G] for k, v in arrays.items()}


@functools.lru_cache(maxsize=None)
def _net(name):
    sd = {"sharp": R.sharp_counting_state_dict, "zero": R.zero_state_dict}[name]()
    return PolicyValueNet(sd, device=DEV, dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def _early_roots():
    """65 roots two plies in: a move later no game is over."""
    arrays = two_plies_in(E.G_MAX, 3)
    legal = oracle.node_info(boards(arrays))[2]
    return arrays, [[a for a in range(36) if (int(m) >> a) & 1] for m in legal]


def _tree(G, mode, seed=E.SEED, offset=E.OFFSET, first=0, capacity=64, early=False, zero=False):
    """A tree over the first G open roots (from `first`; early: the roots two plies in) after reset: mode "uniform",
    "network" (playouts guided by the sharp counting network) or "value".  (tree, env, legal lists)."""
    arrays, lists = _early_roots() if early else _open_roots()
    env = env_from_arrays(_prefix(arrays, G, first))
    kw = {"uniform": {}, "network": {"net": _net("sharp")}, "value": {"net": _net("sharp"), "leaf_eval": "value"}}[mode]
    t = TreeSearch(G, capacity=capacity, num_simulations=2, seed=seed, board_offset=offset, device=DEV, **kw)
    if zero:
        t.tree.zero_()                # the bytes no entry writes (padding, unused nodes) compare equal between two trees
    t.reset(env)
    return t, env, lists[first:first + G]


def _noise(t, epsilon=0.25, alpha=0.3):
    """add_root_noise with both outputs asked for, pre-filled so that an unwritten entry shows: (noise, applied, P)."""
    noise = torch.full((t.num_games, 36), 7.0, dtype=torch.float64, device=DEV)
    applied = torch.full((t.num_games,), 7, dtype=torch.uint8, device=DEV)
    t.add_root_noise(epsilon, alpha, noise=noise, applied=applied)
    return noise.cpu().numpy(), applied.cpu().numpy(), t.root_stats()["P"].cpu().numpy()


def _assert_noise_is_the_model(t, legal, epsilon, alpha, noise_idx=0):
    """One noise call on `t` against the model; returns (the largest relative deviation of the noise, the noise)."""
    G = t.num_games
    before = t.root_stats()["P"].cpu().numpy()
    assert t.noise_idx == noise_idx
    noise, applied, after = _noise(t, epsilon, alpha)
    assert (t.seed, t.board_offset, noise_idx, E.G_MAX) in E.NOISE_CASES and (epsilon, alpha) in E.NOISE_PARAMS
    ref, ref_applied, _ = E.noise_rows(t.seed, t.board_offset, noise_idx, legal, alpha)
    assert ref_applied.all() and (applied == 1).all()
    np.testing.assert_allclose(noise, ref, rtol=1e-9, atol=0.0)
    worst = 0.0
    for g in range(G):
        illegal = [a for a in range(36) if a not in legal[g]]
        assert not noise[g, illegal].any() and not after[g, illegal].any(), g
        worst = max(worst, float(np.max(np.abs(noise[g, legal[g]] - ref[g, legal[g]]) / ref[g, legal[g]])))
        want = E.mix(before[g], ref[g], legal[g], epsilon)
        got = after[g].astype(np.float32)
        assert np.array_equal(got.astype(np.float64), after[g]), g                 # P is a stored f32 now
        assert (np.abs(got[legal[g]] - want[legal[g]]) <= np.spacing(want[legal[g]])).all(), g
    return worst, noise


# ---------------------------------------------------------------- 1. the noise against the model
@pytest.mark.parametrize("epsilon,alpha", E.NOISE_PARAMS)
@pytest.mark.parametrize("mode", ["uniform", "network"])
@pytest.mark.parametrize("G", GS)
def test_noise_and_mixed_priors_match_the_model(G, mode, epsilon, alpha):
    t, _, legal = _tree(G, mode)
    t.contemplate(1)
    before = t.root_stats()["P"].cpu().numpy()
    for g in range(G):
        if mode == "uniform":
            assert (before[g, legal[g]] == 1.0 / len(legal[g])).all()
        else:
            assert len(set(before[g, legal[g]].tolist())) > 1 or len(legal[g]) == 1      # the sharp network's priors
    worst, _ = _assert_noise_is_the_model(t, legal, epsilon, alpha)
    print("G = %d, %s, alpha = %g: largest relative deviation of the noise from the model %.3g" % (G, mode, alpha, worst))


# ---------------------------------------------------------------- 2. only the root changes
@pytest.mark.parametrize("G", GS)
def test_only_the_roots_prior_row_and_flags_change(G):
    t, env, legal = _tree(G, "uniform", early=True)
    t.contemplate(6)                                         # children with statistics and priors of their own
    from qtttgym_amd.actions import action36_to_pairs
    env.step_raw(action36_to_pairs(t.choose()).contiguous())
    t.sync(env)                                              # the root is a node in the middle of the pool now
    t.contemplate(1)
    cap = t.capacity
    g0, n0, p0, tail0 = (x.copy() for x in tree_layout.decode(t.tree.cpu().numpy(), G, cap))
    _, applied, _ = _noise(t)
    g1, n1, p1, tail1 = tree_layout.decode(t.tree.cpu().numpy(), G, cap)
    assert (applied == 1).all()
    assert g0.tobytes() == g1.tobytes() and tail0.tobytes() == tail1.tobytes()
    root = g0["root"]
    assert (root > 0).all()
    rows = np.arange(G)
    assert ((n0["flags"][rows, root] & tree_layout.NODE_UNIFORM) != 0).all()
    assert np.array_equal(n1["flags"][rows, root], n0["flags"][rows, root] & ~np.uint32(tree_layout.NODE_UNIFORM))
    assert ((n1["flags"][rows, root] & tree_layout.NODE_PRIORS) != 0).all()
    n0["flags"][rows, root] = n1["flags"][rows, root]
    assert n0.tobytes() == n1.tobytes()                      # every other byte of every node record
    assert not np.array_equal(p0[rows, root], p1[rows, root])
    p0[rows, root] = p1[rows, root]
    assert p0.tobytes() == p1.tobytes()                      # every other priors row


# ---------------------------------------------------------------- 3. roots that stay untouched
@pytest.mark.parametrize("G", GS)
def test_roots_without_priors_and_terminal_roots_are_left_alone(G):
    t, _, _ = _tree(G, "uniform")                            # straight after reset: no priors yet
    before = t.tree.clone()
    noise, applied, P = _noise(t)
    assert not applied.any() and not noise.any() and not P.any() and torch.equal(t.tree, before)
    env = VecEnv(G, device=DEV, seed=3)
    env.step_random_many(9)                                  # finished games
    assert bool(env.node_info(python_key=False)["terminal"].all())
    for mode in ("uniform", "value"):
        t, _, _ = _tree(G, mode)
        t.reset(env)
        t.contemplate(2)                                     # a terminal root never gets priors
        before = t.tree.clone()
        noise, applied, _ = _noise(t)
        assert not applied.any() and not noise.any() and torch.equal(t.tree, before), mode
        assert t.noise_idx == 1


# ---------------------------------------------------------------- 4. the search goes on from the noised priors
def _adopt_priors(m, P, applied):
    for g, st in enumerate(m.games):
        if applied[g]:
            n = st["nodes"][st["root"]]
            n.P = {a: float(P[g, a]) for a in n.legal}
            n.probs = P[g].astype(np.float32)


@pytest.mark.parametrize("mode", ["uniform", "network", "value"])
@pytest.mark.parametrize("G", GS)
def test_the_search_goes_on_from_the_noised_priors(G, mode):
    arrays = _prefix(_open_roots()[0], G)
    capacity = 1 + 2 * 25
    if mode == "value":
        net = _net("sharp")
        env = env_from_arrays(arrays)
        t = TreeSearch(G, capacity=capacity, net=net, seed=E.SEED, board_offset=E.OFFSET, device=DEV, leaf_eval="value")
        t.reset(env)
        m = ValueTreeModel(1, seed=E.SEED, board_offset=E.OFFSET)
        m.reset(boards(arrays))

        def one():
            m.select()
            t.contemplate(1)
            ev = t.leaf.evaluate(net, rows=("value", "probs"))
            m.backup(ev["value"].cpu().numpy(), ev["probs"].cpu().numpy())
    else:
        t, m, env = search(arrays, capacity, 2, net=None if mode == "uniform" else _net("sharp"), seed=E.SEED, offset=E.OFFSET)

        def one():
            rollout(t, m)
    one()
    _, applied, P = _noise(t)
    assert (applied == 1).all()
    _adopt_priors(m, P, applied)
    for _ in range(24):
        one()
    dev, ref = stats(t), m.root_stats()
    assert_stats_equal(dev, ref, ("N", "W", "Q", "P", "Ntot", "choose", "nodes_used"))
    assert (dev["Ntot"] == 24).all()                         # 25 rollouts; the first ends on the root: no edge


# ---------------------------------------------------------------- 5. compaction keeps the noise
@pytest.mark.parametrize("G", GS)
def test_compaction_keeps_a_formerly_uniform_roots_noised_priors(G):
    from qtttgym_amd.actions import action36_to_pairs
    t, env, _ = _tree(G, "uniform", early=True)
    t.contemplate(8)
    env.step_raw(action36_to_pairs(t.choose()).contiguous())
    t.sync(env)                                              # the root: a visited child, uniform priors, index > 0
    t.contemplate(1)
    _, applied, P = _noise(t)
    assert (applied == 1).all()
    twin = TreeSearch(G, capacity=t.capacity, num_simulations=2, seed=t.seed, board_offset=t.board_offset, device=DEV)
    twin.reset(env)
    twin.tree.copy_(t.tree)
    twin.rollout_idx, twin._bound = t.rollout_idx, t._bound
    used = t.nodes_used().cpu().numpy()
    t.compact()
    assert (t.nodes_used().cpu().numpy() < used).all()       # it moved the root down to index 0
    assert np.array_equal(t.root_stats()["P"].cpu().numpy(), P)
    t.contemplate(8)
    twin.contemplate(8)
    a, b = stats(t), stats(twin)
    assert_stats_equal(a, b, ("N", "W", "Q", "P", "Ntot", "choose"))
    assert np.array_equal(a["P"], P)


# ---------------------------------------------------------------- 6. determinism and sharding
def test_noise_is_a_function_of_seed_index_and_offset():
    G = E.G_MAX
    runs = {}
    for key, (seed, idx) in {"a": (E.SEED, 0), "b": (E.SEED, 0), "idx": (E.SEED, 1), "seed": (E.SEED + 1, 0)}.items():
        t, _, legal = _tree(G, "uniform", seed=seed, zero=True)
        t.contemplate(1)
        t.noise_idx = idx
        runs[key] = (_assert_noise_is_the_model(t, legal, 0.25, 0.3, noise_idx=idx)[1], t.tree.clone())
    assert np.array_equal(runs["a"][0], runs["b"][0]) and torch.equal(runs["a"][1], runs["b"][1])
    for other in ("idx", "seed"):
        assert not np.isclose(runs["a"][0], runs[other][0], rtol=1e-3, atol=0.0)[runs["a"][0] > 0].all(), other


def test_a_shard_draws_what_its_games_draw_in_the_whole_batch():
    whole, _, legal = _tree(E.G_MAX, "uniform", offset=E.BIG_OFFSET)
    whole.contemplate(1)
    _assert_noise_is_the_model(whole, legal, 0.25, 0.3)       # fold_id's high word takes part: offset > 2^32
    whole2, _, _ = _tree(E.G_MAX, "uniform", offset=E.BIG_OFFSET)
    whole2.contemplate(1)
    noise, _, P = _noise(whole2)
    part, _, _ = _tree(3, "uniform", offset=E.BIG_OFFSET + 3, first=3)
    part.contemplate(1)
    noise3, applied3, P3 = _noise(part)
    assert (applied3 == 1).all() and np.array_equal(noise3, noise[3:6]) and np.array_equal(P3, P[3:6])


# ---------------------------------------------------------------- 7. epsilon = 0
@pytest.mark.parametrize("G", GS)
def test_epsilon_zero_leaves_network_priors_bit_for_bit(G):
    t, _, _ = _tree(G, "network")
    t.contemplate(1)
    before = t.root_stats()["P"]
    noise, applied, after = _noise(t, 0.0, 0.3)
    assert (applied == 1).all() and (noise.sum(1) > 0.99).all()
    assert np.array_equal(before.cpu().numpy().view(np.uint64), after.view(np.uint64))


# ---------------------------------------------------------------- the sampled record
def _host(batch):
    return {k: getattr(batch, k).cpu().numpy() for k in FIELDS}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _assert_same_bytes(a, b):
    for k in FIELDS:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), (k, np.argwhere(_bits(a[k]) != _bits(b[k]))[:6])


def _record_args(sp, tree, ply, batch):
    return (tree.tree.data_ptr(), sp.num_games, tree.capacity, ply, sp.n_rollouts, sp.alpha, sp.v_first, sp.v_second,
            batch.states.data_ptr(), batch.pi.data_ptr(), batch.mask.data_ptr(), batch.done.data_ptr(), batch.v.data_ptr(),
            batch.action36.data_ptr(), batch.length.data_ptr(), batch.winner.data_ptr(), batch.actions.data_ptr())


def _hand_loop(sp, seed, record, noise=None):
    """play() spelled out with the public calls on an env and a tree of its own; record(tree, ply, batch) -> actions."""
    G, Rn = sp.num_games, sp.n_rollouts
    env = VecEnv(G, device=DEV, seed=seed)
    tree = TreeSearch(G, capacity=sp.capacity, num_simulations=sp.num_simulations, c_puct=sp.c_puct, net=sp.net,
                      seed=2 * seed + 1, device=DEV, leaf_eval=sp.leaf_eval)
    tree.reset(env)
    batch = sp.new_batch()
    for ply in range(ROWS):
        if ply < ROWS - 1:
            if noise is None:
                tree.contemplate(Rn)
            else:
                tree.contemplate(1)
                tree.add_root_noise(*noise)
                tree.contemplate(Rn - 1)
        env.step_raw(record(tree, ply, batch))
        tree.sync(env)
    return batch, env


# 8. sample_plies = 0 is qttt_selfplay_record
@pytest.mark.parametrize("G", GS)
def test_sampled_record_with_no_sampled_ply_is_the_record(G):
    seed = 7
    sp = SelfPlay(G, n_rollouts=8, num_simulations=2, seed=seed, device=DEV)

    def sampled(tree, ply, batch):
        sp._call("qttt_selfplay_record_sampled", *_record_args(sp, tree, ply, batch), tree.seed, tree.board_offset, 0.5, 0)
        return batch.actions

    def plain(tree, ply, batch):
        sp._call("qttt_selfplay_record", *_record_args(sp, tree, ply, batch))
        return batch.actions

    a, env_a = _hand_loop(sp, seed, sampled)
    b, env_b = _hand_loop(sp, seed, plain)
    _assert_same_bytes(_host(a), _host(b))
    assert torch.equal(env_a.state, env_b.state)
    _assert_same_bytes(_host(sp.play()), _host(b))           # and play()'s default path is that loop


# 9, 10. whole games against the model
@functools.lru_cache(maxsize=None)
def _model_games(temperature, sample_plies):
    return E.play(*E.PLAY, temperature=temperature, sample_plies=sample_plies)


@pytest.mark.parametrize("temperature,sample_plies", [(1.0, 10), (1.0, 2), (0.5, 10)])
@pytest.mark.parametrize("G", GS)
def test_whole_sampled_games_match_the_model(G, temperature, sample_plies):
    """temperature = 1: every quantity of the draw is an exact integer in a double.  temperature = 0.5: pow, under the
    margin condition of tests/test_explore_cpu.py.  sample_plies = 2: the later plies play choose."""
    _, Rn, S, seed = E.PLAY
    ref, ref_env, _ = _model_games(temperature, sample_plies)
    sp = SelfPlay(G, n_rollouts=Rn, num_simulations=S, seed=seed, temperature=temperature, sample_plies=sample_plies, device=DEV)
    dev = _host(sp.play())
    for k in KEYS:
        want = ref[k][:, :G] if ref[k].shape[0] == ROWS and k not in ("length", "winner", "actions") else ref[k][:G]
        assert np.array_equal(_bits(dev[k]), _bits(np.ascontiguousarray(want))), (k, np.argwhere(_bits(dev[k]) != _bits(np.ascontiguousarray(want)))[:6])
    words = dev["states"].view(np.uint64).reshape(ROWS, 2, -1)[:, :, :G]
    for t in range(ROWS):
        live = [g for g in range(G) if ref["recs"][t][g] is not None]
        if live:
            P, Q = tree_layout.pack_positions([ref["recs"][t][g] for g in live], DEV)
            assert np.array_equal(words[t, 0, live], P) and np.array_equal(words[t, 1, live], Q), t
    ex = {k: v.cpu().numpy() for k, v in sp.env.export_boards().items()}
    assert np.array_equal(ex["board"], ref_env.board[:G]) and np.array_equal(ex["n_moves"], ref_env.n_moves[:G])
    if G == E.G_MAX:
        import selfplay_model
        plain, _ = selfplay_model.play(G, Rn, S, seed=seed)
        assert (plain["action36"][0] != ref["action36"][0]).any()          # the draw is not choose
        if sample_plies == 2:
            assert not np.array_equal(_model_games(temperature, 10)[0]["action36"], ref["action36"])


# 11. a root without a visit
def test_sampled_record_of_an_unvisited_root_falls_back_to_choose():
    G = 3
    sp = SelfPlay(G, n_rollouts=4, num_simulations=2, sample_plies=10, device=DEV)
    tree = TreeSearch(G, capacity=4, num_simulations=2, device=DEV)
    tree.reset(VecEnv(G, device=DEV))
    batch = sp.new_batch()
    sp.record(tree, 0, batch)
    assert torch.isnan(batch.pi[0]).all() and (batch.mask[0] == 1).all() and not batch.pi[1:].any()
    assert (batch.action36[0] == 0).all() and (batch.actions == torch.tensor([0, 1], dtype=torch.uint8, device=DEV)).all()


# ---------------------------------------------------------------- 12. play() against the public calls
@pytest.mark.parametrize("mode", ["uniform", "value"])
def test_play_with_exploration_is_the_hand_loop_of_the_public_calls(mode):
    G, Rn, seed = 65, 12, 11
    kw = dict(n_rollouts=Rn, num_simulations=2, seed=seed, device=DEV)
    if mode == "value":
        kw.update(net=_net("sharp"), leaf_eval="value")
    sp = SelfPlay(G, root_noise=(0.25, 0.3), sample_plies=4, **kw)
    batch = _host(sp.play())
    other = SelfPlay(G, root_noise=(0.25, 0.3), sample_plies=4, **kw)
    hand, env = _hand_loop(other, seed, other.record, noise=(0.25, 0.3))
    _assert_same_bytes(batch, _host(hand))
    assert torch.equal(sp.env.state, env.state) and sp.tree.noise_idx == ROWS - 1 == sp.tree.rollout_idx // Rn
    # the defaults: only the entries that existed before
    plain = SelfPlay(G, **kw)

    def record(tree, ply, b):
        plain._call("qttt_selfplay_record", *_record_args(plain, tree, ply, b))
        return b.actions

    hand0, env0 = _hand_loop(plain, seed, record)
    base = _host(plain.play())
    _assert_same_bytes(base, _host(hand0))
    assert torch.equal(plain.env.state, env0.state) and plain.tree.noise_idx == 0
    assert not np.array_equal(base["action36"], batch["action36"])


# ---------------------------------------------------------------- 13. diversity
def test_sampling_the_first_move_makes_the_games_of_a_batch_differ():
    G, Rn, seed = 65, 8, 4
    kw = dict(n_rollouts=Rn, net=_net("zero"), leaf_eval="value", seed=seed, device=DEV)
    first = SelfPlay(G, **kw).play().action36[0].cpu().numpy()
    assert len(set(first.tolist())) == 1                     # one network, one empty board, no draw: one opening
    sampled = SelfPlay(G, sample_plies=1, **kw).play().action36[0].cpu().numpy()
    tree = TreeSearch(G, capacity=1 + 2 * Rn, net=_net("zero"), seed=2 * seed + 1, device=DEV, leaf_eval="value")
    tree.reset(VecEnv(G, device=DEV, seed=seed))
    tree.contemplate(Rn)
    N = tree.root_stats()["N"].cpu().numpy()
    want = np.array([E.sample_move(N[g], list(range(36)), 2 * seed + 1, g, 0, 1.0)[0] for g in range(G)])
    assert np.array_equal(sampled, want)
    assert np.array_equal(np.bincount(sampled, minlength=36), np.bincount(want, minlength=36))
    assert len(set(sampled.tolist())) > 1


# ---------------------------------------------------------------- 14. the example
def test_selfplay_train_example_runs_with_the_exploration_flags(tmp_path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "selfplay_train.py"), "--games", "64", "--rollouts", "8",
                          "--epochs", "1", "--runs", "1", "--leaf-eval", "value", "--value-targets", "1,-1",
                          "--root-noise", "0.25,0.3", "--temperature", "0.5", "--sample-plies", "4",
                          "--out", str(tmp_path / "model.pt")], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "run 0:" in out.stdout and " of 64 games " in out.stdout, out.stdout
    assert (tmp_path / "model.pt").exists()
