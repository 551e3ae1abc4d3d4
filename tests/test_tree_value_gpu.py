"""The value rollout (include/qttt_tree_value.h, TreeSearch(leaf_eval="value")) on the MI355X: whole trees bit for bit
against tests/value_tree_model.py's ValueTreeModel under the exact networks, in both precisions, at one game more than
each tile, through a move, a sync and a compaction, and in a pool small enough to overflow; under general weights with
the model fed qttt_evaluate's rows, where the fused call's own leaf_value / leaf_probs must be those rows; the modes'
independence; a NaN weight; SelfPlay; games == 0.

The model's trees are computed once per (network, pool capacity) for the 129-game pool and shared: games are
independent, so the first G games of that model are the model of the G-game pool."""
import copy
import functools

import numpy as np
import pytest
import torch

import nn_reference64 as R
import selfplay_model
import tree_layout
import tree_model
from tree_harness import DEV, SENTINEL, TAIL, boards, env_from_arrays, export
from value_tree_model import OVERFLOW_CAPACITY, ValueTreeModel, root_pool

from qtttgym_amd import PolicyValueNet, SelfPlay, TreeSearch, VecEnv
from qtttgym_amd.actions import action36_to_pairs

pytestmark = pytest.mark.gpu
SEED, OFFSET, G_MAX = 5, 17, 129
FIRST, SECOND = 40, 20                       # rollouts before and after the move
CAPACITY = 1 + 2 * FIRST + 1 + 2 * SECOND
NETS = {"zero": R.zero_state_dict, "greedy": R.greedy_state_dict, "counting": R.counting_state_dict,
        "sharp": R.sharp_counting_state_dict}
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}


def _prefix(arrays, G):
    return {k: np.asarray(v)[:G] for k, v in arrays.items()}


@functools.lru_cache(maxsize=None)
def _pool():
    return root_pool(G_MAX)


@functools.lru_cache(maxsize=None)
def _device_net(name, dtype):
    sd = NETS[name]() if name in NETS else (R.golden_state_dict(R.load_golden()) if name == "shipped"
                                             else R.random_state_dict(int(name)))
    return PolicyValueNet(sd, device=DEV, dtype=DTYPES[dtype])


def _move_of(m):
    """The move of every game after the first rollouts: even games play the model's choice, odd games their least
    visited legal action (often a child that was never expanded: a fresh root); finished games do not move."""
    act = np.full(len(m.games), 255, dtype=np.uint8)
    for g, st in enumerate(m.games):
        n = st["nodes"][st["root"]]
        if not n.terminal and n.legal:
            act[g] = tree_model.choose(n) if g % 2 == 0 else min(n.legal, key=lambda a: n.N[a])
    return act, (np.arange(len(m.games)) // 2 % 2).astype(np.uint8)


def _evaluate_probs(leaves):
    """qttt_evaluate's f32 probs of positions given as OracleBoards, under the counting network."""
    env = env_from_arrays({"board": leaves.board, "moves": leaves.moves, "n_moves": leaves.n_moves, "qmask": leaves.qmask,
                           "n_q": leaves.n_q})
    return env.evaluate(_device_net("counting", "f32"), rows=("probs",))["probs"].cpu().numpy()


@functools.lru_cache(maxsize=None)
def _model_stages(net, capacity):
    """The model of the 129-game pool: its trees after FIRST rollouts, after the move and the sync, and after SECOND
    more rollouts without and with a compaction in between; and the move."""
    arrays = _pool()
    m = ValueTreeModel(1, seed=SEED, board_offset=OFFSET, capacity=capacity, net=NETS[net]())
    if net == "counting":             # exact value and logits, but the softmax of its logits is the device's expf
        m.probs_of = _evaluate_probs
    m.reset(boards(arrays))
    for _ in range(FIRST):
        m.rollout()
    stages = {"first": copy.deepcopy(m)}
    act, bits = _move_of(m)
    after, _ = tree_model.after_move(m.root_positions(), act, bits)
    m.sync(after)
    stages["synced"] = copy.deepcopy(m)
    for compact in (False, True):
        c = copy.deepcopy(m)
        if compact:
            c.compact()
        for _ in range(SECOND):
            c.rollout()
        stages["second", compact] = c
    return stages, act, bits


def _view(m, G):
    v = copy.copy(m)
    v.games = m.games[:G]
    return v


def _search(arrays, capacity, net, S=1, **kw):
    """A value search over a sentinel-filled buffer of the test's own, with a tail, as tree_harness.search makes."""
    env = env_from_arrays(arrays)
    G = env.num_envs
    t = TreeSearch(G, capacity=capacity, num_simulations=S, net=net, seed=SEED, board_offset=OFFSET, device=DEV, **kw)
    nbytes = tree_layout.tree_bytes(G, capacity)
    t.tree = torch.full((nbytes + TAIL,), SENTINEL, dtype=torch.uint8, device=DEV)
    t.reset(env)
    return t, env


def _check(t, m, compacted=False):
    return tree_layout.assert_tree_equals_model(t.tree.cpu().numpy(), t.num_games, t.capacity, m, SENTINEL, DEV,
                                                compacted=compacted)


def _rollouts(t, n, bounded=True):
    if bounded:
        t.contemplate(n)
    else:
        for _ in range(n):
            t._rollout()


# ---------------------------------------------------------------- whole trees under the exact networks
def _whole_trees(net, dtype, G, compact, capacity, model_capacity):
    stages, act, bits = _model_stages(net, model_capacity)
    bounded = model_capacity is None
    t, env = _search(_prefix(_pool(), G), capacity, _device_net(net, dtype), leaf_eval="value")
    assert t._out is None and t.max_rollouts == 1 << 24
    _rollouts(t, FIRST, bounded)
    rows = _check(t, _view(stages["first"], G))
    assert rows > 0 or G == 1
    even = np.arange(G) % 2 == 0
    assert np.array_equal(t.choose().cpu().numpy()[even & (act[:G] != 255)], act[:G][even & (act[:G] != 255)])
    env.step_raw(action36_to_pairs(torch.as_tensor(act[:G], device=DEV)).contiguous(), torch.as_tensor(bits[:G], device=DEV))
    if bounded:
        t.sync(env)
    else:
        t._call("qttt_tree_sync", t.tree.data_ptr(), G, capacity, env.state.data_ptr())
    _check(t, _view(stages["synced"], G))
    if compact:
        t.compact()
    _rollouts(t, SECOND, bounded)
    final = _view(stages["second", compact], G)
    _check(t, final, compacted=compact)
    over = np.array([d["overflow"] for d in final.dump()])
    assert np.array_equal(t.root_stats()["overflow"].cpu().numpy(), over)
    if G == G_MAX:                    # the coverage floor of tests/test_tree_value_cpu.py, on the trees just compared
        ends = final.ends
        assert len(ends["terminal"]) == 6 and ends["fresh"] > 0 and (ends["overflowed"] > 0) == (model_capacity is not None)
    return over


@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("G", [1, 3, 65, 129])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("net", list(NETS))
def test_whole_trees_match_the_model_bit_for_bit(net, dtype, G, compact):
    assert not _whole_trees(net, dtype, G, compact, CAPACITY, None).any()


@pytest.mark.parametrize("G", [65, 129])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_whole_trees_in_a_pool_that_overflows(dtype, G):
    over = _whole_trees("counting", dtype, G, False, OVERFLOW_CAPACITY, OVERFLOW_CAPACITY)
    assert over.any() and not over.all()


# ---------------------------------------------------------------- general weights
def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("G", [65, 129])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("weights", ["shipped", "1234"])
def test_general_weights_with_the_model_fed_by_evaluate(weights, dtype, G):
    """Select and the fused call by hand, asking for leaf_value / leaf_probs; the same leaves through qttt_evaluate; the
    two agree with ==, NaN rows (leaves with no legal action) included, and the model backs evaluate's rows up."""
    net = _device_net(weights, dtype)
    arrays = _prefix(_pool(), G)
    t, env = _search(arrays, CAPACITY, net, leaf_eval="value")
    m = ValueTreeModel(1, seed=SEED, board_offset=OFFSET)
    m.reset(boards(arrays))
    value = torch.empty(G, dtype=torch.float32, device=DEV)
    probs = torch.empty((G, 36), dtype=torch.float32, device=DEV)
    nan_rows = 0
    for k in range(24):
        leaves = m.select()
        value.fill_(7.0)
        probs.fill_(7.0)
        t._call("qttt_tree_select", t.tree.data_ptr(), G, t.capacity, t.seed, k, t.board_offset, t.c_puct,
                t.leaf.state.data_ptr())
        t._call("qttt_tree_value_rollout", t.tree.data_ptr(), G, t.capacity, t.leaf.state.data_ptr(), net.blob.data_ptr(),
                net.precision, value.data_ptr(), probs.data_ptr())
        ex = export(t.leaf)
        for key, val in (("board", leaves.board), ("moves", leaves.moves), ("n_moves", leaves.n_moves)):
            assert np.array_equal(ex[key], val), (key, k)
        ev = t.leaf.evaluate(net, rows=("value", "probs"))
        ev_v, ev_p = ev["value"].cpu().numpy(), ev["probs"].cpu().numpy()
        assert np.array_equal(_bits(value.cpu().numpy()), _bits(ev_v)), k
        assert np.array_equal(_bits(probs.cpu().numpy()), _bits(ev_p)), k
        nan_rows += int(np.isnan(ev_p).all(1).sum())
        m.backup(ev_v, ev_p)
        if k in (0, 1, 7, 23):
            _check(t, m)
    assert nan_rows > 0 and m.ends["fresh"] > 0 and len(m.ends["terminal"]) == 6


# ---------------------------------------------------------------- the modes
def test_value_mode_ignores_num_simulations():
    net = _device_net("shipped", "f32")
    arrays = _prefix(_pool(), 65)
    trees = []
    for S in (1, 10):
        t, _ = _search(arrays, 41, net, S=S, leaf_eval="value")
        t.contemplate(20)
        trees.append(t.tree.clone())
    assert torch.equal(trees[0], trees[1])
    t, _ = _search(arrays, 41, net, S=10 ** 6, leaf_eval="value")          # not even its range is looked at
    t.contemplate(20)
    assert torch.equal(t.tree, trees[0])


def test_the_default_mode_is_untouched():
    net = _device_net("shipped", "f32")
    arrays = _prefix(_pool(), 65)
    trees = []
    for kw in ({}, {"leaf_eval": "playouts"}):
        t, _ = _search(arrays, 25, net, S=2, **kw)
        assert t.leaf_eval == "playouts" and set(t._out) == {"result", "probs"}
        t.contemplate(12)
        trees.append(t.tree.clone())
    assert torch.equal(trees[0], trees[1])
    t, _ = _search(arrays, 25, net, S=2, leaf_eval="value")
    t.contemplate(12)
    assert not torch.equal(t.tree, trees[0])


# ---------------------------------------------------------------- a NaN weight
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_a_nan_weight_gives_nan_in_w_and_the_launch_returns(dtype):
    sd = R.golden_state_dict(R.load_golden())
    sd["V_head.1.bias"] = torch.tensor([float("nan")])
    net = PolicyValueNet(sd, device=DEV, dtype=DTYPES[dtype])
    G = 65
    t, _ = _search(_prefix(_pool(), G), 13, net, leaf_eval="value")
    t.contemplate(2)                             # the roots get their priors, then every open root one child
    torch.cuda.synchronize()
    ref_value = R.forward_reference32(sd, t.leaf.encode(with_mask=False).cpu())[0].numpy()
    assert np.isnan(ref_value).all()             # torch's forward: a NaN value for every leaf
    games, nodes, _, _ = tree_layout.decode(t.tree.cpu().numpy(), G, t.capacity)
    nan_edges = finite_edges = 0
    for g in range(G):
        depth = int(games["depth"][g])
        assert depth <= 1
        if depth == 0:
            continue
        W = nodes[g, games["path_node"][g, 0]]["slots"]["W"][games["path_action"][g, 0]]
        if games["flags"][g] & tree_layout.GAME_LEAF_TERMINAL:
            assert W in (-1.0, 0.0, 1.0), g       # a terminal leaf: the reward, the network is not consulted
            finite_edges += 1
        else:
            assert np.isnan(W), g
            nan_edges += 1
    assert nan_edges > 0 and finite_edges > 0
    t.contemplate(4)                             # selects over NaN scores: bounded all the same
    torch.cuda.synchronize()
    assert int(t.root_stats()["Ntot"].max()) == 5


# ---------------------------------------------------------------- SelfPlay
@pytest.mark.parametrize("G", [3, 65])
def test_selfplay_with_value_leaves_matches_the_model(G, monkeypatch):
    R_, seed = 8, 7
    sp = SelfPlay(G, n_rollouts=R_, num_simulations=10, net=_device_net("sharp", "f32"), seed=seed, device=DEV,
                  leaf_eval="value")
    assert sp.capacity == 1 + 10 * (2 * R_ + 1)
    batch = sp.play()
    assert sp.tree.leaf_eval == "value"
    dev = {k: getattr(batch, k).cpu().numpy() for k in ("pi", "mask", "done", "v", "action36", "length", "winner", "actions")}
    monkeypatch.setattr(tree_model, "TreeModel", ValueTreeModel)           # selfplay_model.play builds its tree by this name
    ref, ref_env = selfplay_model.play(G, R_, 1, seed=seed, net=NETS["sharp"]())
    for k, d in dev.items():
        a, b = np.ascontiguousarray(d), np.ascontiguousarray(ref[k])
        if a.dtype.kind == "f":
            a, b = a.view("u%d" % a.dtype.itemsize), b.view("u%d" % b.dtype.itemsize)
        assert np.array_equal(a, b), (k, np.argwhere(a != b)[:6])          # pi with == at alpha = 1
    words = batch.states.cpu().numpy().view(np.uint64).reshape(10, 2, -1)[:, :, :G]
    for row in range(10):
        live = [g for g in range(G) if ref["recs"][row][g] is not None]
        if live:
            P, Q = tree_layout.pack_positions([ref["recs"][row][g] for g in live], DEV)
            assert np.array_equal(words[row, 0, live], P) and np.array_equal(words[row, 1, live], Q), row
    ex = export(sp.env)
    assert np.array_equal(ex["board"], ref_env.board) and np.array_equal(ex["n_moves"], ref_env.n_moves)


# ---------------------------------------------------------------- games == 0
def test_no_games_is_accepted():
    net = _device_net("shipped", "f32")
    t = TreeSearch(0, capacity=8, net=net, device=DEV, leaf_eval="value")
    t.reset(VecEnv(0, device=DEV))
    t.contemplate(3)
    assert t.rollout_idx == 3 and t.root_stats()["N"].shape == (0, 36)
    assert SelfPlay(0, n_rollouts=2, net=net, device=DEV, leaf_eval="value").play().length.numel() == 0
