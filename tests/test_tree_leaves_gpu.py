"""Leaf-parallel rounds (include/qttt_tree_leaves.h, TreeSearch(leaf_eval="value", leaves=K)) on the MI355X: whole trees
bit for bit against tests/leaf_parallel_model.py under the exact networks, in both precisions, at G = 1, 3 and 65 and
K = 1, 2, 5 and 8, through a move, a sync and a compaction, and in a pool small enough to overflow; rounds in lockstep
with the model under general weights (the path records, the leaf rows, the in-flight bits in the middle of a round and
their absence after it); rounds of one against today's rollout, byte for byte; the path that qttt_tree_select leaves
in the game header against the record of a round of one; a NaN weight; the argument errors;
SelfPlay; the defaults.

The model's trees are computed once per (network, K, pool capacity) for the 65-game pool and shared: games are
independent, so the first G games of that model are the model of the G-game pool."""
import copy
import functools

import numpy as np
import pytest
import torch

import leaf_parallel_model as LP
import nn_reference64 as R
import selfplay_model
import tree_layout
import tree_model
from tree_harness import DEV, SENTINEL, TAIL, boards, env_from_arrays, export
from value_tree_model import OVERFLOW_CAPACITY, ValueTreeModel

from qtttgym_amd import PolicyValueNet, SelfPlay, TreeSearch, _native
from qtttgym_amd.actions import action36_to_pairs

pytestmark = pytest.mark.gpu
SEED, OFFSET, G_MAX = LP.SEED, LP.OFFSET, 65
NETS = {"zero": R.zero_state_dict, "greedy": R.greedy_state_dict, "counting": R.counting_state_dict,
        "sharp": R.sharp_counting_state_dict}
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
ERR_NULL, ERR_SIZE, ERR_ACTION = -1, -2, -3


def _capacity(K):
    return 1 + 2 * LP.first_rollouts(K) + 1 + 2 * LP.second_rollouts(K)


def _prefix(arrays, G):
    return {k: np.asarray(v)[:G] for k, v in arrays.items()}


@functools.lru_cache(maxsize=None)
def _pool():
    return LP.root_pool(G_MAX)


@functools.lru_cache(maxsize=None)
def _device_net(name, dtype):
    sd = NETS[name]() if name in NETS else (R.golden_state_dict(R.load_golden()) if name == "shipped"
                                             else R.random_state_dict(int(name)))
    return PolicyValueNet(sd, device=DEV, dtype=DTYPES[dtype])


def _evaluate_probs(leaves):
    """qttt_evaluate's f32 probs of positions given as OracleBoards, under the counting network."""
    env = env_from_arrays({"board": leaves.board, "moves": leaves.moves, "n_moves": leaves.n_moves, "qmask": leaves.qmask,
                           "n_q": leaves.n_q})
    return env.evaluate(_device_net("counting", "f32"), rows=("probs",))["probs"].cpu().numpy()


@functools.lru_cache(maxsize=None)
def _model_stages(net, K, capacity):
    # the counting network: exact value and logits, but the softmax of its logits is the device's expf
    return LP.model_stages(NETS[net](), K, capacity, G_MAX, probs_of=_evaluate_probs if net == "counting" else None)


def _view(m, G):
    v = copy.copy(m)
    v.games = m.games[:G]
    return v


def _search(arrays, capacity, net, **kw):
    """A value search over a sentinel-filled buffer of the test's own, with a tail, as tree_harness.search makes."""
    env = env_from_arrays(arrays)
    G = env.num_envs
    t = TreeSearch(G, capacity=capacity, net=net, seed=SEED, board_offset=OFFSET, device=DEV, leaf_eval="value", **kw)
    t.tree = torch.full((tree_layout.tree_bytes(G, capacity) + TAIL,), SENTINEL, dtype=torch.uint8, device=DEV)
    t.reset(env)
    return t, env


def _check(t, m, compacted=False):
    return tree_layout.assert_tree_equals_model(t.tree.cpu().numpy(), t.num_games, t.capacity, m, SENTINEL, DEV,
                                                compacted=compacted)


def _contemplate(t, r, K, bounded):
    """TreeSearch.contemplate's schedule.  bounded and K > 1: contemplate itself.  Otherwise the same launches through
    _rollout() and _round(): without the host's node bound in the pool that overflows, and at K = 1, where contemplate
    keeps today's path, so that the new kernels run at K = 1 too."""
    if bounded and K > 1:
        assert t.leaves == K
        return t.contemplate(r)
    if r and t._fresh:
        t._rollout()
        r -= 1
        t._fresh = False
    for k in [K] * (r // K) + [r % K] * (r % K > 0):
        t._round(k)


def _no_bits_in_flight(t):
    """No N or Ntot word of a used record has a bit at or above 24."""
    games, nodes, _, _ = tree_layout.decode(t.tree.cpu().numpy(), t.num_games, t.capacity)
    live = np.arange(t.capacity)[None, :] < games["used"][:, None]
    assert (nodes[live]["slots"]["N"] < 1 << 24).all() and (nodes[live]["Ntot"] < 1 << 24).all()


# ---------------------------------------------------------------- whole trees under the exact networks
def _whole_trees(net, dtype, G, K, compact, capacity, model_capacity):
    stages, act, bits = _model_stages(net, K, model_capacity)
    bounded = model_capacity is None
    t, env = _search(_prefix(_pool(), G), capacity, _device_net(net, dtype), leaves=K)
    _contemplate(t, LP.first_rollouts(K), K, bounded)
    assert t.rollout_idx == LP.first_rollouts(K)
    _check(t, _view(stages["first"], G))                  # W with ==, N and Ntot as raw words: no bit in flight
    env.step_raw(action36_to_pairs(torch.as_tensor(act[:G], device=DEV)).contiguous(), torch.as_tensor(bits[:G], device=DEV))
    if bounded:
        t.sync(env)
    else:
        t._call("qttt_tree_sync", t.tree.data_ptr(), G, capacity, env.state.data_ptr())
        t._fresh = True
    _check(t, _view(stages["synced"], G))
    if compact:
        t.compact()
    _contemplate(t, LP.second_rollouts(K), K, bounded)
    final = _view(stages["second", compact], G)
    _check(t, final, compacted=compact)
    assert t.rollout_idx == LP.first_rollouts(K) + LP.second_rollouts(K)
    if bounded and K > 1:                                 # (at K = 1 _contemplate goes round the host's bound)
        assert t._bound >= int(t.nodes_used().max())
    over = np.array([d["overflow"] for d in final.dump()])
    assert np.array_equal(t.root_stats()["overflow"].cpu().numpy(), over)
    return over


@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("K", LP.LEAVES)
@pytest.mark.parametrize("G", [1, 3, 65])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("net", list(NETS))
def test_whole_trees_match_the_model_bit_for_bit(net, dtype, G, K, compact):
    assert not _whole_trees(net, dtype, G, K, compact, _capacity(K), None).any()


@pytest.mark.parametrize("K", LP.LEAVES)
@pytest.mark.parametrize("G", [3, 65])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("net", ["counting", "sharp"])
def test_whole_trees_in_a_pool_that_overflows(net, dtype, G, K):
    over = _whole_trees(net, dtype, G, K, False, OVERFLOW_CAPACITY, OVERFLOW_CAPACITY)
    assert G < G_MAX or (over.any() and not over.all())


# ---------------------------------------------------------------- general weights: rounds in lockstep with the model
def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("K", [2, 5, 8])
@pytest.mark.parametrize("G", [3, 65])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("weights", ["shipped", "1234"])
def test_rounds_in_lockstep_with_the_model_fed_by_evaluate(weights, dtype, G, K):
    """Per round: the path records and the leaf rows equal the model's, duplicates included; between the two tree
    launches N and Ntot hold the model's in-flight counts in bits 24-31; the model backs up the device's own
    leaf.evaluate(net) rows; afterwards no word has a bit at or above 24 and the whole trees are equal."""
    net = _device_net(weights, dtype)
    arrays = _prefix(_pool(), G)
    rounds = 5
    t, env = _search(arrays, 1 + 2 * (1 + rounds * K), net, leaves=K)
    m = LP.LeafParallelModel(1, seed=SEED, board_offset=OFFSET, leaves=K)
    m.reset(boards(arrays))
    leaves = m.select()                                        # the single rollout
    t._rollout()
    ev = t.leaf.evaluate(net, rows=("value", "probs"))
    m.backup(ev["value"].cpu().numpy(), ev["probs"].cpu().numpy())
    _check(t, m)
    b = t._round_buffers(K)
    duplicates = 0
    for r in range(rounds):
        leaves = m.select_batch(K, t.virtual_loss)
        t._call("qttt_tree_select_batch", t.tree.data_ptr(), G, t.capacity, t.seed, t.rollout_idx, K, t.board_offset, t.c_puct,
                t.virtual_loss, b["paths"].data_ptr(), b["leaf"].state.data_ptr())
        ex = export(b["leaf"])
        for key, val in (("board", leaves.board), ("moves", leaves.moves), ("n_moves", leaves.n_moves)):
            assert np.array_equal(ex[key], val), (key, r)
        got = b["paths"].cpu().numpy()[:G * K * LP.PATH_BYTES].view(LP.PATH_DTYPE).reshape(G, K)
        ref = m.records()
        for f in ("leaf", "depth", "flags"):
            assert np.array_equal(got[f], ref[f]), (f, r)
        on = np.arange(10)[None, None, :] < ref["depth"][:, :, None]
        assert np.array_equal(got["node"][on], ref["node"][on]) and np.array_equal(got["action"][on], ref["action"][on]), r
        duplicates += sum(len(set(row)) < K for row in ref["leaf"].tolist())
        # the middle of the round: counts | in flight << 24
        games, nodes, _, _ = tree_layout.decode(t.tree.cpu().numpy(), G, t.capacity)
        for g, words in enumerate(m.raw_words()):
            assert games["used"][g] == len(words) and games["depth"][g] == 0 and games["leaf"][g] == games["root"][g]
            assert np.array_equal(nodes[g, :len(words)]["slots"]["N"], np.array([w[0] for w in words], dtype=np.uint32)), (g, r)
            assert np.array_equal(nodes[g, :len(words)]["Ntot"], np.array([w[1] for w in words], dtype=np.uint32)), (g, r)
        ev = b["leaf"].evaluate(net, out=b["out"])
        t._call("qttt_tree_backup_batch", t.tree.data_ptr(), G, t.capacity, K, b["paths"].data_ptr(),
                ev["value"].data_ptr(), ev["probs"].data_ptr())
        t.rollout_idx += K
        m.backup_batch(ev["value"].cpu().numpy(), ev["probs"].cpu().numpy())
        _no_bits_in_flight(t)
        _check(t, m)
    assert m.in_flight() == 0 and (duplicates > 0 or G < G_MAX)


# ---------------------------------------------------------------- rounds of one are today's rollouts
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_rounds_of_one_leave_the_bytes_that_rollouts_leave(dtype):
    """40 x _round(1) against 40 x _rollout() under the shipped weights: over the used records the tree buffers are byte
    for byte the same, which holds with real weights because W is never perturbed.  (The game headers' recorded path is
    what differs: a round leaves it as a compaction does.)"""
    net = _device_net("shipped", dtype)
    G, n = 65, 40
    arrays = _prefix(_pool(), G)
    a, _ = _search(arrays, 1 + 2 * n, net)
    b, _ = _search(arrays, 1 + 2 * n, net)
    for _ in range(n):
        a._rollout()
        b._round(1)
    ga, na, pa, _ = tree_layout.decode(a.tree.cpu().numpy(), G, a.capacity)
    gb, nb, pb, _ = tree_layout.decode(b.tree.cpu().numpy(), G, b.capacity)
    assert np.array_equal(ga["used"], gb["used"]) and np.array_equal(ga["root"], gb["root"]) and ga["used"].max() > 20
    assert np.array_equal(ga["flags"] & 1, gb["flags"] & 1) and (gb["depth"] == 0).all()
    live = np.arange(a.capacity)[None, :] < ga["used"][:, None]
    assert np.array_equal(na[live].view(np.uint8), nb[live].view(np.uint8))
    assert np.array_equal(pa[live].view(np.uint8), pb[live].view(np.uint8))


# ---------------------------------------------------------------- the header's path is the record's path
PATH_SEED, PATH_POOL_FIRST = 6, 3      # roots 5, 6 and 8 plies deep first; under this seed the model's 13th select goes three
#                                        edges deep in games 0 and 1 and expands a pair in game 0 (tests/value_tree_model.py)


@pytest.mark.parametrize("G", [1, 3, 65])
def test_select_leaves_the_path_in_the_header_that_a_round_of_one_records(G):
    """qttt_tree_select and qttt_tree_select_batch(leaves = 1) on two copies of one tree, 12 value rollouts in: the game
    header's depth, leaf and path entries below depth are the record's, the entries at and past depth keep the bytes they
    had, the leaf states are equal and so are the pools over the used records."""
    net, cap = _device_net("sharp", "f32"), 64
    pool = LP.root_pool(PATH_POOL_FIRST + G)
    env = env_from_arrays({k: np.asarray(v)[PATH_POOL_FIRST:] for k, v in pool.items()})
    t = TreeSearch(G, capacity=cap, net=net, seed=PATH_SEED, board_offset=OFFSET, device=DEV, leaf_eval="value")
    t.tree = torch.full((tree_layout.tree_bytes(G, cap) + TAIL,), SENTINEL, dtype=torch.uint8, device=DEV)
    t.reset(env)
    t.contemplate(12)
    before, other = t.tree.clone(), t.tree.clone()
    b = t._round_buffers(1)
    t._call("qttt_tree_select", t.tree.data_ptr(), G, cap, t.seed, t.rollout_idx, t.board_offset, t.c_puct,
            t.leaf.state.data_ptr())
    t._call("qttt_tree_select_batch", other.data_ptr(), G, cap, t.seed, t.rollout_idx, 1, t.board_offset, t.c_puct,
            t.virtual_loss, b["paths"].data_ptr(), b["leaf"].state.data_ptr())
    g0, _, _, _ = tree_layout.decode(before.cpu().numpy(), G, cap)
    ga, na, pa, tail_a = tree_layout.decode(t.tree.cpu().numpy(), G, cap)
    gb, nb, pb, tail_b = tree_layout.decode(other.cpu().numpy(), G, cap)
    rec = b["paths"].cpu().numpy()[:G * LP.PATH_BYTES].view(LP.PATH_DTYPE)
    assert np.array_equal(ga["depth"], rec["depth"]) and np.array_equal(ga["leaf"], rec["leaf"])
    on = np.arange(10)[None, :] < ga["depth"][:, None]
    assert np.array_equal(ga["path_node"][on], rec["node"][on]) and np.array_equal(ga["path_action"][on], rec["action"][on])
    assert np.array_equal(ga["path_node"][~on], g0["path_node"][~on])
    assert np.array_equal(ga["path_action"][~on], g0["path_action"][~on])
    assert torch.equal(t.leaf.state, b["leaf"].state)
    assert np.array_equal(ga["used"], gb["used"]) and np.array_equal(ga["flags"] & 1, gb["flags"] & 1)
    live = np.arange(cap)[None, :] < ga["used"][:, None]
    marked = na.copy()                           # the round's copy holds one visit in flight on every edge of its path
    for g in range(G):
        for d in range(int(rec["depth"][g])):
            marked["slots"]["N"][g, rec["node"][g, d], rec["action"][g, d]] += 1 << LP.FLIGHT_SHIFT
            marked["Ntot"][g, rec["node"][g, d]] += 1 << LP.FLIGHT_SHIFT
    assert np.array_equal(marked[live].view(np.uint8), nb[live].view(np.uint8))
    assert np.array_equal(pa[live].view(np.uint8), pb[live].view(np.uint8))
    assert (tail_a == SENTINEL).all() and (tail_b == SENTINEL).all()
    assert ga["depth"].max() >= 3 and (ga["used"] > g0["used"]).any()          # the floor: a deep path, an expansion


# ---------------------------------------------------------------- a NaN weight
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_a_nan_weight_gives_nan_in_w_and_the_launches_return(dtype):
    sd = R.golden_state_dict(R.load_golden())
    sd["V_head.1.bias"] = torch.tensor([float("nan")])
    net = PolicyValueNet(sd, device=DEV, dtype=DTYPES[dtype])
    G, K = 65, 4
    t, _ = _search(_prefix(_pool(), G), 1 + 2 * (2 + 2 * K), net, leaves=K)
    t.contemplate(2)                             # the roots get their priors, then a short round of one descent
    torch.cuda.synchronize()
    recs = t._rounds[1]["paths"].cpu().numpy()[:G * LP.PATH_BYTES].view(LP.PATH_DTYPE)
    _, nodes, _, _ = tree_layout.decode(t.tree.cpu().numpy(), G, t.capacity)
    nan_edges = finite_edges = 0
    for g in range(G):
        depth = int(recs["depth"][g])
        assert depth <= 1
        if depth == 0:
            continue
        W = nodes[g, recs["node"][g, 0]]["slots"]["W"][recs["action"][g, 0]]
        if recs["flags"][g] & LP.REC_LEAF_TERMINAL:
            assert W in (-1.0, 0.0, 1.0), g       # a terminal leaf: the reward, the network is not consulted
            finite_edges += 1
        else:
            assert np.isnan(W), g
            nan_edges += 1
    assert nan_edges > 0 and finite_edges > 0
    t.contemplate(2 * K)                         # descents over NaN scores: bounded all the same
    torch.cuda.synchronize()
    assert int(t.root_stats()["Ntot"].max()) == 2 * K + 1
    _no_bits_in_flight(t)


# ---------------------------------------------------------------- argument errors
def _select(L, tree=0x1000, games=1, capacity=4, seed=0, idx0=0, leaves=2, offset=0, c_puct=1.0, vloss=1.0, paths=0x2000,
            leaf=0x3000):
    """The entries with fake addresses (never dereferenced: every call here fails its checks first)."""
    return L.qttt_tree_select_batch(tree, games, capacity, seed, idx0, leaves, offset, c_puct, vloss, paths, leaf, None)


def _backup(L, tree=0x1000, games=1, capacity=4, leaves=2, paths=0x2000, value=0x4000, probs=0x5000):
    return L.qttt_tree_backup_batch(tree, games, capacity, leaves, paths, value, probs, None)


def test_return_codes_in_documented_order_without_device_work():
    L = _native.lib()
    assert L.qttt_tree_paths_bytes(5, 8) == 5 * 8 * 64 and L.qttt_tree_paths_bytes(0, 1) == 0
    for games, leaves in ((-1, 2), (4, 0), (4, -1), (4, 65), (1 << 62, 2)):
        assert L.qttt_tree_paths_bytes(games, leaves) == ERR_SIZE, (games, leaves)
    sizes = (dict(games=-1), dict(capacity=0), dict(capacity=(1 << 30) + 1), dict(leaves=0), dict(leaves=65))
    for kw in sizes + (dict(offset=-1), dict(idx0=(1 << 24) - 1), dict(idx0=(1 << 24) - 7, leaves=8), dict(idx0=(1 << 32) - 1),
                       dict(vloss=-1.0), dict(vloss=float("inf")), dict(vloss=float("nan"))):
        assert _select(L, **kw) == ERR_SIZE, kw
        assert _select(L, **{"tree": None, "paths": None, "leaf": None, **kw}) == ERR_SIZE, kw        # sizes before nulls
        assert _select(L, **{"tree": 0x1001, "paths": 0x2001, **kw}) == ERR_SIZE, kw                  # and before alignment
        assert _select(L, **{"games": 0, **kw}) == ERR_SIZE or kw == dict(games=-1), kw               # and before games == 0
    for kw in sizes:
        assert _backup(L, **kw) == ERR_SIZE, kw
        assert _backup(L, **{"tree": None, "paths": None, "value": None, "probs": None, **kw}) == ERR_SIZE, kw
        assert _backup(L, **{"tree": 0x1001, "value": 0x4001, **kw}) == ERR_SIZE, kw
    assert _select(L, idx0=(1 << 24) - 8, leaves=8, tree=None) == ERR_NULL      # the last rollouts there are
    assert _select(L, games=0, tree=None, paths=None, leaf=None) == 0           # nothing to do, no pointer looked at
    assert _select(L, games=0, tree=0x1001, paths=0x2001) == 0
    assert _backup(L, games=0, tree=None, paths=None, value=None, probs=None) == 0
    assert _backup(L, games=0, tree=0x1001, paths=0x2001, value=0x4001, probs=0x5001) == 0
    for kw in (dict(tree=None), dict(paths=None), dict(leaf=None)):
        assert _select(L, **kw) == ERR_NULL, kw
        assert _select(L, **{"tree": 0x1001, "paths": 0x2008, **kw}) == ERR_NULL, kw                  # nulls before alignment
    for kw in (dict(tree=None), dict(paths=None), dict(value=None), dict(probs=None)):
        assert _backup(L, **kw) == ERR_NULL, kw
        assert _backup(L, **{"tree": 0x1001, "paths": 0x2008, "value": 0x4002, "probs": 0x5001, **kw}) == ERR_NULL, kw
    for kw in (dict(tree=0x1008), dict(tree=0x1001), dict(paths=0x2008), dict(paths=0x2004)):
        assert _select(L, **kw) == ERR_ACTION, kw
        assert _backup(L, **kw) == ERR_ACTION, kw
    for kw in (dict(value=0x4002), dict(value=0x4001), dict(probs=0x5002), dict(probs=0x5001)):
        assert _backup(L, **kw) == ERR_ACTION, kw


def test_python_checks_come_before_any_launch():
    net = _device_net("shipped", "f32")
    t, _ = _search(_prefix(_pool(), 3), 9, net, leaves=2)
    before = t.tree.clone()
    with pytest.raises(ValueError, match="capacity"):
        t.contemplate(5)                         # 1 + 2 * 5 nodes do not fit 9
    assert torch.equal(t.tree, before) and t.rollout_idx == 0 and t._fresh
    t.contemplate(4)
    assert t.rollout_idx == 4 and t._bound == 9 and sorted(t._rounds) == [1, 2]
    for k in (0, 65):
        with pytest.raises(ValueError, match="round"):
            t._round(k)
    plain = TreeSearch(3, capacity=9, net=net, device=DEV)
    with pytest.raises(ValueError, match="leaf_eval"):
        plain._round(2)


# ---------------------------------------------------------------- SelfPlay
@pytest.mark.parametrize("G", [3, 65])
def test_selfplay_with_four_leaves_matches_the_model(G, monkeypatch):
    R_, seed, K = 8, 7, 4
    sp = SelfPlay(G, n_rollouts=R_, net=_device_net("sharp", "f32"), seed=seed, device=DEV, leaf_eval="value", leaves=K)
    batch = sp.play()
    assert sp.tree.leaves == K and sp.tree.virtual_loss == 1.0 and sorted(sp.tree._rounds) == [3, 4]
    dev = {k: getattr(batch, k).cpu().numpy() for k in ("pi", "mask", "done", "v", "action36", "length", "winner", "actions")}
    # selfplay_model.play builds its tree by this name and calls rollout() R_ times per move: the model queues them
    monkeypatch.setattr(tree_model, "TreeModel", functools.partial(LP.LeafParallelModel, leaves=K))
    ref, ref_env = selfplay_model.play(G, R_, 1, seed=seed, net=NETS["sharp"]())
    for k, d in dev.items():
        a, b = np.ascontiguousarray(d), np.ascontiguousarray(ref[k])
        if a.dtype.kind == "f":
            a, b = a.view("u%d" % a.dtype.itemsize), b.view("u%d" % b.dtype.itemsize)
        assert np.array_equal(a, b), (k, np.argwhere(a != b)[:6])          # pi with == at alpha = 1
    ex = export(sp.env)
    assert np.array_equal(ex["board"], ref_env.board) and np.array_equal(ex["n_moves"], ref_env.n_moves)


# ---------------------------------------------------------------- the defaults
def test_the_default_search_is_the_search_it_was():
    net = _device_net("sharp", "f32")
    arrays = _prefix(_pool(), G_MAX)
    t, _ = _search(arrays, 25, net)
    assert t.leaves == 1 and t.virtual_loss == 1.0 and TreeSearch(0, capacity=4, device=DEV).leaves == 1
    t.contemplate(12)
    assert t._rounds == {}                       # today's path: no round buffer was made
    m = ValueTreeModel(1, seed=SEED, board_offset=OFFSET, net=NETS["sharp"]())
    m.reset(boards(arrays))
    for _ in range(12):
        m.rollout()
    _check(t, m)
