"""qttt_tree_compact / TreeSearch.compact on the MI355X: the compacted buffer compared node by node with the Python
model of the renumbering (TreeModel.compact, tests/tree_model.py), full games in which a tree that compacts after
every move computes bit for bit what a tree eight times its size computes without compacting, and the edges (straight
after reset, twice, a game that did not move, a fresh root, a set overflow flag, no games, a collapse pair, the host's
bound).

Every test owns its tree buffer (tree_harness.search), filled with a sentinel byte before qttt_tree_reset; what lies at
or beyond `used` is unspecified after a compaction and is not compared, the headers' padding and the bytes after the
tree are."""
import numpy as np
import pytest
import torch

import tree_layout
import tree_model
from tree_harness import (DEV, SENTINEL, assert_stats_equal, boards, export, move, rollout, search, stats,
                          two_plies_in)
from tree_harness import net as _net

pytestmark = pytest.mark.gpu
STAT_KEYS = ("N", "W", "Q", "P", "Ntot", "choose")


# ---------------------------------------------------------------- helpers
def _plan_moves(m, stay=(), special=True):
    """One move per game from the model's trees: the action and collapse bit whose child holds the largest subtree,
    preferring one with a collapse pair in it.  With `special`, game 0 plays choose() instead and game 1 an action
    never expanded (a fresh root).  Games in `stay`, finished games and games without an expanded action do not move
    (255)."""
    act, bits = np.full(len(m.games), 255, dtype=np.uint8), np.zeros(len(m.games), dtype=np.uint8)
    for g, st in enumerate(m.games):
        root = st["nodes"][st["root"]]
        if g in stay or root.terminal or not root.legal:
            continue
        bare = [a for a in root.legal if not root.children[a]]
        if special and g == 0:
            act[g] = tree_model.choose(root)
            continue
        if special and g == 1 and bare:
            act[g] = bare[-1]
            continue
        best = None
        for a in root.legal:
            for b, c in enumerate(root.children[a] or ()):
                sub = tree_model.reachable({"nodes": st["nodes"], "root": c})
                pair = any(len(k or ()) == 2 for i in sub for k in st["nodes"][i].children)
                if best is None or (pair, len(sub)) > best[0]:
                    best = ((pair, len(sub)), a, b)
        if best is not None:
            act[g], bits[g] = best[1], best[2]
    return act, bits


def _check(t, m):
    n = tree_layout.assert_tree_equals_model(t.tree.cpu().numpy(), t.num_games, t.capacity, m, SENTINEL, DEV,
                                             compacted=True)
    assert_stats_equal(stats(t), m.root_stats(), STAT_KEYS + ("nodes_used", "overflow"))
    return n


def _live_bytes(t):
    """The bytes of the tree buffer that mean something: the game headers, and per game the node records and priors
    rows below `used`."""
    buf = t.tree.cpu().numpy()
    games, nodes, priors, _ = tree_layout.decode(buf, t.num_games, t.capacity)
    live = np.arange(t.capacity)[None, :] < games["used"][:, None]
    return games.tobytes(), nodes[live].tobytes(), priors[live].tobytes()


# ---------------------------------------------------------------- (1) every node
@pytest.mark.parametrize("network", [False, True])
def test_every_node_of_the_compacted_trees_equals_the_model(network):
    G, capacity, S, R = 5, 96, 4, 24
    t, m, env = search(two_plies_in(G, 31), capacity, S, net=_net(torch.float32) if network else None)
    for _ in range(R):
        rollout(t, m)
    act, bits = _plan_moves(m, stay=(4,))
    move(t, m, env, act, bits)
    before = m.root_stats()
    kept = m.reachable_counts()
    t.compact()
    m.compact()
    assert t._bound == int(kept.max())
    network_rows = _check(t, m)
    assert (network_rows > 0) == network
    st = stats(t)
    assert np.array_equal(st["nodes_used"], kept)
    assert kept[4] == before["nodes_used"][4] and act[4] == 255     # the game that did not move keeps every node
    assert (kept[:4] < before["nodes_used"][:4]).all()              # the others give nodes back
    if not network:                                                 # (the uniform trees are known from the model alone)
        assert kept[1] == 1                                         # a fresh root: one node
        assert kept.max() > 3                                       # and real subtrees were kept
    # the search goes on, in lockstep with the model, on the compacted trees: another move's rollouts, a move, a
    # compaction of trees that hold carried nodes and new ones
    for _ in range(R):
        rollout(t, m)
    _check(t, m)
    act, bits = _plan_moves(m)
    move(t, m, env, act, bits)
    t.compact()
    m.compact()
    _check(t, m)
    assert not st["overflow"].any()


# ---------------------------------------------------------------- (2) the search does not notice
def test_full_games_compacting_after_every_move_equal_full_games_that_never_compact():
    """Tree A (capacity 1 024) never compacts; tree B (capacity 160) compacts after every sync; 32 rollouts per move,
    so B needs the carried subtree + 2 * 32 new nodes + 1 for the sync.  A tree of B's capacity that does not
    compact cannot finish the game: its host bound refuses the third move's rollouts (1 + 2 * (64 + 1) + 64 > 160)."""
    from qtttgym_amd import TreeSearch, VecEnv
    from qtttgym_amd.actions import action36_to_pairs
    G, S, R, seed = 8, 4, 32, 13
    env = VecEnv(G, device=DEV, seed=seed)
    A = TreeSearch(G, capacity=1024, num_simulations=S, seed=seed, board_offset=2, device=DEV)
    B = TreeSearch(G, capacity=160, num_simulations=S, seed=seed, board_offset=2, device=DEV)
    C = TreeSearch(G, capacity=160, num_simulations=S, seed=seed, board_offset=2, device=DEV)
    for t in (A, B, C):
        t.reset(env)
    done = torch.zeros(G, dtype=torch.bool, device=DEV)
    refused_at = None
    moves = 0
    gave_back = 0
    while moves < 9 and not bool(done.all()):
        A.contemplate(R)
        assert B._bound + 2 * R + 1 <= B.capacity, (moves, B._bound)
        B.contemplate(R)
        if refused_at is None:
            try:
                C.contemplate(R)
            except ValueError:
                refused_at = moves
        sa, sb = A.root_stats(), B.root_stats()
        for k in STAT_KEYS:
            assert torch.equal(sa[k], sb[k]), (k, moves)
        assert not sa["overflow"].any() and not sb["overflow"].any()
        act = torch.where(done, torch.full_like(sa["choose"], 255), sa["choose"])
        bits = torch.as_tensor(((np.arange(G) + moves) % 2).astype(np.uint8), device=DEV)
        _, term = env.step_raw(action36_to_pairs(act).contiguous(), bits)
        done |= term
        A.sync(env)
        B.sync(env)
        if refused_at is None:
            C.sync(env)
        B.compact()
        sa, sb = A.root_stats(), B.root_stats()
        for k in STAT_KEYS:
            assert torch.equal(sa[k], sb[k]), (k, moves)
        assert not sa["overflow"].any() and not sb["overflow"].any()
        assert bool((sb["nodes_used"] <= sa["nodes_used"]).all())
        gave_back += int((sa["nodes_used"] - sb["nodes_used"]).sum())
        assert B._bound == int(sb["nodes_used"].max())
        moves += 1
    assert moves >= 5 and gave_back > 0
    assert refused_at is not None and refused_at < moves, refused_at
    assert int(A.nodes_used().max()) > B.capacity                 # the games did need more than B's pool without compaction


# ---------------------------------------------------------------- (3) edges
def test_compact_straight_after_reset_and_twice():
    G, S = 5, 4
    t, m, env = search(two_plies_in(G, 32), 96, S)
    snap = t.tree.cpu().numpy().copy()
    t.compact()
    assert np.array_equal(t.tree.cpu().numpy(), snap)               # 1 node per game: not a byte changes
    assert (stats(t)["nodes_used"] == 1).all() and t._bound == 1
    for _ in range(24):
        rollout(t, m)
    snap = t.tree.cpu().numpy().copy()
    t.compact()                                                     # no game moved: compact already, the path stays
    assert np.array_equal(t.tree.cpu().numpy(), snap)
    _check(t, m)
    act, bits = _plan_moves(m)
    move(t, m, env, act, bits)
    t.compact()
    m.compact()
    _check(t, m)
    live = _live_bytes(t)
    t.compact()                                                     # twice: no byte below `used` changes
    assert _live_bytes(t) == live
    _check(t, m)


def test_a_kept_subtree_with_a_collapse_pair_keeps_it_adjacent_with_bit_30():
    G, S = 5, 4
    t, m, env = search(two_plies_in(G, 33), 96, S, seed=9, offset=4)
    for _ in range(40):
        rollout(t, m)
    act, bits = _plan_moves(m, special=False)
    move(t, m, env, act, bits)
    t.compact()
    m.compact()
    _check(t, m)
    games, nodes, _, _ = tree_layout.decode(t.tree.cpu().numpy(), G, t.capacity)
    pairs = 0
    for g in range(G):
        child = nodes[g, :games["used"][g]]["slots"]["child"]
        idx = np.arange(games["used"][g])[:, None]
        c0 = child & (tree_layout.CHILD_PAIR - 1)
        n = np.where(child & tree_layout.CHILD_PAIR, 2, 1)
        assert ((child < 0) | ((c0 > idx) & (c0 + n <= games["used"][g]))).all()       # above the parent, below `used`
        pairs += int(((child >= 0) & (child & tree_layout.CHILD_PAIR != 0)).sum())
        spans = sorted((int(a), int(a + b)) for a, b in zip(c0[child >= 0], n[child >= 0]))
        assert spans == [] or (spans[0][0] == 1 and all(x[1] == y[0] for x, y in zip(spans, spans[1:]))
                               and spans[-1][1] == games["used"][g])                 # every node but the root: one parent
    assert pairs > 0


def test_a_set_overflow_flag_outlives_the_compaction():
    G, S, capacity = 5, 2, 8
    t, m, env = search(two_plies_in(G, 34), capacity, S, seed=8, offset=1, model_capacity=capacity)
    for _ in range(16):
        rollout(t, m, bounded=False)               # the pool is too small: the well-defined overflow flag is set
    flagged = stats(t)["overflow"].copy()
    assert flagged.any()
    act, bits = _plan_moves(m, special=False)       # onto expanded children: a full pool could not hold a fresh root
    from qtttgym_amd.actions import action36_to_pairs
    env.step_raw(action36_to_pairs(torch.as_tensor(act, device=DEV)).contiguous(), torch.as_tensor(bits, device=DEV))
    t._call("qttt_tree_sync", t.tree.data_ptr(), G, capacity, env.state.data_ptr())        # TreeSearch.sync less its bound
    m.sync(boards(export(env)))
    t.compact()
    m.compact()
    _check(t, m)
    st = stats(t)
    assert np.array_equal(st["overflow"], flagged)
    assert (st["nodes_used"] < capacity).all()


def test_no_games_and_the_bound_without_a_read_back(monkeypatch):
    from qtttgym_amd import TreeSearch
    t = TreeSearch(0, capacity=8, device=DEV)
    t._bound = 1                                    # as reset() leaves it; there is no board to reset from
    t.compact()
    assert t._bound == 1
    assert t._lib.qttt_tree_compact(None, 0, 8, None, None) == 0
    t, m, env = search(two_plies_in(5, 35), 96, 4)
    t.contemplate(10)
    bound = t._bound
    monkeypatch.setattr(t, "_root", lambda **kw: pytest.fail("update_bound=False must not read anything back"))
    t.compact(update_bound=False)
    assert t._bound == bound == 21 and t.rollout_idx == 10
    with pytest.raises(RuntimeError, match="reset"):
        TreeSearch(5, capacity=8, device=DEV).compact()
