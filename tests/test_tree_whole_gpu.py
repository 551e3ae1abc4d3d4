"""The device search trees (include/qttt_tree.h) compared whole with the float64 model (tests/tree_model.py) on the
MI355X: the selection score bit for bit at c_puct values where a fused multiply-add would show, every node of every
game after lockstep rollouts (tests/tree_harness.py, tests/tree_layout.py), wide simulation counts and draw indices at
the top of their range, full games through up to nine syncs, and the overflow branches of select and sync.

Every test owns its tree buffer (tree_harness.search): it is filled with a sentinel byte before qttt_tree_reset and ends
in a tail of four node records, so a write outside what the header allows shows as a failed comparison inside the
allocation."""
import fractions
import math

import numpy as np
import pytest
import torch

import oracle
import tree_layout
from tree_harness import (DEV, SENTINEL, assert_stats_equal, boards, export, random_positions, rollout, search, stats)
from tree_harness import net as _net

pytestmark = pytest.mark.gpu
SQRT2 = math.sqrt(2.0)
STAT_KEYS = ("N", "W", "Q", "P", "Ntot", "choose", "nodes_used", "overflow")


# ---------------------------------------------------------------- helpers
def _check_tree(t, m):
    tree_layout.assert_tree_equals_model(t.tree.cpu().numpy(), t.num_games, t.capacity, m, SENTINEL, DEV)


def _check_stats(t, m):
    st = stats(t)
    assert_stats_equal(st, m.root_stats(), STAT_KEYS)
    return st


# ---------------------------------------------------------------- (a) the score, bit for bit
def _score_tuples(n, seed=2026):
    """(W, N, prior, Ntot) shaped like real trees: Ntot < 2^24 (half of them below 4096), N <= min(Ntot, 4095) with one
    row in eight at N = 0, W a multiple of 1 / S in [-N, N], priors half 1 / k (k = 1..36) and half f32 values."""
    rng = np.random.default_rng(seed)
    Ntot = np.where(rng.random(n) < 0.5, rng.integers(0, 4096, n), rng.integers(0, 1 << 24, n)).astype(np.uint32)
    N = (rng.random(n) * (np.minimum(Ntot, 4095) + 1.0)).astype(np.uint32)
    N[rng.random(n) < 0.125] = 0
    S = rng.choice(np.array([1, 3, 4, 10, 64, 128]), n)
    numer = np.rint((rng.random(n) * 2.0 - 1.0) * N * S)
    W = np.clip(numer / S, -1.0 * N, 1.0 * N)
    prior = np.where(rng.random(n) < 0.5, 1.0 / rng.integers(1, 37, n), rng.random(n).astype(np.float32).astype(np.float64))
    return np.ascontiguousarray(W), N, np.ascontiguousarray(prior), Ntot


def _score_reference(W, N, prior, Ntot, c):
    """The reference's score (mcts.py:282-284), one IEEE double operation per step."""
    Nd = N.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(N > 0, W / Nd, 0.0)
    u = prior * np.sqrt(Ntot.astype(np.float64))
    u = u / (1.0 + Nd)
    cu = c * u
    return q, u, q + cu


@pytest.fixture(scope="module")
def score_tuples():
    return _score_tuples(1 << 20)


@pytest.mark.parametrize("c_puct", [1.0, 0.3, SQRT2, 2.5])
def test_select_score_is_the_reference_score_bit_for_bit(score_tuples, c_puct):
    from qtttgym_amd import _native
    W, N, prior, Ntot = score_tuples
    n = len(W)
    q, u, ref = _score_reference(W, N, prior, Ntot, c_puct)
    if c_puct in (0.3, SQRT2):
        # not vacuous: at this c_puct a fused q + c * u (rounded once) is another double in >= 5 % of the tuples
        sub = np.random.default_rng(7).choice(n, 20000, replace=False)
        fc = fractions.Fraction(c_puct)
        fused = np.array([float(fractions.Fraction(float(q[i])) + fc * fractions.Fraction(float(u[i]))) for i in sub])
        differ = np.mean(fused.view(np.int64) != ref[sub].view(np.int64))
        print("c_puct %r: a fused score differs in %.1f %% of the tuples" % (c_puct, 100 * differ))
        assert differ >= 0.05, differ
    d = [torch.as_tensor(x, device=DEV) for x in (W, N.view(np.int32), prior, Ntot.view(np.int32))]
    out = torch.empty(n, dtype=torch.float64, device=DEV)
    rc = _native.lib().qttt_tree_score(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), c_puct, n,
                                       out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    dev = out.cpu().numpy()
    bad = np.nonzero(dev.view(np.int64) != ref.view(np.int64))[0]
    assert bad.size == 0, (bad.size, bad[:4], dev[bad[:4]], ref[bad[:4]], W[bad[:4]], N[bad[:4]], prior[bad[:4]],
                           Ntot[bad[:4]])


# ---------------------------------------------------------------- (b) whole-tree lockstep
@pytest.fixture(scope="module")
def positions_257():
    return random_positions(257, 5)


def _whole_tree_lockstep(arrays, c_puct, net=None, rollouts=48, S=3, checks=(1, 2, 7)):
    t, m, _ = search(arrays, 3 + 2 * rollouts, S, c_puct=c_puct, net=net)
    _check_tree(t, m)
    for r in range(1, rollouts + 1):
        rollout(t, m)
        if r in checks or r == rollouts:
            _check_tree(t, m)
    _check_stats(t, m)
    # more than the roots were compared: interior nodes with visits, and collapse pairs
    dump = m.dump()
    assert any(n["Ntot"] > 0 for d in dump for i, n in enumerate(d["nodes"]) if i != d["root"])
    assert any(len(c) == 2 for d in dump for n in d["nodes"] for c in n["children"])


@pytest.mark.parametrize("c_puct", [1.0, 0.3, SQRT2])
def test_whole_tree_lockstep_uniform_playouts(positions_257, c_puct):
    _whole_tree_lockstep(positions_257, c_puct)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_whole_tree_lockstep_network_playouts(positions_257, dtype):
    _whole_tree_lockstep(positions_257, SQRT2, net=_net(dtype))


# ---------------------------------------------------------------- (c) wide simulations and high indices
@pytest.fixture(scope="module")
def positions_65():
    return random_positions(65, 65)


@pytest.mark.parametrize("S,high", [(64, False), (65, False), (128, False), (64, True), (65, True), (128, True), (1, True)])
def test_wide_simulations_and_draw_indices_at_the_top_of_their_range(positions_65, S, high):
    from qtttgym_amd import _native
    G, R, seed, offset = 65, 6, 11, 3
    t, m, _ = search(positions_65, 3 + 2 * R, S, seed=seed, offset=offset)
    if high:
        t.rollout_idx = m.k = t.max_rollouts - R
        assert t.max_rollouts == min(1 << 24, (1 << 31) // (16 * S))
    for _ in range(R):
        k = m.k
        leaves, result = rollout(t, m)
    # the last rollout's playouts are qttt_rollout_many's at step_idx0 = k * S * 16: a sample against the oracle
    assert not high or (k + 2) * S * _native.SIM_STRIDE > (1 << 31) or k + 1 == (1 << 24)
    for g in (0, 31, 64):
        leaf = oracle.OracleBoards.from_records(leaves.b[g:g + 1])
        ref = [oracle.rollout(leaf, seed, k * S * 16 + s * 16, offset + g)[0][0] for s in range(S)]
        assert np.array_equal(result[g], np.array(ref, dtype=np.int8)), g
    _check_tree(t, m)
    _check_stats(t, m)
    if high:
        with pytest.raises(ValueError):
            t.contemplate(1)


# ---------------------------------------------------------------- (d) full games
@pytest.mark.parametrize("network", [False, True])
def test_full_games_through_every_sync(network):
    from qtttgym_amd import VecEnv
    from qtttgym_amd.actions import action36_to_pairs
    G, R, S = 257, 12, 3
    capacity = 1 + 9 * (2 * R + 1) + 1
    t, m, env = search(export(VecEnv(G, device=DEV)), capacity, S, net=_net(torch.float32) if network else None,
                       seed=13, offset=2)
    env.seed = 4                        # (never drawn from: every step_raw below is given its bits)
    done = torch.zeros(G, dtype=torch.bool, device=DEV)
    onto_child = fresh_root = 0
    moves = 0
    while True:
        roots = [st["nodes"][st["root"]] for st in m.games]
        frozen = np.array([n.terminal or not n.legal for n in roots]) | done.cpu().numpy()
        if frozen.all():
            break
        assert moves < 9
        for _ in range(R):
            rollout(t, m)
        st = _check_stats(t, m)
        assert np.array_equal(t.choose().cpu().numpy(), st["choose"])
        # even games play the chosen action, odd games the least visited legal one (often a child never expanded)
        act = np.full(G, 255, dtype=np.uint8)
        for g, n in enumerate(roots):
            if not frozen[g]:
                act[g] = st["choose"][g] if g % 2 == 0 else min(n.legal, key=lambda a: n.N[a])
        bits = ((np.arange(G) // 2 + moves) % 2).astype(np.uint8)
        _, term = env.step_raw(action36_to_pairs(torch.as_tensor(act, device=DEV)).contiguous(),
                               torch.as_tensor(bits, device=DEV))
        done |= term
        t.sync(env)
        before = [(st_["root"], len(st_["nodes"])) for st_ in m.games]
        m.sync(boards(export(env)))
        for g, st_ in enumerate(m.games):
            if not frozen[g]:
                assert st_["root"] != before[g][0], g
                fresh_root += len(st_["nodes"]) > before[g][1]
                onto_child += len(st_["nodes"]) == before[g][1]
        _check_stats(t, m)
        moves += 1
        if moves == 3:
            _check_tree(t, m)
    _check_tree(t, m)
    assert onto_child > 0 and fresh_root > 0, (onto_child, fresh_root)
    assert not stats(t)["overflow"].any()
    # every game is over: one more rollout selects nothing, expands nothing and backs nothing up (launched without the
    # host-side bound, which nine moves may have used up: it counts two nodes per rollout whatever the games do)
    snap = t.tree.cpu().numpy().copy()
    rollout(t, m, bounded=False)
    o = G * tree_layout.GAME_BYTES
    assert np.array_equal(t.tree.cpu().numpy()[o:], snap[o:])
    _check_tree(t, m)


# ---------------------------------------------------------------- (e) overflow
@pytest.fixture(scope="module")
def positions_130():
    return random_positions(130, 130)


@pytest.mark.parametrize("capacity", [1, 2, 3, 8])
def test_overflow_in_select_and_sync(positions_130, capacity):
    from qtttgym_amd.actions import action36_to_pairs
    G, S, R = 130, 2, 16
    t, m, env = search(positions_130, capacity, S, seed=8, offset=1, model_capacity=capacity)
    for _ in range(R):
        rollout(t, m, bounded=False)
        st = _check_stats(t, m)                     # overflow and nodes_used among them
        assert (st["nodes_used"] <= capacity).all()
        _check_tree(t, m)
    flagged = st["overflow"].copy()
    assert flagged.any()
    # ---- sync: even games onto an expanded root child (when there is one), odd games onto a never-expanded action
    roots = [s["nodes"][s["root"]] for s in m.games]
    act = np.full(G, 255, dtype=np.uint8)
    for g, n in enumerate(roots):
        if n.terminal or not n.legal:
            continue
        grown = [a for a in n.legal if n.children[a]]
        bare = [a for a in n.legal if not n.children[a]]
        act[g] = grown[0] if (g % 2 == 0 and grown) else (bare[-1] if bare else grown[0])
    bits = (np.arange(G) // 2 % 2).astype(np.uint8)
    env.step_raw(action36_to_pairs(torch.as_tensor(act, device=DEV)).contiguous(), torch.as_tensor(bits, device=DEV))
    before = m.dump()
    t._call("qttt_tree_sync", t.tree.data_ptr(), G, capacity, env.state.data_ptr())       # TreeSearch.sync less its bound
    m.sync(boards(export(env)))
    st = _check_stats(t, m)
    _check_tree(t, m)
    after = m.dump()
    no_room = rerooted = 0
    for g, n in enumerate(roots):
        if act[g] == 255:
            continue
        if n.children[act[g]]:                      # an expanded child: re-roots, however full the pool is
            assert after[g]["root"] in n.children[act[g]] and after[g]["used"] == before[g]["used"], g
            assert st["overflow"][g] == flagged[g]
            rerooted += 1
        elif before[g]["used"] == capacity:         # a fresh root that does not fit
            assert st["overflow"][g] and after[g]["root"] == before[g]["root"] and after[g]["used"] == capacity, g
            no_room += 1
        else:
            assert after[g]["root"] == before[g]["used"] and after[g]["used"] == before[g]["used"] + 1, g
    assert no_room > 0 and (rerooted > 0 or capacity < 3), (no_room, rerooted)
    # ---- the flag outlives later selects (above) and a sync; qttt_tree_reset clears it
    t.tree.fill_(SENTINEL)
    t.reset(env)
    m.reset(boards(export(env)))
    assert not _check_stats(t, m)["overflow"].any()
    _check_tree(t, m)
