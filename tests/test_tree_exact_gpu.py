"""GPU tests of the exact leaves of the device search trees (include/qttt_tree_exact.h, TreeSearch(exact_from=M)): whole
trees, solved flags and leaf rows against tests/exact_leaves_model.py's float64 model; every solved node against
VecEnv.solve; W / N at the root against the solver's q (the test that fails without the feature); unchanged bytes where
nothing is eligible; sync, compact and further search; guard bytes and nullable outputs; self-play and one Gumbel case.
tests/test_tree_exact_cpu.py asserts, without a GPU, that every search compared here solves nodes."""
import functools
import os

import numpy as np
import pytest
import torch

import exact_leaves_model as E
import gumbel_model as GM
import selfplay_model
import tree_harness as H
import tree_layout
import tree_model
from tree_harness import DEV, GUARD, env_from_arrays, export
from tree_harness import bits32 as _bits, check_exact_tree as _check, env_of_planes as _env_of_planes, exact_net as _net
from tree_harness import exact_rounds as _rounds, games_view as _view, prefix as _prefix

from qtttgym_amd import SelfPlay
from qtttgym_amd.actions import action36_to_pairs

pytestmark = pytest.mark.gpu
NETS = H.exact_nets()
SOLVED, SHIFT, MASK = E.NODE_SOLVED, E.NODE_VALUE_SHIFT, E.NODE_VALUE_MASK
_model = functools.partial(H.exact_model, E)
_stages = functools.partial(H.exact_stages, E)
_search = functools.partial(H.exact_search, E)


# ---------------------------------------------------------------- whole trees under the exact networks
@pytest.mark.parametrize("G", [3, 65])
@pytest.mark.parametrize("case", E.WHOLE_CASES, ids=lambda c: "%s-K%d-M%d-cap%d" % c)
def test_whole_trees_match_the_model_bit_for_bit(case, G):
    net, K, M, capacity = case
    m = _view(_model(net, K, M, capacity), G)
    t, _ = _search(_prefix(E.roots(E.G_MAX)[0], G), capacity, _net(net), leaves=K, exact_from=M)
    if capacity == E.OVERFLOW_CAPACITY:
        _rounds(t, E.ROLLOUTS)
    else:
        t.contemplate(E.ROLLOUTS)
    assert t.rollout_idx == E.ROLLOUTS and set(t._rounds) <= {1, K, (E.ROLLOUTS - 1) % K}
    _check(t, m)
    over = np.array([d["overflow"] for d in m.dump()])
    assert np.array_equal(t.root_stats()["overflow"].cpu().numpy(), over)
    assert (M == 9) == (int(t.solved_count().sum()) == 0) or G < E.G_MAX


# ---------------------------------------------------------------- the golden network: rounds in lockstep
@pytest.mark.parametrize("K,M", [(1, 7), (4, 6), (8, 7)])
def test_rounds_in_lockstep_with_the_model_fed_by_evaluate(K, M):
    """Per round the model backs up the device's own evaluate rows; the device's leaf_value / leaf_exact rows after
    qttt_tree_solve_leaves equal the model's, bit for bit, and so does the whole tree."""
    G, net = E.G_MAX, _net("shipped")
    arrays = E.roots(G)[0]
    t, _ = _search(arrays, E.CAPACITY, net, leaves=K, exact_from=M)
    m = E.ExactLeavesModel(1, seed=E.SEED, board_offset=E.OFFSET, capacity=E.CAPACITY, leaves=K, exact_from=M)
    m.reset(E.boards_of(arrays))
    exact_rows = shared = 0
    for r, k in enumerate([1] + [K] * 5):
        b = t._round_buffers(k)
        leaves = m.select_batch(k, t.virtual_loss)
        t._call("qttt_tree_select_batch", t.tree.data_ptr(), G, t.capacity, t.seed, t.rollout_idx, k, t.board_offset, t.c_puct,
                t.virtual_loss, b["paths"].data_ptr(), b["leaf"].state.data_ptr())
        ex = export(b["leaf"])
        assert np.array_equal(ex["board"], leaves.board) and np.array_equal(ex["n_moves"], leaves.n_moves), r
        ev = b["leaf"].evaluate(net, out=b["out"])
        value, probs = ev["value"].cpu().numpy().copy(), ev["probs"].cpu().numpy()
        state = b["leaf"].state.clone()
        t._backup_round(b, k)
        t.rollout_idx += k
        assert torch.equal(state, b["leaf"].state)
        m.backup_batch(value, probs)
        ref_value, ref_exact = m.last_rows
        assert np.array_equal(b["exact"].cpu().numpy(), ref_exact), r
        assert np.array_equal(_bits(b["out"]["value"].cpu().numpy()), _bits(ref_value)), r
        assert np.array_equal(_bits(value)[ref_exact == 0], _bits(ref_value)[ref_exact == 0])
        exact_rows += int(ref_exact.sum())
        shared = m.met["same_eligible_leaf"]
        _check(t, m)
    assert exact_rows > 0 and m.met["reused"] > 0 and (shared > 0 or K == 1) and m.in_flight() == 0


# ---------------------------------------------------------------- a workgroup whose list of boards is full
def _fresh_rows(m):
    """Per game and record of the model's round in flight: the leaf is eligible and not yet solved."""
    return np.array([[bool(m.eligible(st, rec)) and rec["leaf"] not in st["solved"] for rec in m.round[g]]
                     for g, st in enumerate(m._games)])


def _model_at(arrays, K, M):
    m = E.ExactLeavesModel(1, seed=E.SEED, board_offset=E.OFFSET, capacity=E.CAPACITY, net=NETS["sharp"](), leaves=K, exact_from=M)
    m.reset(E.boards_of(arrays))
    return m


def test_a_round_whose_aligned_blocks_of_64_records_are_all_fresh_eligible_leaves():
    """qttt_tree_solve_leaves with full lists: 33 games * 4 leaves, so records 0..63 and 64..127 are two workgroups of
    64 and records 128..131 a third.  The roots are the fixture's five-move boards, chosen with the model alone: game g
    takes the first board, cycling from g, whose four leaves of the second round the model finds eligible and unsolved
    (a game's descents depend on its position and its index only).  After the one-leaf round that gives the roots their
    priors, every record of the round of four is then a six-move child that needs enumeration."""
    K, M, G = 4, 6, 33
    z = E.fixture()
    five = np.flatnonzero(z["played"] == 5)
    ok = np.zeros((len(five), G), dtype=bool)
    for i, p in enumerate(five):
        m = _model_at({k: z[k][np.full(G, p)] for k in E.ARRAYS}, K, M)
        m.round_of(1)
        m.select_batch(K, m.virtual_loss)
        ok[i] = _fresh_rows(m).all(1)
    assert ok.any(0).all()
    pick = [five[next((g + i) % len(five) for i in range(len(five)) if ok[(g + i) % len(five), g])] for g in range(G)]
    arrays = {k: z[k][np.array(pick)] for k in E.ARRAYS}
    m = _model_at(arrays, K, M)
    t, _ = _search(arrays, E.CAPACITY, _net("sharp"), leaves=K, exact_from=M)
    m.round_of(1)
    t._round(1)
    assert int(t.solved_count().sum()) == 0
    leaves = m.select_batch(K, m.virtual_loss)
    assert _fresh_rows(m).all()                                   # the model alone: both blocks of 64 are full
    distinct = np.array([len({rec["leaf"] for rec in m.round[g]}) for g in range(G)])
    m.backup_batch(m.playouts(leaves), m.priors(leaves))
    t._round(K)
    exact = t._rounds[K]["exact"].cpu().numpy()
    assert exact.shape == (G * K,) and (exact[:128] == 1).all() and np.array_equal(exact, m.last_rows[1])
    assert np.array_equal(t.solved_count().cpu().numpy(), distinct) and (distinct >= 1).all()   # from 0: none was solved before
    assert np.array_equal(_bits(t._rounds[K]["out"]["value"].cpu().numpy()), _bits(m.last_rows[0]))
    _check(t, m)


# ---------------------------------------------------------------- solved nodes against the solver
@pytest.mark.parametrize("K,M", [(8, 6), (4, 7), (1, 8)])
def test_every_solved_node_holds_the_solver_s_value_and_is_a_leaf(K, M):
    G = E.G_MAX
    t, _ = _search(E.roots(G)[0], E.CAPACITY, _net("shipped"), leaves=K, exact_from=M)
    t.contemplate(E.ROLLOUTS)
    games, nodes, _, _ = tree_layout.decode(t.tree.cpu().numpy(), G, t.capacity)
    live = np.arange(t.capacity)[None, :] < games["used"][:, None]
    solved = live & ((nodes["flags"] & SOLVED) != 0)
    assert solved.sum() > 0 and not (nodes["flags"][live & ~solved] & np.uint32(SOLVED | MASK)).any()
    sel = nodes[solved]
    res = _env_of_planes(sel["P"], sel["Q"]).solve(min_ply=M)
    assert res.solved.all()
    stored = ((sel["flags"] & MASK) >> SHIFT).astype(np.int64)
    assert (stored <= 32).all()
    assert np.array_equal(_bits(((stored - 16) / 16.0).astype(np.float32)), _bits(res.value.cpu().numpy()))
    # every one of them is below its root here (nothing was synced): no priors, no terminal flag, no child
    roots = np.zeros_like(solved)
    roots[np.arange(G), games["root"]] = True
    assert not (solved & roots).any()
    assert not (sel["flags"] & (tree_layout.NODE_PRIORS | tree_layout.NODE_TERMINAL)).any()
    assert (sel["slots"]["child"] == -1).all() and not sel["Ntot"].any() and not sel["slots"]["N"].any()


# ---------------------------------------------------------------- the test that fails without the feature
def _root_statistics_are_the_solver_s_q(arrays, K):
    """From a root with five moves played every child has six, so with exact_from = 6 every child is a solved leaf and W
    of a root action is a sum of sixteenths, exact in f64: for an action that is no collapse W / N == the solver's q, bit
    for bit; for a collapse W / N lies between the two children's negated values.  Without exact_from the same search
    backs the network's values up and differs.  Returns the q compared: (of the actions that are no collapse, of the
    collapses whose two children were both visited)."""
    G, rollouts, net = len(arrays["n_moves"]), 41, _net("sharp")
    seen_exact, seen_between = [], []
    env = env_from_arrays(arrays)
    q = env.solve(min_ply=5).q.double().cpu().numpy()
    t, _ = _search(arrays, 2 + 2 * rollouts, net, leaves=K, exact_from=6)
    t.contemplate(rollouts)
    st = {k: v.cpu().numpy() for k, v in t.root_stats().items()}
    _, nodes, _, _ = tree_layout.decode(t.tree.cpu().numpy(), G, t.capacity)
    child = nodes[:, 0]["slots"]["child"]
    exact = between = 0
    for g in range(G):
        for a in np.flatnonzero(st["N"][g] > 0):
            c = int(child[g, a])
            assert c >= 0
            mean = st["W"][g, a] / st["N"][g, a]
            if not c & tree_layout.CHILD_PAIR:
                assert mean == q[g, a] == st["Q"][g, a], (g, a)
                exact += 1
                seen_exact.append(q[g, a])
            else:
                kids = nodes[g, [c & (tree_layout.CHILD_PAIR - 1), (c & (tree_layout.CHILD_PAIR - 1)) + 1]]
                vals = [0.0 - (((int(f) & MASK) >> SHIFT) - 16) / 16.0 for f in kids["flags"] if f & SOLVED]
                if len(vals) == 2:                       # both children were visited, and neither is terminal
                    assert min(vals) <= mean <= max(vals) and (min(vals) + max(vals)) / 2 == q[g, a], (g, a)
                    between += 1
                    seen_between.append(q[g, a])
    assert exact >= 3 * G and between > 0
    plain, _ = _search(arrays, 2 + 2 * rollouts, net, leaves=K)
    plain.contemplate(rollouts)
    ps = {k: v.cpu().numpy() for k, v in plain.root_stats().items()}
    seen = ps["N"] > 0
    assert (ps["W"][seen] / ps["N"][seen] != q[seen]).any()
    assert int(plain.solved_count().sum()) == 0
    return np.array(seen_exact), np.array(seen_between)


@pytest.mark.parametrize("K", [1, 4])
def test_root_statistics_of_five_move_boards_are_the_solver_s_q(K):
    _root_statistics_are_the_solver_s_q(E.roots(16, played=5)[0], K)


@pytest.mark.parametrize("K", [1, 4])
def test_root_statistics_of_the_deep_five_move_boards_are_the_solver_s_q_down_to_sixteenths(K):
    """The same from tests/golden/solve_deep.npz's five-move boards that carry sixteenths and eighths: the value kept in
    a node's spare flag bits is then compared at odd multiples of 1/8 (W / N of a single child) and its halved sum at odd
    multiples of 1/16 (a collapse whose two children were visited)."""
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "solve_deep.npz")) as z:
        five = np.flatnonzero(z["played"] == 5)
        q16 = z["q"][five].astype(np.float64) * 16
        fin = np.isfinite(q16)
        odd8 = (fin & (np.where(fin, q16, 0) % 4 != 0)).any(1)           # an eighth or a sixteenth among the board's q
        assert (fin & (np.where(fin, q16, 0) % 2 != 0)).any(1).sum() >= 1 and odd8.sum() >= 9
        arrays = {k: z[k][five[odd8]] for k in E.ARRAYS}
    exact, between = _root_statistics_are_the_solver_s_q(arrays, K)
    odd = lambda x, m: int((np.round(x * 16).astype(np.int64) % m != 0).sum())  # noqa: E731
    print("deep roots K=%d: %d boards, %d single-child q (%d eighths), %d collapse q (%d eighths or sixteenths, %d sixteenths)"
          % (K, len(five[odd8]), len(exact), odd(exact, 4), len(between), odd(between, 4), odd(between, 2)))
    assert odd(exact, 4) + odd(between, 4) > 0


# ---------------------------------------------------------------- unchanged results
@pytest.mark.parametrize("K", [1, 4])
def test_where_nothing_is_eligible_the_tree_bytes_are_those_of_the_search_without_exact_leaves(K):
    """exact_from = 9 finds no eligible leaf (a position with nine moves played is terminal), and exact_from = None is the
    parent's route: both leave the same bytes, the bytes after the tree included.  At leaves = 1 the parent's contemplate()
    goes through qttt_tree_select, which records its path in the game header where a round clears it
    (qttt_tree_leaves.h), so there the whole buffer is compared with the parent's rounds of one leaf, and everything but
    the headers' recorded path with its contemplate()."""
    G, net = E.G_MAX, _net("shipped")
    arrays = E.roots(G)[0]
    a, _ = _search(arrays, E.CAPACITY, net, leaves=K)
    b, _ = _search(arrays, E.CAPACITY, net, leaves=K, exact_from=9)
    for t in (a, b):
        t.contemplate(E.ROLLOUTS)
    assert a.exact_from is None and all("exact" not in r for r in a._rounds.values()) and (K > 1 or a._rounds == {})
    assert "exact" in b._rounds[1] and not any(int(r["exact"].sum()) for r in b._rounds.values())
    assert int(b.solved_count().sum()) == 0
    if K > 1:
        assert torch.equal(a.tree, b.tree)
        return
    rounds, _ = _search(arrays, E.CAPACITY, net, leaves=1)
    for _ in range(E.ROLLOUTS):
        rounds._round(1)
    assert torch.equal(rounds.tree, b.tree)
    ga, na, pa, ta = tree_layout.decode(a.tree.cpu().numpy(), G, E.CAPACITY)
    gb, nb, pb, tb = tree_layout.decode(b.tree.cpu().numpy(), G, E.CAPACITY)
    assert np.array_equal(na.view(np.uint8), nb.view(np.uint8)) and np.array_equal(pa.view(np.uint32), pb.view(np.uint32))
    assert np.array_equal(ta, tb) and np.array_equal(ga["used"], gb["used"]) and np.array_equal(ga["root"], gb["root"])
    assert np.array_equal(ga["flags"] & tree_layout.GAME_OVERFLOW, gb["flags"] & tree_layout.GAME_OVERFLOW)


# ---------------------------------------------------------------- sync, compact, further search
@pytest.mark.parametrize("compact", [False, True])
def test_sync_compact_and_further_search_stay_equal_to_the_model(compact):
    K, M, G = 4, 7, E.G_MAX
    stages, act, bits = _stages("sharp", K, M)
    t, env = _search(E.roots(G)[0], E.CAPACITY, _net("sharp"), leaves=K, exact_from=M)
    t.contemplate(E.ROLLOUTS)
    _check(t, stages["first"])
    env.step_raw(action36_to_pairs(torch.as_tensor(act, device=DEV)).contiguous(), torch.as_tensor(bits, device=DEV))
    t.sync(env)
    _check(t, stages["synced"])
    games, nodes, _, _ = tree_layout.decode(t.tree.cpu().numpy(), G, t.capacity)
    was_leaf = (nodes[np.arange(G), games["root"]]["flags"] & (SOLVED | tree_layout.NODE_PRIORS)) == SOLVED
    assert was_leaf.sum() > 0
    if compact:
        t.compact()
    t.contemplate(2 * K + 1)
    _check(t, stages["second", compact], compacted=compact)
    games, nodes, _, _ = tree_layout.decode(t.tree.cpu().numpy(), G, t.capacity)
    roots = nodes[np.arange(G), games["root"]][was_leaf]
    assert ((roots["flags"] & (SOLVED | tree_layout.NODE_PRIORS)) == (SOLVED | tree_layout.NODE_PRIORS)).all()
    assert (roots["slots"]["child"] >= 0).any(1).all() and (roots["Ntot"] == 2 * K).all()      # the first round gave the priors


# ---------------------------------------------------------------- arguments and output buffers
def test_guard_bytes_nullable_outputs_and_an_untouched_leaf_state():
    K, M, G = 4, 7, E.G_MAX
    net = _net("sharp")
    t, _ = _search(E.roots(G)[0], E.CAPACITY, net, leaves=K, exact_from=M)
    t.contemplate(1 + 2 * K)
    b = t._round_buffers(K)
    t._call("qttt_tree_select_batch", t.tree.data_ptr(), G, t.capacity, t.seed, t.rollout_idx, K, t.board_offset, t.c_puct,
            t.virtual_loss, b["paths"].data_ptr(), b["leaf"].state.data_ptr())
    ev = b["leaf"].evaluate(net, out=b["out"])
    before, state, paths, n = t.tree.clone(), b["leaf"].state.clone(), b["paths"].clone(), G * K

    def run(value, exact):
        t.tree.copy_(before)
        t._call("qttt_tree_solve_leaves", t.tree.data_ptr(), G, t.capacity, K, b["paths"].data_ptr(),
                b["leaf"].state.data_ptr(), M, None if value is None else value.data_ptr(),
                None if exact is None else exact.data_ptr())
        assert torch.equal(b["leaf"].state, state) and torch.equal(b["paths"], paths)
        return t.tree.clone()

    pad = 16
    value = torch.full((n + 2 * pad,), float("nan"), dtype=torch.float32, device=DEV)
    value[pad:pad + n] = ev["value"]
    guard_v = value.clone()
    exact = torch.full((n + 2 * pad,), GUARD, dtype=torch.uint8, device=DEV)
    both = run(value[pad:pad + n], exact[pad:pad + n])
    hit = exact[pad:pad + n].bool()
    assert 0 < int(hit.sum()) < n and set(exact[pad:pad + n].unique().tolist()) == {0, 1}
    assert (exact[:pad] == GUARD).all() and (exact[pad + n:] == GUARD).all()
    assert torch.equal(value[:pad].view(torch.int32), guard_v[:pad].view(torch.int32))
    assert torch.equal(value[pad + n:].view(torch.int32), guard_v[pad + n:].view(torch.int32))
    got = value[pad:pad + n]
    assert torch.equal(got[~hit].view(torch.int32), ev["value"][~hit].view(torch.int32))          # untouched rows
    assert ((got[hit] * 16).round() == got[hit] * 16).all() and (got[hit].abs() <= 1).all()
    assert not torch.equal(both, before)                                                           # nodes were solved
    only_v = ev["value"].clone()
    assert torch.equal(run(only_v, None), both) and torch.equal(only_v.view(torch.int32), got.view(torch.int32))
    only_e = torch.full((n,), GUARD, dtype=torch.uint8, device=DEV)
    assert torch.equal(run(None, only_e), both) and torch.equal(only_e, exact[pad:pad + n])
    assert torch.equal(run(None, None), both)
    # a second call finds every eligible node solved: the same rows, the tree unchanged
    again_v, again_e = ev["value"].clone(), torch.zeros(n, dtype=torch.uint8, device=DEV)
    t._call("qttt_tree_solve_leaves", t.tree.data_ptr(), G, t.capacity, K, b["paths"].data_ptr(), b["leaf"].state.data_ptr(),
            M, again_v.data_ptr(), again_e.data_ptr())
    assert torch.equal(t.tree, both) and torch.equal(again_e, only_e) and torch.equal(again_v.view(torch.int32), got.view(torch.int32))
    t._call("qttt_tree_backup_batch_exact", t.tree.data_ptr(), G, t.capacity, K, b["paths"].data_ptr(), again_v.data_ptr(),
            ev["probs"].data_ptr())
    t.rollout_idx += K
    m = E.searched(NETS["sharp"](), K, M, E.CAPACITY, rollouts=1 + 3 * K)
    _check(t, m)


# ---------------------------------------------------------------- SelfPlay
def test_selfplay_with_exact_leaves_matches_the_model(monkeypatch):
    G, R_, seed, K, M = 8, 8, 7, 4, 7
    sp = SelfPlay(G, n_rollouts=R_, net=_net("sharp"), seed=seed, device=DEV, leaf_eval="value", leaves=K, exact_from=M)
    batch = sp.play()
    assert sp.tree.exact_from == M and sorted(sp.tree._rounds) == [1, 3, 4] and int(sp.tree.solved_count().sum()) > 0
    dev = {k: getattr(batch, k).cpu().numpy() for k in ("pi", "mask", "done", "v", "action36", "length", "winner", "actions")}
    made = []

    def make(*args, **kw):
        made.append(E.ExactLeavesModel(*args, leaves=K, exact_from=M, **kw))
        return made[-1]

    monkeypatch.setattr(tree_model, "TreeModel", make)
    ref, ref_env = selfplay_model.play(G, R_, 1, seed=seed, net=NETS["sharp"]())
    for k, d in dev.items():
        a, b = np.ascontiguousarray(d), np.ascontiguousarray(ref[k])
        if a.dtype.kind == "f":
            a, b = a.view("u%d" % a.dtype.itemsize), b.view("u%d" % b.dtype.itemsize)
        assert np.array_equal(a, b), (k, np.argwhere(a != b)[:6])
    ex = export(sp.env)
    assert np.array_equal(ex["board"], ref_env.board) and np.array_equal(ex["n_moves"], ref_env.n_moves)
    assert made[0].met["enumerated"] > 0 and made[0].met["solved_root_expanded"] > 0
    plain = SelfPlay(G, n_rollouts=R_, net=_net("sharp"), seed=seed, device=DEV, leaf_eval="value", leaves=K).play()
    assert not torch.equal(plain.pi, batch.pi)


def test_the_gumbel_root_with_exact_leaves_matches_the_gumbel_model():
    G, K, M, n = E.G_MAX, 4, 7, 16
    arrays = E.roots(G)[0]
    t, _ = _search(arrays, E.CAPACITY, _net("sharp"), leaves=K, exact_from=M, root_policy="gumbel", max_considered=4)
    t.contemplate(n + 1)
    rec = t._gumbel["rec"].cpu().numpy()[:G * GM.GUMBEL_BYTES].view(GM.REC_DTYPE)
    m = E.ExactGumbelModel(1, seed=E.SEED, board_offset=E.OFFSET, capacity=E.CAPACITY, net=NETS["sharp"](), leaves=K,
                           max_considered=4, exact_from=M)
    m.reset(E.boards_of(arrays))
    m.contemplate_gumbel(n + 1, records=rec)
    assert m.met["enumerated"] > 0 and m.met["reused"] > 0
    _check(t, m)
    st = t.root_stats()
    choose = np.array([f[0] for f in m.finals()], dtype=np.uint8)
    assert np.array_equal(st["choose"].cpu().numpy(), choose)
