"""GPU tests of the proven interior nodes of the device search trees (include/qttt_tree_prove.h, TreeSearch(exact_from=M,
prove=True)): whole trees, solved flags, kept priors rows and the per-round `proved` counts against tests/prove_model.py's
float64 model; every solved node against VecEnv.solve; q_exact, root_value_exact and choose(exact=True) against the
solver's q, value and best of the roots (the test that pins the rule); unchanged bytes and launches without the keyword;
sync onto a proven child, compact and further search; guard bytes, nullable outputs and idempotence; one Gumbel search
and one self-play.  tests/test_tree_prove_cpu.py asserts, without a GPU, what each search compared here proves."""
import functools

import numpy as np
import pytest
import torch

import exact_leaves_model as E
import gumbel_model as GM
import prove_model as PM
import selfplay_model
import tree_harness as H
import tree_layout
import tree_model
from tree_harness import DEV, GUARD, SENTINEL, TAIL, export
from tree_harness import bits32 as _bits, env_of_planes as _env_of_planes, exact_net as _net
from tree_harness import exact_rounds as _rounds, games_view as _view, prefix as _prefix

from qtttgym_amd import SelfPlay
from qtttgym_amd.actions import action36_to_pairs

pytestmark = pytest.mark.gpu
NETS = H.exact_nets()
SOLVED, SHIFT, MASK = E.NODE_SOLVED, E.NODE_VALUE_SHIFT, E.NODE_VALUE_MASK
_model = functools.partial(H.exact_model, PM)
_stages = functools.partial(H.exact_stages, PM)
_search = functools.partial(H.exact_search, PM)
_check = functools.partial(H.check_exact_tree, kept_rows=True)      # and the priors rows that proven nodes keep


# ---------------------------------------------------------------- whole trees under the exact networks
@pytest.mark.parametrize("G", [3, 65])
@pytest.mark.parametrize("case", PM.WHOLE_CASES, ids=lambda c: "%s-K%d-M%d-cap%d" % c)
def test_whole_trees_match_the_model_bit_for_bit(case, G):
    net, K, M, capacity = case
    m = _view(_model(net, K, M, capacity), G)
    t, _ = _search(_prefix(PM.roots(PM.G_MAX)[0], G), capacity, _net(net), leaves=K, exact_from=M, prove=True)
    if capacity == PM.OVERFLOW_CAPACITY:
        _rounds(t, PM.ROLLOUTS)
    else:
        t.contemplate(PM.ROLLOUTS)
    assert t.rollout_idx == PM.ROLLOUTS and all("proved" in b for b in t._rounds.values())
    _check(t, m)
    over = np.array([d["overflow"] for d in m.dump()])
    assert np.array_equal(t.root_stats()["overflow"].cpu().numpy(), over)
    ex = m.root_exact()
    st = t.root_stats()
    for k in ("proven", "root_solved"):
        assert np.array_equal(st[k].cpu().numpy(), ex[k]), k
    for k in ("q_exact", "root_value_exact"):
        assert np.array_equal(_bits(st[k].cpu().numpy())[~np.isnan(ex[k])], _bits(ex[k])[~np.isnan(ex[k])]), k
        assert np.isnan(st[k].cpu().numpy()[np.isnan(ex[k])]).all(), k
    assert np.array_equal(t.choose(exact=True).cpu().numpy(), m.choose_exact(t.choose().cpu().numpy()))


@pytest.mark.parametrize("case", PM.FLOOR_CASES, ids=lambda c: "%s-K%d-M%d-cap%d" % c)
def test_after_every_round_the_tree_and_the_proved_counts_match_the_model(case):
    net, K, M, capacity = case
    G = PM.G_MAX
    arrays = PM.roots(G)[0]
    t, _ = _search(arrays, capacity, _net(net), leaves=K, exact_from=M, prove=True)
    m = PM.ProveLeavesModel(1, seed=PM.SEED, board_offset=PM.OFFSET, capacity=capacity, net=NETS[net](), leaves=K, exact_from=M)
    m.reset(E.boards_of(arrays))
    total = kept = 0
    for k in PM.schedule(24, K):
        m.round_of(k)
        t._round(k)
        proved = t._rounds[k]["proved"].cpu().numpy()
        assert np.array_equal(proved, m.last_proved), m.met["rounds"]
        total += int(proved.sum())
        kept += _check(t, m)
    assert total > 0 and kept > 0 and m.met["ended_on_proven_early"] > 0


@pytest.mark.parametrize("K,M", [(4, 8), (1, 7), (8, 6)])
def test_rounds_in_lockstep_with_the_model_fed_by_evaluate(K, M):
    """The golden network: per round the model backs up the device's own evaluate rows and proves; the device's proved
    counts and whole tree equal the model's, bit for bit.  A record that ends on a proven node with fewer than M moves
    played is not eligible: its leaf_value row stays the network's and its leaf_exact is 0 (the model's last_rows)."""
    G, net = PM.G_MAX, _net("shipped")
    arrays = PM.roots(G)[0]
    t, _ = _search(arrays, PM.CAPACITY, net, leaves=K, exact_from=M, prove=True)
    m = PM.ProveLeavesModel(1, seed=PM.SEED, board_offset=PM.OFFSET, capacity=PM.CAPACITY, leaves=K, exact_from=M)
    m.reset(E.boards_of(arrays))
    total = 0
    for r, k in enumerate([1] + [K] * (9 if K > 1 else 30)):
        b = t._round_buffers(k)
        m.select_batch(k, t.virtual_loss)
        t._call("qttt_tree_select_batch", t.tree.data_ptr(), G, t.capacity, t.seed, t.rollout_idx, k, t.board_offset, t.c_puct,
                t.virtual_loss, b["paths"].data_ptr(), b["leaf"].state.data_ptr())
        ev = b["leaf"].evaluate(net, out=b["out"])
        value, probs = ev["value"].cpu().numpy().copy(), ev["probs"].cpu().numpy()
        t._backup_round(b, k)
        t.rollout_idx += k
        m.backup_batch(value, probs)
        ref_value, ref_exact = m.last_rows
        assert np.array_equal(b["exact"].cpu().numpy(), ref_exact), r
        assert np.array_equal(_bits(b["out"]["value"].cpu().numpy()), _bits(ref_value)), r
        assert np.array_equal(b["proved"].cpu().numpy(), m.last_proved), r
        total += int(m.last_proved.sum())
    _check(t, m)
    assert m.in_flight() == 0
    print("golden network K=%d M=%d: %d nodes proven, %d below the root, %d records ended on a proven node"
          % (K, M, total, m.met["proved_below_root"], m.met["ended_on_proven"]))
    if M == 8:                        # the other two are comparisons alone: what this network proves there is not known beforehand
        assert total > 0 and m.met["ended_on_proven_early"] > 0 and m.met["proved_below_root"] > 0


# ---------------------------------------------------------------- solved nodes and the roots against the solver
@pytest.mark.parametrize("K,M", [(4, 8), (8, 7), (1, 8)])
def test_every_solved_node_holds_the_solver_s_value_of_its_own_state(K, M):
    G = PM.G_MAX
    t, _ = _search(PM.roots(G)[0], PM.CAPACITY, _net("shipped"), leaves=K, exact_from=M, prove=True)
    t.contemplate(PM.ROLLOUTS)
    games, nodes, _, _ = tree_layout.decode(t.tree.cpu().numpy(), G, t.capacity)
    live = np.arange(t.capacity)[None, :] < games["used"][:, None]
    solved = live & ((nodes["flags"] & SOLVED) != 0)
    assert solved.sum() > 0 and not (nodes["flags"][live & ~solved] & np.uint32(SOLVED | MASK)).any()
    sel = nodes[solved]
    interior = (sel["slots"]["child"] >= 0).any(1)                # a solved node with children was proven, not enumerated
    assert interior.sum() > 0
    res = _env_of_planes(sel["P"], sel["Q"]).solve(min_ply=4)
    assert res.solved.all()
    stored = ((sel["flags"] & MASK) >> SHIFT).astype(np.int64)
    assert (stored <= 32).all()
    assert np.array_equal(_bits(((stored - 16) / 16.0).astype(np.float32)), _bits(res.value.cpu().numpy()))
    # below its root a solved node has no priors; every root keeps them
    roots = np.zeros_like(solved)
    roots[np.arange(G), games["root"]] = True
    assert not (nodes["flags"][solved & ~roots] & (tree_layout.NODE_PRIORS | tree_layout.NODE_UNIFORM | tree_layout.NODE_TERMINAL)).any()
    assert (nodes["flags"][roots] & tree_layout.NODE_PRIORS).all()


@pytest.mark.parametrize("K,M,net", [(4, 8, "shipped"), (8, 7, "shipped"), (4, 6, "zero"), (1, 8, "zero")])
def test_q_exact_is_the_solver_s_q_and_the_exact_choice_its_best_move(K, M, net):
    """The test that pins the rule: wherever an action of the root is proven, q_exact equals VecEnv.solve's q of the
    root, bit for bit and never -0.0; a solved root's value is solve's value and choose(exact=True) its best move; every
    other game keeps its ordinary choice."""
    G = PM.G_MAX
    arrays = PM.roots(G)[0]
    t, env = _search(arrays, PM.CAPACITY, _net(net), leaves=K, exact_from=M, prove=True)
    t.contemplate(PM.ROLLOUTS)
    sol = env.solve(min_ply=4)
    q, value, best = sol.q.cpu().numpy(), sol.value.cpu().numpy(), sol.best.cpu().numpy()
    st = {k: v.cpu().numpy() for k, v in t.root_stats().items()}
    proven, solved = st["proven"], st["root_solved"]
    assert proven.dtype == bool and solved.dtype == bool and st["q_exact"].dtype == np.float32
    assert proven.any() and solved.any() and not solved.all()
    assert np.array_equal(_bits(st["q_exact"])[proven], _bits(q)[proven])
    assert np.isnan(st["q_exact"][~proven]).all() and np.isnan(st["root_value_exact"][~solved]).all()
    assert not np.signbit(st["q_exact"][proven][st["q_exact"][proven] == 0]).any()
    assert np.array_equal(_bits(st["root_value_exact"])[solved], _bits(value)[solved])
    legal = np.isfinite(q)
    assert np.array_equal(proven[solved], legal[solved])         # a root that a round proved: every legal action is proven
    ordinary, exact = t.choose().cpu().numpy(), t.choose(exact=True).cpu().numpy()
    assert np.array_equal(exact[solved], best[solved]) and np.array_equal(exact[~solved], ordinary[~solved])
    assert np.array_equal(st["choose"], ordinary)
    plain, _ = _search(arrays, PM.CAPACITY, _net(net), leaves=K, exact_from=M)
    assert "proven" not in plain.root_stats()
    with pytest.raises(ValueError, match="needs prove=True"):
        plain.choose(exact=True)


# ---------------------------------------------------------------- unchanged results
@pytest.mark.parametrize("K", [1, 4])
def test_without_the_keyword_the_bytes_and_the_launches_are_those_of_the_exact_leaves(K):
    G, net, M = PM.G_MAX, _net("shipped"), 8
    arrays = PM.roots(G)[0]
    trees, calls = {}, {}
    for name, kw in (("none", {}), ("false", dict(prove=False)), ("true", dict(prove=True))):
        t, _ = _search(arrays, PM.CAPACITY, net, leaves=K, exact_from=M, **kw)
        log, call = [], t._call
        t._call = lambda entry, *a, _log=log, _call=call: (_log.append(entry), _call(entry, *a))[1]
        t.contemplate(24)
        trees[name], calls[name] = t, log
    rounds = len(PM.schedule(24, K))
    per_round = ["qttt_tree_select_batch", "qttt_tree_solve_leaves", "qttt_tree_backup_batch_exact"]
    assert calls["none"] == calls["false"] == per_round * rounds              # and one evaluate per round, as ever
    assert calls["true"] == (per_round + ["qttt_tree_prove"]) * rounds
    assert trees["none"].prove is False and all("proved" not in b for b in trees["false"]._rounds.values())
    assert torch.equal(trees["none"].tree, trees["false"].tree)
    assert not torch.equal(trees["none"].tree, trees["true"].tree)
    assert int(trees["true"].solved_count().sum()) > int(trees["false"].solved_count().sum())


# ---------------------------------------------------------------- sync, compact, further search
@pytest.mark.parametrize("compact", [False, True])
def test_sync_onto_a_proven_child_compact_and_further_search_stay_equal_to_the_model(compact):
    net, K, M, G = "zero", 4, 8, PM.G_MAX
    stages, act, bits = _stages(net, K, M)
    t, env = _search(PM.roots(G)[0], PM.CAPACITY, _net(net), leaves=K, exact_from=M, prove=True)
    t.contemplate(PM.ROLLOUTS)
    _check(t, stages["first"])
    env.step_raw(action36_to_pairs(torch.as_tensor(act, device=DEV)).contiguous(), torch.as_tensor(bits, device=DEV))
    t.sync(env)
    _check(t, stages["synced"])
    games, nodes, _, _ = tree_layout.decode(t.tree.cpu().numpy(), G, t.capacity)
    root = nodes[np.arange(G), games["root"]]
    onto = ((root["flags"] & (SOLVED | tree_layout.NODE_PRIORS)) == SOLVED) & (root["slots"]["child"] >= 0).any(1)
    assert onto.sum() > 0                                         # roots that were proven while they were children
    if compact:
        t.compact()
    t.contemplate(2 * K + 1)
    _check(t, stages["second", compact], compacted=compact)
    games, nodes, _, _ = tree_layout.decode(t.tree.cpu().numpy(), G, t.capacity)
    root = nodes[np.arange(G), games["root"]][onto]
    assert ((root["flags"] & (SOLVED | tree_layout.NODE_PRIORS)) == (SOLVED | tree_layout.NODE_PRIORS)).all()
    ex = stages["second", compact].root_exact()
    st = t.root_stats()
    assert np.array_equal(st["proven"].cpu().numpy(), ex["proven"]) and np.array_equal(st["root_solved"].cpu().numpy(), ex["root_solved"])
    assert np.array_equal(t.choose(exact=True).cpu().numpy(), stages["second", compact].choose_exact(t.choose().cpu().numpy()))


# ---------------------------------------------------------------- arguments and output buffers
def test_guard_bytes_nullable_outputs_and_idempotence():
    K, M, G = 4, 8, PM.G_MAX
    net = _net("zero")
    t, _ = _search(PM.roots(G)[0], PM.CAPACITY, net, leaves=K, exact_from=M, prove=True)
    t.contemplate(1 + 3 * K)
    b = t._round_buffers(K)
    t._call("qttt_tree_select_batch", t.tree.data_ptr(), G, t.capacity, t.seed, t.rollout_idx, K, t.board_offset, t.c_puct,
            t.virtual_loss, b["paths"].data_ptr(), b["leaf"].state.data_ptr())
    ev = b["leaf"].evaluate(net, out=b["out"])
    t._call("qttt_tree_solve_leaves", t.tree.data_ptr(), G, t.capacity, K, b["paths"].data_ptr(), b["leaf"].state.data_ptr(),
            M, ev["value"].data_ptr(), b["exact"].data_ptr())
    t._call("qttt_tree_backup_batch_exact", t.tree.data_ptr(), G, t.capacity, K, b["paths"].data_ptr(), ev["value"].data_ptr(),
            ev["probs"].data_ptr())
    t.rollout_idx += K
    before, paths = t.tree.clone(), b["paths"].clone()
    assert (before[-TAIL:] == SENTINEL).all()
    pad = 16
    proved = torch.full((G + 2 * pad,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    guard = proved.clone()

    def prove(out):
        t._call("qttt_tree_prove", t.tree.data_ptr(), G, t.capacity, K, b["paths"].data_ptr(), None if out is None else out.data_ptr())
        assert torch.equal(b["paths"], paths)
        return t.tree.clone()

    first = prove(proved[pad:pad + G])
    assert torch.equal(proved[:pad], guard[:pad]) and torch.equal(proved[pad + G:], guard[pad + G:])
    assert int(proved[pad:pad + G].sum()) > 0 and (proved[pad:pad + G] >= 0).all()
    assert not torch.equal(first, before) and (first[-TAIL:] == SENTINEL).all()
    # only flags words changed: the buffers differ in the four bytes at offset 28 of node records alone
    diff = (first != before).nonzero().flatten().cpu().numpy()
    off = diff - G * tree_layout.GAME_BYTES
    assert (off >= 0).all() and (off < G * t.capacity * tree_layout.NODE_BYTES).all()
    assert ((off % tree_layout.NODE_BYTES >= 28) & (off % tree_layout.NODE_BYTES < 32)).all()
    again = torch.full((G,), -1, dtype=torch.int32, device=DEV)
    assert torch.equal(prove(again), first) and (again == 0).all()            # idempotent: the same bytes, nothing new
    t.tree.copy_(before)
    assert torch.equal(prove(None), first)                                     # proved is nullable
    m = PM.searched(NETS["zero"](), K, M, PM.CAPACITY, rollouts=1 + 4 * K)
    _check(t, m)
    assert np.array_equal(proved[pad:pad + G].cpu().numpy(), m.last_proved)

    # qttt_tree_root_exact: all four outputs between guards, then each alone
    n = G * 36
    q = torch.full((n + 2 * pad,), 7.5, dtype=torch.float32, device=DEV)
    pr = torch.full((n + 2 * pad,), GUARD, dtype=torch.uint8, device=DEV)
    val = torch.full((G + 2 * pad,), 7.5, dtype=torch.float32, device=DEV)
    so = torch.full((G + 2 * pad,), GUARD, dtype=torch.uint8, device=DEV)
    tree = t.tree.clone()

    def root(q_, pr_, val_, so_):
        t._call("qttt_tree_root_exact", t.tree.data_ptr(), G, t.capacity, *(None if x is None else x.data_ptr() for x in (q_, pr_, val_, so_)))
        assert torch.equal(t.tree, tree)                                       # read only

    root(q[pad:pad + n], pr[pad:pad + n], val[pad:pad + G], so[pad:pad + G])
    for x, size, fill in ((q, n, 7.5), (pr, n, GUARD), (val, G, 7.5), (so, G, GUARD)):
        assert (x[:pad] == fill).all() and (x[pad + size:] == fill).all()
    assert set(pr[pad:pad + n].unique().tolist()) == {0, 1} and set(so[pad:pad + G].unique().tolist()) <= {0, 1}
    ex = m.root_exact()
    assert np.array_equal(pr[pad:pad + n].cpu().numpy().reshape(G, 36).astype(bool), ex["proven"])
    assert np.array_equal(so[pad:pad + G].cpu().numpy().astype(bool), ex["root_solved"])
    alone = [torch.full((n,), 7.5, dtype=torch.float32, device=DEV), torch.full((n,), GUARD, dtype=torch.uint8, device=DEV),
             torch.full((G,), 7.5, dtype=torch.float32, device=DEV), torch.full((G,), GUARD, dtype=torch.uint8, device=DEV)]
    for i, (x, ref, size) in enumerate(zip(alone, (q, pr, val, so), (n, n, G, G))):
        root(*[x if j == i else None for j in range(4)])
        a, r = x.cpu().numpy(), ref[pad:pad + size].cpu().numpy()
        assert np.array_equal(a.view("u%d" % a.dtype.itemsize), r.view("u%d" % r.dtype.itemsize)), i
    root(None, None, None, None)


# ---------------------------------------------------------------- SelfPlay and the Gumbel root
def test_selfplay_that_proves_matches_the_model(monkeypatch):
    G, R_, seed, K, M = 8, 8, 7, 4, 7
    sp = SelfPlay(G, n_rollouts=R_, net=_net("sharp"), seed=seed, device=DEV, leaf_eval="value", leaves=K, exact_from=M, prove=True)
    batch = sp.play()
    assert sp.tree.prove is True and all("proved" in b for b in sp.tree._rounds.values())
    dev = {k: getattr(batch, k).cpu().numpy() for k in ("pi", "mask", "done", "v", "action36", "length", "winner", "actions")}
    made = []

    def make(*args, **kw):
        made.append(PM.ProveLeavesModel(*args, leaves=K, exact_from=M, **kw))
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
    assert made[0].met["proved_root"] + made[0].met["proved_below_root"] > 0


def test_the_gumbel_root_that_proves_matches_the_gumbel_model():
    G, K, M, n = PM.G_MAX, 4, 8, 24
    arrays = PM.roots(G)[0]
    t, _ = _search(arrays, PM.CAPACITY, _net("zero"), leaves=K, exact_from=M, prove=True, root_policy="gumbel", max_considered=4)
    t.contemplate(n + 1)
    rec = t._gumbel["rec"].cpu().numpy()[:G * GM.GUMBEL_BYTES].view(GM.REC_DTYPE)
    m = PM.ProveGumbelModel(1, seed=PM.SEED, board_offset=PM.OFFSET, capacity=PM.CAPACITY, net=NETS["zero"](), leaves=K,
                            max_considered=4, exact_from=M)
    m.reset(E.boards_of(arrays))
    m.contemplate_gumbel(n + 1, records=rec)
    assert sum(len(st["proven"]) for st in m.games) > 0
    _check(t, m)
    st = t.root_stats()
    choose = np.array([f[0] for f in m.finals()], dtype=np.uint8)
    assert np.array_equal(st["choose"].cpu().numpy(), choose)
    assert np.array_equal(st["proven"].cpu().numpy(), m.root_exact()["proven"])
    assert np.array_equal(t.choose(exact=True).cpu().numpy(), m.choose_exact(choose))
