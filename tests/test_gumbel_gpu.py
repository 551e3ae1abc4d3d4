"""The Gumbel root (include/qttt_tree_gumbel.h, TreeSearch(root_policy="gumbel")) on the MI355X against
tests/gumbel_model.py: the Gumbel values and the considered sets of begin; whole searches in lockstep with the model fed by
the device's own record and evaluations, every node after every round, through a move, a sync, a compaction and a second
search on the reused subtrees, also in a pool that overflows; the halving invariants on the device's result; the in-flight
bits; the unchanged PUCT path; SelfPlay; the C ABI's argument errors.  The cases are tests/gumbel_cases.py's.
The tests print the largest differences they meet before they assert (DESIGN.md §19 records them)."""
import numpy as np
import pytest
import torch

import gumbel_cases as C
import gumbel_model as GM
import leaf_parallel_model as LP
import selfplay_model
import tree_layout
import tree_model
from tree_harness import DEV, SENTINEL, TAIL, env_from_arrays, export
from value_tree_model import ValueTreeModel

from qtttgym_amd import PolicyValueNet, SelfPlay, TreeSearch, VecEnv, _native
from qtttgym_amd.actions import action36_to_pairs

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52
ERR_NULL, ERR_SIZE, ERR_ACTION = -1, -2, -3
LEFT_OUT = {"cases": 0, "left_out": 0}
_NETS = {}


def _net(name, dtype=torch.float32):
    if (name, dtype) not in _NETS:
        _NETS[name, dtype] = PolicyValueNet(C.net_state_dict(name), device=DEV, dtype=dtype)
    return _NETS[name, dtype]


def _search(case, net, **kw):
    G, K, n, m, cap = case
    env = env_from_arrays(C.positions(G))
    capacity = C.capacity_of(case)
    t = TreeSearch(G, capacity=capacity, net=net, seed=C.SEED, board_offset=C.OFFSET, device=DEV, leaf_eval="value",
                   leaves=K, root_policy="gumbel", max_considered=m, **kw)
    t.tree = torch.full((tree_layout.tree_bytes(G, capacity) + TAIL,), SENTINEL, dtype=torch.uint8, device=DEV)
    t.reset(env)
    return t, env


def _records(t):
    return t._gumbel["rec"].cpu().numpy()[:t.num_games * GM.GUMBEL_BYTES].view(GM.REC_DTYPE)


def _check(t, m, compacted=False):
    tree_layout.assert_tree_equals_model(t.tree.cpu().numpy(), t.num_games, t.capacity, m, SENTINEL, DEV, compacted=compacted)
    games, nodes, _, _ = tree_layout.decode(t.tree.cpu().numpy(), t.num_games, t.capacity)
    live = np.arange(t.capacity)[None, :] < games["used"][:, None]
    assert (nodes[live]["slots"]["N"] < 1 << 24).all() and (nodes[live]["Ntot"] < 1 << 24).all()      # nothing in flight


def _rel(dev, ref):
    """The largest |dev - ref| / max(|ref|, the smallest normal double)."""
    return float(np.max(np.abs(dev - ref) / np.maximum(np.abs(ref), np.finfo(np.float64).tiny), initial=0.0))


def _check_finals(t, m):
    st = {k: v.cpu().numpy() for k, v in t.root_stats().items()}
    assert np.array_equal(st["choose"], t.choose().cpu().numpy())
    worst = 0.0
    for g, (choose, pi, q_hat, _) in enumerate(m.finals()):
        assert st["choose"][g] == choose, g
        assert np.array_equal(st["q_completed"][g].view(np.int64), q_hat.view(np.int64)), g             # bit for bit
        finite = np.isfinite(pi).all()
        assert finite == np.isfinite(st["pi"][g]).all()
        if finite:
            worst = max(worst, _rel(st["pi"][g], pi))
            root = m.games[g]["nodes"][m.games[g]["root"]]
            assert not root.legal or abs(st["pi"][g].sum() - 1.0) <= 36 * EPS, g
    print("pi: largest relative difference %.3g (%.2f * 2^-52)" % (worst, worst / EPS))
    assert worst <= 36 * EPS
    return st


def _lockstep(t, m, r, compacted=False):
    """TreeSearch.contemplate(r) launch by launch, the model beside it: the plain rollout where the roots are fresh, begin
    (the model reads the device's gumbel, prior, logits and root_value and must find its considered set, m_eff and n0),
    then the rounds; every node of every tree after every step."""
    net = t.net
    if r and t._fresh:
        m.select()
        t._rollout()
        ev = t.leaf.evaluate(net, rows=("value", "probs"))
        ValueTreeModel.backup(m, ev["value"].cpu().numpy(), ev["probs"].cpu().numpy())
        t._fresh = m.fresh = False
        r -= 1
        _check(t, m, compacted)
    if r == 0:
        return
    t._gumbel_begin(r)
    rec = _records(t)
    m.begin(r, records=rec)
    ref = m.device_records()
    for k in ("considered", "m_eff", "n0"):
        assert np.array_equal(rec[k], ref[k]), k
    assert np.array_equal(t._gumbel["table"].cpu().numpy(), m.table)
    K = t.leaves
    for k in [K] * (r // K) + [r % K] * (r % K > 0):
        b = t._round_buffers(k)
        t._gumbel_round(k)
        m.select_batch_gumbel(k)
        got = b["paths"].cpu().numpy()[:t.num_games * k * LP.PATH_BYTES].view(LP.PATH_DTYPE).reshape(t.num_games, k)
        want = m.path_records()
        m.backup_batch(b["out"]["value"].cpu().numpy(), b["out"]["probs"].cpu().numpy())
        for f in ("leaf", "depth", "flags"):
            assert np.array_equal(got[f], want[f]), (f, np.argwhere(got[f] != want[f])[:4].tolist())
        _check(t, m, compacted)


def _whole_search(name, case, dtype=torch.float32, holder=None):
    G, K, n, m_c, cap = case
    t, env = _search(case, _net(name, dtype))
    m = C.new_model(case)
    if holder is not None:
        holder["model"] = m
    _lockstep(t, m, n + 1)
    first = _check_finals(t, m)
    margins = [f[3] for f in m.finals()]
    act, bits = C.move_of(m)
    env.step_raw(action36_to_pairs(torch.as_tensor(act, device=DEV)).contiguous(), torch.as_tensor(bits, device=DEV))
    t._call("qttt_tree_sync", t.tree.data_ptr(), G, t.capacity, env.state.data_ptr())       # (round the host's node bound)
    t._fresh = True
    after, _ = tree_model.after_move(m.root_positions(), act, bits)
    m.sync(after)
    t.compact()
    m.compact()
    _check(t, m, compacted=True)
    _lockstep(t, m, n + 1, compacted=True)
    _check_finals(t, m)
    m.final_margins = [min(a, f[3]) for a, f in zip(margins, m.finals())]
    reused = sum(int(r["n0"].sum() > 1) for r in m.recs)
    return t, m, first, reused


# ---------------------------------------------------------------- 1. the Gumbel values, the prior, the considered set
@pytest.mark.parametrize("case", [C.CASES[2], C.CASES[3], C.CASES[4], C.CASES[7]], ids=str)
def test_gumbel_values_prior_and_considered_set(case):
    G, K, n, m_c, cap = case
    t, _ = _search(case, _net("random"))
    t.contemplate(1)
    t._gumbel_begin(n)
    t._gumbel_begin(n)                                       # the second move's draws: another index
    rec = _records(t)
    m = C.new_model(case)
    worst_g = worst_p = 0.0
    terminal = short = 0
    for g, stg in enumerate(m.games):
        root = stg["nodes"][stg["root"]]
        legal = [] if root.terminal else list(root.legal)
        ref = np.zeros(36)
        ref[legal] = GM.gumbel_of(GM.uniforms(C.SEED, C.OFFSET + g, 1, legal))
        err = np.abs(rec["gumbel"][g] - ref) / np.maximum(1.0, np.abs(ref))
        worst_g = max(worst_g, float(err.max()))
        assert (err <= 8 * EPS).all(), g
        prior = GM.softmax_legal(rec["logits"][g].astype(np.float64), legal)
        worst_p = max(worst_p, _rel(rec["prior"][g], prior))
        considered, m_eff = GM.top_considered(rec["gumbel"][g], rec["logits"][g], legal, m_c)      # on the device's bits
        assert rec["considered"][g] == considered and rec["m_eff"][g] == m_eff, g
        terminal += root.terminal
        short += 0 < len(legal) < m_c
    print("gumbel: largest error %.3g (%.2f * 2^-52); prior: largest relative difference %.3g (%.2f * 2^-52)"
          % (worst_g, worst_g / EPS, worst_p, worst_p / EPS))
    assert worst_p <= 36 * EPS
    ev = t._gumbel["out"]
    assert np.array_equal(rec["root_value"].view(np.uint32), ev["value"].cpu().numpy().view(np.uint32))
    assert np.array_equal(rec["logits"].view(np.uint32), ev["logits"].cpu().numpy().view(np.uint32))
    root_env = export(t._gumbel["root"])
    assert np.array_equal(root_env["board"], C.positions(G)["board"])
    assert G < 67 or (terminal > 0 and short > 0)


def test_the_positions_cover_what_a_root_can_be():
    """tests/gumbel_cases.py draws the roots with the oracle's uniform play, 0..7 plies deep as tree_harness.random_positions
    does on the device, so that tests/test_gumbel_cpu.py searches the same roots without one."""
    ref = C.positions(67)
    m = C.new_model(C.CASES[2])
    roots = [st["nodes"][st["root"]] for st in m.games]
    assert sum(r.terminal for r in roots) > 0 and sum(0 < len(r.legal) < 4 for r in roots) > 0
    assert sum(1 for g in range(67) if (np.asarray(ref["qmask"][g]) != 0).any()) > 0          # open entanglements at the root
    assert int(ref["n_moves"].min()) == 0 and int(ref["n_moves"].max()) >= 7


# ---------------------------------------------------------------- 2. and 4. whole searches, exactly
@pytest.mark.parametrize("case", C.CASES, ids=str)
@pytest.mark.parametrize("net", ["zero", "greedy", "counting"])
def test_whole_searches_under_the_exact_networks(net, case):
    t, m, first, reused = _whole_search(net, case)
    G, K, n, m_c, cap = case
    over = np.array([d["overflow"] for d in m.dump()])
    assert np.array_equal(t.root_stats()["overflow"].cpu().numpy(), over)
    assert cap is None or G < 67 or (over.any() and not over.all())
    assert G < 67 or n < 33 or cap is not None or reused > 0     # some second search started from a subtree with visits


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", C.RANDOM_CASES, ids=str)
def test_whole_searches_under_a_random_network(case, dtype):
    """As above.  Only here a search whose model met a root decision with a top-two gap below GAP may be left out when it
    differs; the last test of the file holds the count to LEFT_OUT_CAP."""
    LEFT_OUT["cases"] += case[0]
    holder = {}
    try:
        _whole_search("random", case, dtype, holder)
    except AssertionError:
        m = holder["model"]          # the margins of the decisions the model took, fed by the device, up to the difference
        close = np.minimum(m.min_margin(), [f[3] for f in m.finals()]) < C.GAP
        if not close.any():
            raise
        LEFT_OUT["left_out"] += case[0]


# ---------------------------------------------------------------- 3. the halving invariants on the device's result
@pytest.mark.parametrize("case", [c for c in C.CASES if c[4] is None and c[1] in (1, 8)], ids=str)
def test_root_visits_are_the_visit_tables(case):
    G, K, n, m_c, cap = case
    t, _ = _search(case, _net("random"))
    t.contemplate(n + 1)
    assert t._gumbel["sim"] == n and t.rollout_idx == n + 1 and t.gumbel_idx == 1
    rec, st = _records(t), {k: v.cpu().numpy() for k, v in t.root_stats().items()}
    assert not st["overflow"].any()
    for g in range(G):
        cons = [a for a in range(36) if (int(rec["considered"][g]) >> a) & 1]
        assert len(cons) == rec["m_eff"][g]
        since = st["N"][g].astype(np.int64) - rec["n0"][g]
        assert (since[[a for a in range(36) if a not in cons]] == 0).all(), g
        if cons:
            counts = np.zeros(len(cons), dtype=np.int64)                       # the sweeps of the sequence, position by position
            seq, i, c, L = GM.visit_sequence(len(cons), n), 0, len(cons), max(1, int(np.ceil(np.log2(max(len(cons), 2)))))
            if len(cons) == 1:
                counts[0] = n
            else:
                while i < n:
                    for _ in range(max(1, n // (L * c))):
                        counts[:max(0, min(c, n - i))] += 1
                        i += c
                    c = max(2, c // 2)
            assert sorted(since[cons].tolist()) == sorted(counts.tolist()), (g, seq)
            assert st["choose"][g] in cons and since[st["choose"][g]] == since[cons].max()
        else:
            assert st["choose"][g] == 255 and st["Ntot"][g] in (0, n + 1)


def test_contemplate_is_the_lockstep_search():
    """contemplate(n + 1) leaves the bytes that the launches of _lockstep leave."""
    case = C.CASES[2]
    a, _ = _search(case, _net("random"))
    b, _ = _search(case, _net("random"))
    a.contemplate(case[2] + 1)
    _lockstep(b, C.new_model(case), case[2] + 1)
    assert torch.equal(a.tree, b.tree) and torch.equal(a._gumbel["rec"], b._gumbel["rec"])
    assert a._bound == 1 + 2 * (case[2] + 1) >= int(a.nodes_used().max())


# ---------------------------------------------------------------- 5. the PUCT path is the parent's
@pytest.mark.parametrize("K", [1, 4])
def test_root_policy_puct_is_the_search_without_the_argument(K):
    G = 67
    net = _net("random")
    trees = []
    for kw in (dict(), dict(root_policy="puct", max_considered=3, c_visit=7.0, c_scale=2.0)):
        env = env_from_arrays(C.positions(G))
        t = TreeSearch(G, capacity=64, net=net, seed=C.SEED, board_offset=C.OFFSET, device=DEV, leaf_eval="value", leaves=K, **kw)
        t.tree = torch.full((tree_layout.tree_bytes(G, 64) + TAIL,), SENTINEL, dtype=torch.uint8, device=DEV)
        t.reset(env)
        t.contemplate(19)
        assert t._gumbel is None and t.gumbel_idx == 0 and "pi" not in t.root_stats()
        trees.append(t)
    assert torch.equal(trees[0].tree, trees[1].tree)
    assert torch.equal(trees[0].choose(), trees[1].choose())
    games, nodes, _, _ = tree_layout.decode(trees[0].tree.cpu().numpy(), G, 64)
    live = np.arange(64)[None, :] < games["used"][:, None]
    assert (nodes[live]["slots"]["N"] < 1 << 24).all() and (nodes[live]["Ntot"] < 1 << 24).all()


# ---------------------------------------------------------------- 6. SelfPlay
def test_selfplay_records_the_gumbel_choice_and_the_improved_policy():
    G, R_, K, seed = 5, 9, 4, 7
    net = _net("random")
    kw = dict(n_rollouts=R_, net=net, seed=seed, device=DEV, leaf_eval="value", leaves=K, root_policy="gumbel", max_considered=4)
    sp = SelfPlay(G, **kw)
    whole = sp.play()
    assert sp.tree.root_policy == "gumbel" and sp.tree.max_considered == 4 and sp.tree.gumbel_idx >= 5
    # the same game ply by ply: the row against root_stats() before the record, and against the plain record's other fields
    env = VecEnv(G, device=DEV, seed=seed)
    tree = TreeSearch(G, capacity=sp.capacity, net=net, seed=2 * seed + 1, device=DEV, leaf_eval="value", leaves=K,
                      root_policy="gumbel", max_considered=4)
    tree.reset(env)
    batch, plain = sp.new_batch(), sp.new_batch()
    plain_sp = SelfPlay(G, n_rollouts=R_, net=net, seed=seed, device=DEV, leaf_eval="value", leaves=K)
    rows = 0
    for ply in range(selfplay_model.ROWS):
        if ply < selfplay_model.ROWS - 1:
            tree.contemplate(R_)
        if ply < selfplay_model.ROWS - 1:
            st = {k: v.cpu().numpy() for k, v in tree.root_stats().items()}
        live_before = (batch.length.cpu().numpy() == ply) & (ply == 0 or batch.done[ply - 1].cpu().numpy() == 0)
        acts = sp.record(tree, ply, batch).clone()
        plain_sp.record(tree, ply, plain)
        for g in np.nonzero(live_before)[0]:
            if batch.done[ply, g]:
                continue
            rows += 1
            assert np.array_equal(batch.pi[ply, g].cpu().numpy().view(np.int64), st["pi"][g].view(np.int64)), (ply, g)
            assert int(batch.action36[ply, g]) == st["choose"][g] != 255, (ply, g)
            assert acts[g].tolist() == list(selfplay_model.oracle.ind2move(int(st["choose"][g]))), (ply, g)
        env.step_raw(acts)
        tree.sync(env)
    assert rows >= 5 * G
    for k in ("states", "mask", "done", "v", "length", "winner"):
        assert torch.equal(getattr(batch, k), getattr(plain, k)), k          # the existing record's rules
    for k in batch._FIELDS:
        assert torch.equal(getattr(batch, k), getattr(whole, k)), k          # play() is these calls
    length, winner = batch.length.cpu().numpy(), batch.winner.cpu().numpy()
    v = batch.v.cpu().numpy()
    for g in range(G):
        assert np.array_equal(v[:length[g], g], selfplay_model.value_targets(int(winner[g]), int(length[g])))
        assert batch.done[length[g] - 1, g] == 1 and not batch.done[:length[g] - 1, g].any()


# ---------------------------------------------------------------- 7. argument errors
def _begin(L, tree=0x1000, games=1, capacity=4, seed=0, move=0, offset=0, m=16, value=0x6000, logits=0x7000, rec=0x8000):
    return L.qttt_tree_gumbel_begin(tree, games, capacity, seed, move, offset, m, value, logits, rec, None)


def _select(L, tree=0x1000, games=1, capacity=4, seed=0, idx0=0, leaves=2, offset=0, c_puct=1.0, vloss=1.0, paths=0x2000,
            leaf=0x3000, rec=0x8000, table=0x9000, n=8, sim0=0, c_visit=50.0, c_scale=1.0):
    return L.qttt_tree_select_batch_gumbel(tree, games, capacity, seed, idx0, leaves, offset, c_puct, vloss, paths, leaf, rec,
                                           table, n, sim0, c_visit, c_scale, None)


def _root(L, tree=0x1000, rec=0x8000, games=1, capacity=4, c_visit=50.0, c_scale=1.0, choose=0xA000, pi=0xB000, q=0xC000):
    return L.qttt_tree_gumbel_root(tree, rec, games, capacity, c_visit, c_scale, choose, pi, q, None)


def test_return_codes_in_documented_order_without_device_work():
    """Fake addresses, never dereferenced: every call fails its checks first (or has no games)."""
    L = _native.lib()
    inf, nan = float("inf"), float("nan")
    sizes = (dict(games=-1), dict(capacity=0), dict(capacity=(1 << 30) + 1))
    for kw in sizes + (dict(offset=-1), dict(m=0), dict(m=37), dict(move=_native.TREE_MAX_GUMBEL)):
        assert _begin(L, **kw) == ERR_SIZE, kw
        assert _begin(L, **{"tree": None, "rec": None, "value": None, "logits": None, **kw}) == ERR_SIZE, kw
        assert _begin(L, **{"tree": 0x1001, "rec": 0x8008, **kw}) == ERR_SIZE, kw
    for kw in sizes + (dict(offset=-1), dict(leaves=0), dict(leaves=65), dict(idx0=(1 << 24) - 1), dict(vloss=-1.0),
                       dict(vloss=nan), dict(n=0), dict(sim0=-1), dict(sim0=7), dict(n=1), dict(c_visit=-1.0),
                       dict(c_visit=inf), dict(c_visit=nan), dict(c_scale=inf), dict(c_scale=nan)):
        assert _select(L, **kw) == ERR_SIZE, kw
        assert _select(L, **{"tree": None, "paths": None, "leaf": None, "rec": None, "table": None, **kw}) == ERR_SIZE, kw
        assert _select(L, **{"tree": 0x1001, "rec": 0x8008, "table": 0x9002, **kw}) == ERR_SIZE, kw
    for kw in sizes + (dict(c_visit=-1.0), dict(c_visit=nan), dict(c_scale=inf)):
        assert _root(L, **kw) == ERR_SIZE, kw
        assert _root(L, **{"tree": None, "rec": None, **kw}) == ERR_SIZE, kw
    assert _select(L, sim0=6, tree=None) == _select(L, n=2, tree=None) == ERR_NULL    # the last simulations of a budget
    assert _begin(L, games=0, tree=None, rec=None, value=None, logits=None) == 0
    assert _select(L, games=0, tree=None, paths=None, leaf=None, rec=None, table=None) == 0
    assert _root(L, games=0, tree=None, rec=None) == 0
    assert L.qttt_tree_root_states(None, 0, 4, None, None) == 0 and L.qttt_tree_root_states(None, -1, 4, None, None) == ERR_SIZE
    assert L.qttt_tree_root_states(None, 1, 4, 0x3000, None) == L.qttt_tree_root_states(0x1000, 1, 4, None, None) == ERR_NULL
    assert L.qttt_tree_root_states(0x1008, 1, 4, 0x3000, None) == L.qttt_tree_root_states(0x1000, 1, 4, 0x3008, None) == ERR_ACTION
    for kw in (dict(tree=None), dict(value=None), dict(logits=None), dict(rec=None)):
        assert _begin(L, **kw) == ERR_NULL, kw
        assert _begin(L, **{"tree": 0x1001, "rec": 0x8008, "value": 0x6002, **kw}) == ERR_NULL, kw        # nulls before alignment
    for kw in (dict(tree=None), dict(paths=None), dict(leaf=None), dict(rec=None), dict(table=None)):
        assert _select(L, **kw) == ERR_NULL, kw
        assert _select(L, **{"tree": 0x1001, "rec": 0x8008, "table": 0x9002, **kw}) == ERR_NULL, kw
    for kw in (dict(tree=None), dict(rec=None)):
        assert _root(L, **kw) == ERR_NULL, kw
        assert _root(L, **{"tree": 0x1001, "rec": 0x8008, "pi": 0xB004, **kw}) == ERR_NULL, kw
    for kw in (dict(tree=0x1008), dict(rec=0x8008), dict(value=0x6002), dict(logits=0x7001)):
        assert _begin(L, **kw) == ERR_ACTION, kw
    for kw in (dict(tree=0x1008), dict(paths=0x2008), dict(rec=0x8008), dict(rec=0x8004), dict(table=0x9002)):
        assert _select(L, **kw) == ERR_ACTION, kw
    for kw in (dict(tree=0x1008), dict(rec=0x8008), dict(pi=0xB004), dict(q=0xC004)):
        assert _root(L, **kw) == ERR_ACTION, kw
    rec_args = [0x1000, 1, 4, 0, 1, 1.0, 1.0, 0.0] + [0x10000 * (i + 2) for i in range(9)]
    rec = lambda *a, **kw: L.qttt_selfplay_record_gumbel(*(kw.get("args") or rec_args), *a, None)  # noqa: E731
    assert rec(0x8000, -1.0, 1.0) == rec(0x8000, 50.0, nan) == rec(None, -1.0, 1.0) == ERR_SIZE
    assert rec(None, 50.0, 1.0) == ERR_NULL and rec(0x8008, 50.0, 1.0) == ERR_ACTION
    bad_ply = list(rec_args)
    bad_ply[3] = 10
    assert rec(None, 50.0, 1.0, args=bad_ply) == ERR_SIZE
    ignored = list(rec_args)
    ignored[4], ignored[5] = 0, nan                              # n_rollouts and alpha are ignored
    assert rec(None, 50.0, 1.0, args=ignored) == ERR_NULL


def test_python_checks_come_before_any_launch():
    case = (5, 3, 16, 4, None)
    t, _ = _search(case, _net("random"))
    with pytest.raises(RuntimeError, match="contemplate"):
        t.root_stats()
    with pytest.raises(ValueError, match="budget"):
        t._gumbel_round(2)
    before = t.tree.clone()
    with pytest.raises(ValueError, match="capacity"):
        t.contemplate(t.capacity)
    assert torch.equal(t.tree, before) and t.gumbel_idx == 0
    t.contemplate(1)
    assert t._gumbel is None and t.gumbel_idx == 0            # the one rollout gave the priors: no budget remained
    t.contemplate(5)
    assert t._gumbel["n"] == 5 and t._gumbel["sim"] == 5 and t.gumbel_idx == 1 and sorted(t._tables) == [5]
    with pytest.raises(ValueError, match="budget"):
        t._gumbel_round(1)
    with pytest.raises(ValueError, match="n_rollouts"):
        SelfPlay(5, n_rollouts=1, net=_net("random"), device=DEV, leaf_eval="value", root_policy="gumbel")


# ---------------------------------------------------------------- the cap on what the random network's searches left out
def test_at_most_two_percent_of_the_random_networks_searches_were_left_out():
    assert LEFT_OUT["left_out"] <= C.LEFT_OUT_CAP * max(LEFT_OUT["cases"], 1), LEFT_OUT
