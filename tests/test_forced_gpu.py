"""Forced playouts and policy target pruning (include/qttt_tree_forced.h, TreeSearch(forced_playouts=k),
SelfPlay(prune_targets=True)) on the MI355X against tests/forced_model.py: whole searches in lockstep with the model fed by
the device's own evaluations and noised priors, every node and every path record after every round, through a move, a sync, a
compaction and a second search on the reused subtrees, also in a pool that overflows; the unchanged search without the
keyword; k = 0; the pruned record in play(), stream() and Reanalyser.run(); root_stats(); exact leaves and proofs.
There is no tolerance anywhere: the rules are +, *, / and comparisons in the model's order.  The cases are
tests/forced_model.py's."""
import numpy as np
import pytest
import torch

import forced_model as M
import gumbel_cases as C
import leaf_parallel_model as LP
import selfplay_model
import tree_layout
import tree_model
from tree_harness import DEV, SENTINEL, TAIL, env_from_arrays
from value_tree_model import ValueTreeModel

from qtttgym_amd import PolicyValueNet, Reanalyser, ReplayBuffer, SelfPlay, TreeSearch, VecEnv
from qtttgym_amd.actions import action36_to_pairs

pytestmark = pytest.mark.gpu
_NETS = {}


def _net(name="random"):
    if name not in _NETS:
        _NETS[name] = PolicyValueNet(C.net_state_dict(name), device=DEV)
    return _NETS[name]


def _search(case, **kw):
    G, K, noise, cap = case
    env = env_from_arrays(C.positions(G))
    capacity = M.capacity_of(case)
    kw.setdefault("forced_playouts", M.K_FORCED)
    t = TreeSearch(G, capacity=capacity, net=_net(), seed=M.SEED, board_offset=M.OFFSET, device=DEV, leaf_eval="value",
                   leaves=K, **kw)
    t.tree = torch.full((tree_layout.tree_bytes(G, capacity) + TAIL,), SENTINEL, dtype=torch.uint8, device=DEV)
    t.reset(env)
    return t, env


def _check(t, m, compacted=False):
    tree_layout.assert_tree_equals_model(t.tree.cpu().numpy(), t.num_games, t.capacity, m, SENTINEL, DEV, compacted=compacted)
    games, nodes, _, _ = tree_layout.decode(t.tree.cpu().numpy(), t.num_games, t.capacity)
    live = np.arange(t.capacity)[None, :] < games["used"][:, None]
    assert (nodes[live]["slots"]["N"] < 1 << 24).all() and (nodes[live]["Ntot"] < 1 << 24).all()      # nothing in flight


def _check_paths(t, m, b, k):
    got = b["paths"].cpu().numpy()[:t.num_games * k * LP.PATH_BYTES].view(LP.PATH_DTYPE).reshape(t.num_games, k)
    want = m.path_records()
    for f in ("leaf", "depth", "flags"):
        assert np.array_equal(got[f], want[f]), (f, np.argwhere(got[f] != want[f])[:4].tolist())
    on_path = np.arange(10)[None, None, :] < want["depth"][:, :, None]
    for f in ("node", "action"):
        assert np.array_equal(got[f][on_path], want[f][on_path]), f


def _check_root_stats(t, m):
    st = t.root_stats()
    assert st["forced"].dtype == torch.bool and st["n_pruned"].dtype == torch.int32
    assert np.array_equal(st["forced"].cpu().numpy(), m.forced_now())
    assert np.array_equal(st["n_pruned"].cpu().numpy(), m.pruned_now())
    return st


def _lockstep(t, m, noise, compacted=False):
    """SelfPlay._search on the device launch by launch, the model beside it: the plain rollout where the roots are fresh,
    the noise (the model adopts the device's priors), then the rounds through the forced select; every node of every tree
    and every path record after every step."""
    net = t.net
    assert t._fresh and m.fresh
    m.select()
    t._rollout()
    ev = t.leaf.evaluate(net, rows=("value", "probs"))
    ValueTreeModel.backup(m, ev["value"].cpu().numpy(), ev["probs"].cpu().numpy())
    t._fresh = m.fresh = False
    _check(t, m, compacted)
    if noise:
        applied = torch.zeros(t.num_games, dtype=torch.uint8, device=DEV)
        t.add_root_noise(*M.NOISE, applied=applied)
        m.adopt_priors(t.root_stats()["P"].cpu().numpy(), applied.cpu().numpy())
        _check(t, m, compacted)
    r, K = M.ROLLOUTS - 1, t.leaves
    for k in [K] * (r // K) + [r % K] * (r % K > 0):
        b = t._round_buffers(k)
        t._round(k)
        m.select_batch_forced(k)
        _check_paths(t, m, b, k)
        m.backup_batch(b["out"]["value"].cpu().numpy(), b["out"]["probs"].cpu().numpy())
        _check(t, m, compacted)


# ---------------------------------------------------------------- 1. whole searches in lockstep, bit for bit
@pytest.mark.parametrize("case", M.CASES, ids=str)
def test_whole_searches_in_lockstep_with_the_model(case):
    G, K, noise, cap = case
    t, env = _search(case)
    m = M.new_model(case)
    _lockstep(t, m, noise)
    first = _check_root_stats(t, m)
    assert t.rollout_idx == M.ROLLOUTS == m.k
    act, bits = M.move_of(m)
    env.step_raw(action36_to_pairs(torch.as_tensor(act, device=DEV)).contiguous(), torch.as_tensor(bits, device=DEV))
    t._call("qttt_tree_sync", t.tree.data_ptr(), G, t.capacity, env.state.data_ptr())       # (round the host's node bound)
    t._fresh = True
    after, _ = tree_model.after_move(m.root_positions(), act, bits)
    m.sync(after)
    t.compact()
    m.compact()
    _check(t, m, compacted=True)
    _lockstep(t, m, noise, compacted=True)
    second = _check_root_stats(t, m)
    over = np.array([d["overflow"] for d in m.dump()])
    assert np.array_equal(second["overflow"].cpu().numpy(), over)
    assert cap is None or (over.any() and not over.all())
    if G >= 3 and cap is None:
        assert m.forced_taken > 0                                 # the rule decided descents
        pruned = sum(int((s["n_pruned"] != s["N"]).any()) for s in (first, second))
        assert G < 130 or pruned == 2                             # and the prune took visits away


def test_contemplate_is_the_lockstep_search():
    """contemplate(), as SelfPlay._search calls it, leaves the bytes that the launches of _lockstep leave."""
    case = (130, 3, True, None)
    a, _ = _search(case)
    b, _ = _search(case)
    a.contemplate(1)
    a.add_root_noise(*M.NOISE)
    a.contemplate(M.ROLLOUTS - 1)
    _lockstep(b, M.new_model(case), True)
    assert torch.equal(a.tree, b.tree) and a.rollout_idx == b.rollout_idx == M.ROLLOUTS
    assert a._bound == 1 + 2 * M.ROLLOUTS >= int(a.nodes_used().max())


# ---------------------------------------------------------------- 2. without the keyword nothing changes; k = 0
@pytest.mark.parametrize("K", [1, 3])
def test_none_is_the_search_without_the_keyword_and_k_zero_equals_it(K):
    case = (130, K, True, None)
    trees = []
    for kw in (dict(forced_playouts=None), dict(forced_playouts=None, _omit=True), dict(forced_playouts=0.0)):
        if kw.pop("_omit", False):
            env = env_from_arrays(C.positions(130))
            t = TreeSearch(130, capacity=M.capacity_of(case), net=_net(), seed=M.SEED, board_offset=M.OFFSET, device=DEV,
                           leaf_eval="value", leaves=K)
            t.tree = torch.full((tree_layout.tree_bytes(130, t.capacity) + TAIL,), SENTINEL, dtype=torch.uint8, device=DEV)
            t.reset(env)
        else:
            t, _ = _search(case, **kw)
        t.contemplate(1)
        t.add_root_noise(*M.NOISE)
        t.contemplate(M.ROLLOUTS - 1)
        trees.append(t)
    none, omitted, zero = trees
    assert torch.equal(none.tree, omitted.tree)                          # byte-identical trees
    assert "forced" not in none.root_stats() and "n_pruned" not in omitted.root_stats()
    a, b = none.root_stats(), zero.root_stats()
    for k in ("N", "W", "Ntot", "P", "choose", "nodes_used"):
        assert torch.equal(a[k], b[k]), k
    assert not b["forced"].any() and torch.equal(b["n_pruned"], b["N"])
    if K > 1:                                                            # the same launches but for the select's entry
        assert torch.equal(none.tree, zero.tree)


def _selfplay(G=5, **kw):
    base = dict(n_rollouts=12, net=_net(), seed=7, device=DEV, leaf_eval="value", leaves=3)
    base.update(kw)
    return SelfPlay(G, **base)


def test_selfplay_without_the_keywords_and_k_zero_give_the_same_batches():
    kw = dict(root_noise=M.NOISE, sample_plies=2)
    plain = _selfplay(**kw).play()
    none = _selfplay(forced_playouts=None, prune_targets=False, **kw).play()
    zero = _selfplay(forced_playouts=0.0, **kw).play()                   # pruned record, nothing to prune
    unpruned = _selfplay(forced_playouts=0.0, prune_targets=False, **kw).play()
    for k in plain._FIELDS:
        assert torch.equal(getattr(plain, k), getattr(none, k)), k       # byte-identical batches
        assert torch.equal(getattr(plain, k), getattr(zero, k)), k
        assert torch.equal(getattr(plain, k), getattr(unpruned, k)), k


# ---------------------------------------------------------------- 3. the pruned record
class _Root:
    terminal = False

    def __init__(self, st, g, mask):
        self.legal = [a for a in range(36) if mask[a]]
        self.N, self.W = st["N"][g].tolist(), st["W"][g].tolist()
        self.P = {a: float(st["P"][g, a]) for a in self.legal}
        self.Ntot = int(st["Ntot"][g])


def _model_row(st, g, mask, sp, tree):
    return M.pruned_pi_row(_Root(st, g, mask), sp.forced_playouts, tree.c_puct, sp.n_rollouts, sp.alpha)


def test_play_records_the_models_pruned_rows_and_the_unpruned_moves():
    G = 5
    kw = dict(forced_playouts=2.0, root_noise=M.NOISE, sample_plies=2)
    sp = _selfplay(G, prune_targets=True, **kw)
    whole = sp.play(seed=11)
    assert sp.tree.forced_playouts == 2.0 and sp.prune_targets
    unpruned = _selfplay(G, prune_targets=False, **kw).play(seed=11)
    for k in ("states", "mask", "done", "v", "action36", "length", "winner", "actions"):
        assert torch.equal(getattr(whole, k), getattr(unpruned, k)), k   # forcing only: the same games, the same moves
    assert not torch.equal(whole.pi, unpruned.pi)                        # and the prune did change rows
    # the same game ply by ply: every row against the model's row from the root's statistics before the record
    env = VecEnv(G, device=DEV, seed=11)
    tree = TreeSearch(G, capacity=sp.capacity, net=sp.net, seed=2 * 11 + 1, device=DEV, leaf_eval="value", leaves=3,
                      forced_playouts=2.0)
    tree.reset(env)
    batch = sp.new_batch()
    rows = changed = 0
    for ply in range(selfplay_model.ROWS):
        if ply < selfplay_model.ROWS - 1:
            sp._search(tree)
            st = {k: v.cpu().numpy() for k, v in tree.root_stats().items()}
        live = (batch.length.cpu().numpy() == ply) & (ply == 0 or batch.done[ply - 1].cpu().numpy() == 0)
        acts = sp.record(tree, ply, batch).clone()
        pi, mask, done = batch.pi[ply].cpu().numpy(), batch.mask[ply].cpu().numpy(), batch.done[ply].cpu().numpy()
        for g in np.nonzero(live)[0]:
            if done[g]:
                continue
            rows += 1
            want = _model_row(st, g, mask[g], sp, tree)
            assert np.array_equal(pi[g].view(np.int64), want.view(np.int64)), (ply, g)
            assert np.array_equal(st["n_pruned"][g], M.pruned_visits(_Root(st, g, mask[g]), 2.0, tree.c_puct)), (ply, g)
            changed += not np.array_equal(want, selfplay_model.pi_row(st["N"][g], _Root(st, g, mask[g]).legal, sp.n_rollouts))
            assert abs(pi[g].sum() - 1.0) < 1e-12 and not (pi[g][st["N"][g] == 0] != 0).any()
        env.step_raw(acts)
        tree.sync(env)
    assert rows >= 5 * G and changed > 0
    for k in batch._FIELDS:
        assert torch.equal(getattr(batch, k), getattr(whole, k)), k      # play() is these calls


def test_a_stream_appends_pruned_rows_of_the_same_games():
    G, plies = 6, 7
    rings, sps = [], []
    for prune in (True, False):
        sp = _selfplay(G, forced_playouts=2.0, prune_targets=prune, root_noise=M.NOISE, sample_plies=2)
        ring = ReplayBuffer(32, device=DEV, seed=3)
        stats = sp.stream(ring, plies, seed=5)
        rings.append(ring.views())
        sps.append((sp, stats))
    a, b = rings
    written = int(a["written"].item())
    assert written == int(b["written"].item()) > 0 and int(sps[0][1].samples) == written
    for k in ("P", "Q", "mask", "v", "done"):
        assert torch.equal(a[k], b[k]), k                                # the same games in both rings
    n = min(written, 32)
    pi = a["pi"][:n]
    assert not torch.equal(pi, b["pi"][:n])                              # some row was pruned
    assert torch.allclose(pi.sum(1), torch.ones(n, dtype=torch.float64, device=DEV), atol=1e-12)
    assert bool((pi[b["pi"][:n] == 0] == 0).all())                       # the support lies inside the unpruned row's
    # the staging batch's row of a game in progress is the model's row of that ply's root statistics: one more ply by hand
    sp, _ = sps[0]
    st_ = sp._stream
    tree, batch = st_["tree"], st_["batch"]
    sp._search(tree)
    st = {k: v.cpu().numpy() for k, v in tree.root_stats().items()}
    length = batch.length.cpu().numpy().copy()
    sp.record(tree, None, batch, draw_index=st_["ply"])
    for g in range(G):
        t = int(length[g])
        row, mask = batch.pi[t, g].cpu().numpy(), batch.mask[t, g].cpu().numpy()
        assert np.array_equal(row.view(np.int64), _model_row(st, g, mask, sp, tree).view(np.int64)), g


def test_a_reanalysis_writes_pruned_rows():
    n = 8
    sp = _selfplay(16, forced_playouts=2.0)
    assert sp.prune_targets                                              # the default with forced_playouts
    ring = ReplayBuffer(64, device=DEV, seed=3)
    ring.add(sp.play(seed=2))
    ra = Reanalyser(sp, ring, n, seed=3)
    assert ra.recorder.forced_playouts == 2.0 and ra.recorder.prune_targets and ra.tree.forced_playouts == 2.0
    stats = ra.run(4)
    st = {k: v.cpu().numpy() for k, v in ra.tree.root_stats().items()}
    updated, slot = stats.updated.cpu().numpy(), stats.slot.cpu().numpy()
    assert updated.sum() >= n // 2 and slot.tolist() == list(range(4, 4 + n))
    pi, mask = ra.batch.pi[0].cpu().numpy(), ra.batch.mask[0].cpu().numpy()
    held = ring.views()["pi"].cpu().numpy()
    for g in range(n):
        if updated[g]:
            want = _model_row(st, g, mask[g], ra.recorder, ra.tree)
            assert np.array_equal(pi[g].view(np.int64), want.view(np.int64)), g
            assert np.array_equal(held[slot[g]].view(np.int64), want.view(np.int64)), g


# ---------------------------------------------------------------- 4. exact leaves and proofs
def test_exact_leaves_and_proofs_go_on_under_the_forced_select():
    """tests/prove_model.py's exact model has no root rule, so the reference is the device's own plain search: identical
    where no action is ever forced (k = 0); and at k = 2 the search composes: every round solved, backed up and proved."""
    case = (130, 3, False, None)
    kw = dict(exact_from=7, prove=True)
    plain, _ = _search(case, forced_playouts=None, **kw)
    zero, _ = _search(case, forced_playouts=0.0, **kw)
    two, _ = _search(case, forced_playouts=2.0, **kw)
    for t in (plain, zero, two):
        t.contemplate(M.ROLLOUTS)
    assert torch.equal(plain.tree, zero.tree)
    a, b = plain.root_stats(), zero.root_stats()
    for k in ("N", "W", "proven", "root_solved"):
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(a["q_exact"].nan_to_num(7.0), b["q_exact"].nan_to_num(7.0))
    st = two.root_stats()
    games, nodes, _, _ = tree_layout.decode(two.tree.cpu().numpy(), 130, two.capacity)
    live = np.arange(two.capacity)[None, :] < games["used"][:, None]
    assert (nodes[live]["slots"]["N"] < 1 << 24).all() and (nodes[live]["Ntot"] < 1 << 24).all()
    assert torch.equal(st["N"].sum(1), st["Ntot"]) and int(two.solved_count().sum()) > 0
    assert not torch.equal(st["N"], a["N"]) and bool(st["proven"].any())  # the rule moved visits, the proofs went on
