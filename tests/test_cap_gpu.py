"""Playout cap randomisation (include/qttt_tree_subset.h, include/qttt_selfplay_cap.h, TreeSearch.contemplate(games=),
SelfPlay(playout_cap=)) on the MI355X, bit for bit: a subset round against the existing full-batch round on a tree of
identical bytes (listed games equal, the others untouched, rows packed densely), also in a pool that overflows and
through a sync, a compaction and a second search; the noise of a subset; the capped record against the existing stream
record; play() and stream() against tests/cap_model.py's composition of the existing entries; the equivalences with the
search without the keyword; the size of the network launch.  There is no tolerance anywhere."""
import numpy as np
import pytest
import torch

import cap_model as M
import gumbel_cases as C
from tree_harness import DEV, env_from_arrays

from qtttgym_amd import PolicyValueNet, ReplayBuffer, SelfPlay, TreeSearch, VecEnv, _native

pytestmark = pytest.mark.gpu
SEED, OFFSET, NOISE = 5, 17, (0.25, 0.3)
_NETS = {}


def _net():
    if "random" not in _NETS:
        _NETS["random"] = PolicyValueNet(C.net_state_dict("random"), device=DEV)
    return _NETS["random"]


def _tree(G, K, capacity):
    t = TreeSearch(G, capacity=capacity, net=_net(), seed=SEED, board_offset=OFFSET, device=DEV, leaf_eval="value", leaves=K)
    t.reset(env_from_arrays(C.positions(G)))                     # roots 0..7 plies deep
    return t


def _ids(ids):
    return torch.as_tensor(ids, dtype=torch.int32, device=DEV)


def _full_round(t, k, forced_k):
    """The existing full-batch round, the entries called by name so that the root rule is the test's choice."""
    b = t._round_buffers(k)
    b["paths"].zero_()
    b["leaf"].state.zero_()
    args = (t.tree.data_ptr(), t.num_games, t.capacity, t.seed, t.rollout_idx, k, t.board_offset, t.c_puct, t.virtual_loss,
            b["paths"].data_ptr(), b["leaf"].state.data_ptr())
    if forced_k < 0:
        t._call("qttt_tree_select_batch", *args)
    else:
        t._call("qttt_tree_select_batch_forced", *args, forced_k)
    snap = {"paths": b["paths"].clone(), "leaf": b["leaf"].state.clone()}
    b["leaf"].evaluate(t.net, out=b["out"])
    t._call("qttt_tree_backup_batch", t.tree.data_ptr(), t.num_games, t.capacity, k, b["paths"].data_ptr(),
            b["out"]["value"].data_ptr(), b["out"]["probs"].data_ptr())
    t.rollout_idx += k
    return snap


def _subset_round(t, k, ids, forced_k):
    full = t._round_buffers(k)                                   # the subset's buffers are views of this storage
    full["paths"].zero_()
    full["leaf"].state.zero_()
    n = len(ids)
    t._round(k, ids=(_ids(ids), n), forced=float(forced_k))
    if not n:
        return None
    b = t._subset_rounds[(n, k)]
    assert b["leaf"].num_envs == n * k                           # the network launch has n_ids * k rows
    assert b["out"]["value"].shape == (n * k,) and b["out"]["probs"].shape == (n * k, 36)
    return {"paths": b["paths"].clone(), "leaf": b["leaf"].state.clone()}


def _listed(G, ids):
    m = torch.zeros(G, dtype=torch.bool, device=DEV)
    m[torch.as_tensor(ids, dtype=torch.int64, device=DEV)] = True
    return m


def _planes(state, n):
    w = state.view(torch.int64)
    stride = w.numel() // 2
    return w[:n], w[stride:stride + n]


def _assert_subset_equals_full(a, b, base, ids, k, snap_a, snap_b, what):
    G, cap = a.num_games, a.capacity
    listed = _listed(G, ids)
    for va, vb, v0, part in zip(M.game_views(a.tree, G, cap), M.game_views(b.tree, G, cap), M.game_views(base, G, cap),
                                ("header", "nodes", "priors")):
        assert torch.equal(vb[listed], va[listed]), (what, part, "listed")
        assert torch.equal(vb[~listed], v0[~listed]), (what, part, "unlisted")
    if not ids:
        return
    rows = (torch.as_tensor(ids, device=DEV)[:, None] * k + torch.arange(k, device=DEV)[None, :]).reshape(-1)
    pa = snap_a["paths"][:G * k * 64].view(G * k, 64)
    pb = snap_b["paths"][:len(ids) * k * 64].view(len(ids) * k, 64)
    assert torch.equal(pb, pa[rows]), (what, "paths")
    for xa, xb in zip(_planes(snap_a["leaf"], G * k), _planes(snap_b["leaf"], len(ids) * k)):
        assert torch.equal(xb, xa[rows]), (what, "leaves")
    if len(ids) == G:                                            # all listed: the existing entries' bytes, all of them
        assert torch.equal(a.tree, b.tree), what
        assert torch.equal(snap_a["paths"][:G * k * 64], snap_b["paths"][:G * k * 64]), what
        assert torch.equal(snap_a["leaf"], snap_b["leaf"]), what


def _prepared(G, K, capacity, noise, rollouts):
    """Two trees of identical bytes whose roots have priors (noised or not) and some statistics."""
    a = _tree(G, K, capacity)
    a.contemplate(1)
    if noise:
        a.add_root_noise(*NOISE)
    a.contemplate(rollouts)
    b = _tree(G, K, capacity)
    b.tree.copy_(a.tree)
    b.rollout_idx, b.noise_idx, b._bound, b._fresh = a.rollout_idx, a.noise_idx, a._bound, a._fresh
    return a, b


# ---------------------------------------------------------------- 1. a subset round equals the full round
@pytest.mark.parametrize("K", [1, 3, 8])
@pytest.mark.parametrize("G", [1, 3, 130])
def test_a_subset_round_equals_the_full_round_on_the_listed_games(G, K):
    capacity = 2 + 2 * (1 + K + 2 * K)
    for noise in (False, True):
        a, b = _prepared(G, K, capacity, noise, K)
        base, idx0 = a.tree.clone(), a.rollout_idx
        for forced_k in (-1.0, 0.0, 2.0):
            a.tree.copy_(base)
            a.rollout_idx = idx0
            snap_a = _full_round(a, K, forced_k)
            for name, ids in M.subsets(G).items():
                b.tree.copy_(base)
                b.rollout_idx = idx0
                snap_b = _subset_round(b, K, ids, forced_k)
                assert b.rollout_idx == idx0 + K                 # the index advances as for a full call, also for no games
                _assert_subset_equals_full(a, b, base, ids, K, snap_a, snap_b, (noise, forced_k, name))
    games = a.tree[:G * M.GAME_BYTES].view(G, -1)[:, 16:20].contiguous().view(torch.int32)
    assert not bool((games & 1).any())                           # no pool overflowed here


def test_a_subset_round_in_a_pool_that_overflows():
    G, K, capacity = 130, 3, 12
    a, b = _prepared(G, K, capacity, True, 0)
    for t in (a, b):
        t._bound = 0                                             # the host's bound is not what is tested
    base, idx0 = a.tree.clone(), a.rollout_idx
    for r in range(3):                                           # three rounds: the pools of the deeper roots run out
        ids = M.subsets(G)["every other"]
        before = b.tree.clone()
        a.tree.copy_(before)
        a.rollout_idx = b.rollout_idx
        snap_a = _full_round(a, K, 2.0)
        snap_b = _subset_round(b, K, ids, 2.0)
        _assert_subset_equals_full(a, b, before, ids, K, snap_a, snap_b, r)
    flags = b.tree[:G * M.GAME_BYTES].view(G, -1)[:, 16:20].contiguous().view(torch.int32).view(G)
    over = (flags & 1) != 0
    assert bool(over[::2].any()) and not bool(over[1::2].any()) and not bool(over[::2].all())


def test_a_subset_search_through_sync_compact_and_a_second_search():
    G, K = 130, 3
    capacity = 64
    a, b = _prepared(G, K, capacity, True, 0)
    ids = M.subsets(G)["one per workgroup"]
    env_a, env_b = env_from_arrays(C.positions(G)), env_from_arrays(C.positions(G))
    for stage in range(2):
        base = b.tree.clone()
        a.tree.copy_(base)
        a.rollout_idx = b.rollout_idx
        a.contemplate(2 * K + 1)                                 # the existing rounds, all games
        b.contemplate(2 * K + 1, games=_ids(ids))                # the subset's, through the public call
        assert a.rollout_idx == b.rollout_idx and a._bound == b._bound
        listed = _listed(G, ids)
        for va, vb, v0 in zip(M.game_views(a.tree, G, capacity), M.game_views(b.tree, G, capacity),
                              M.game_views(base, G, capacity)):
            assert torch.equal(vb[listed], va[listed]) and torch.equal(vb[~listed], v0[~listed]), stage
        if stage == 0:                                           # a move in every game, then the second search
            acts = b.choose()
            b.tree.copy_(a.tree)                                 # from here both hold the fully searched trees
            for t, env in ((a, env_a), (b, env_b)):
                from qtttgym_amd.actions import action36_to_pairs
                env.step_raw(action36_to_pairs(acts).contiguous())       # 255 at a terminal root: a noop
                t.sync(env)
                t.compact()
                t.contemplate(1)
                t.add_root_noise(*NOISE)
            assert torch.equal(a.tree, b.tree)


# ---------------------------------------------------------------- 2. the noise of a subset
@pytest.mark.parametrize("G", [3, 130])
def test_the_noise_of_a_subset_is_the_full_calls_noise_of_those_games(G):
    a, b = _prepared(G, 3, 40, False, 3)
    base = a.tree.clone()
    noise_a = torch.full((G, 36), -7.0, dtype=torch.float64, device=DEV)
    applied_a = torch.full((G,), 9, dtype=torch.uint8, device=DEV)
    a.add_root_noise(*NOISE, noise=noise_a, applied=applied_a)
    assert bool(applied_a.bool().any())
    for name, ids in M.subsets(G).items():
        b.tree.copy_(base)
        b.noise_idx = 0
        noise_b = torch.full((G, 36), -7.0, dtype=torch.float64, device=DEV)
        applied_b = torch.full((G,), 9, dtype=torch.uint8, device=DEV)
        mask = _listed(G, ids).cpu()
        b.add_root_noise(*NOISE, noise=noise_b, applied=applied_b, games=mask if name != "last" else _ids(ids))
        assert b.noise_idx == 1
        listed = mask.to(DEV)
        for va, vb, v0 in zip(M.game_views(a.tree, G, 40), M.game_views(b.tree, G, 40), M.game_views(base, G, 40)):
            assert torch.equal(vb[listed], va[listed]) and torch.equal(vb[~listed], v0[~listed]), name
        assert torch.equal(noise_b[listed], noise_a[listed]) and torch.equal(applied_b[listed], applied_a[listed]), name
        assert bool((noise_b[~listed] == -7.0).all()) and bool((applied_b[~listed] == 9).all()), name


# ---------------------------------------------------------------- 3. the capped record
def _selfplay(G=6, **kw):
    base = dict(n_rollouts=12, net=_net(), seed=7, device=DEV, leaf_eval="value", leaves=3, value_targets=(1.0, -1.0))
    base.update(kw)
    return SelfPlay(G, **base)


@pytest.mark.parametrize("prune", [False, True])
def test_the_capped_record_against_the_stream_record(prune):
    G = 130
    kw = dict(forced_playouts=2.0, prune_targets=prune, root_noise=NOISE, sample_plies=3)
    sp = _selfplay(G, **kw)
    env = env_from_arrays(C.positions(G))                        # roots 0..7 plies deep: some are terminal
    tree = TreeSearch(G, capacity=80, seed=3, device=DEV, **sp.search_kwargs())
    tree.reset(env)
    tree.contemplate(1)
    tree.add_root_noise(*NOISE)
    tree.contemplate(11)
    full = torch.as_tensor(M.full_mask(3, 0, G, 0, 0.5), device=DEV)
    assert 0 < int(full.sum()) < G
    for length in (0, 2):                                        # the rows written are the games' own: row 0, then row 2
        want, got = sp.new_batch(), sp.new_batch()
        for b in (want, got):
            b.length.fill_(length)
            b.v.fill_(0.5)
            b.actions.fill_(77)
            # rows 0..length-1 as earlier plies recorded them: states with one move played (odd), then two (even)
            words = b.states.view(torch.int64).view(M.ROWS, 2, -1)
            for r in range(length):
                words[r, 0, :G] = (r + 1) << 40
        before = M.clone_batch(sp, got)
        sp.record(tree, None, want, draw_index=4)
        acts = sp.record_capped(tree, got, full, draw_index=4)
        term = want.done[length] != 0
        assert 0 < int(term.sum()) < G
        rec = full.bool() | term
        assert torch.equal(acts, want.actions)                   # every game's move is the record's, fast games too
        for f, _ in got._ROWS.items():
            if f == "v":
                continue
            assert torch.equal(getattr(got, f)[:, rec], getattr(want, f)[:, rec]), f
            assert torch.equal(getattr(got, f)[:, ~rec], getattr(before, f)[:, ~rec]), f      # a fast game: nothing but its move
        for (gw, ww, bw) in zip(M.state_words(got.states, G), M.state_words(want.states, G), M.state_words(before.states, G)):
            assert torch.equal(gw[:, rec], ww[:, rec]) and torch.equal(gw[:, ~rec], bw[:, ~rec])
        assert torch.equal(got.length[rec], want.length[rec]) and torch.equal(got.length[~rec], before.length[~rec])
        assert torch.equal(got.winner[term], want.winner[term]) and torch.equal(got.winner[~term], before.winner[~term])
        # v: untouched but in the finished games, whose rows are signed by their states' side to move
        assert torch.equal(got.v[:, ~term], before.v[:, ~term])
        P = M.state_words(got.states, G)[0].cpu().numpy().view(np.uint64)
        v, v_index = got.v.cpu().numpy(), want.v.cpu().numpy()
        for g in np.nonzero(term.cpu().numpy())[0]:
            assert np.array_equal(v[:length + 1, g].view(np.uint32), M.backfill(P[:length + 1, g], v_index[0, g]).view(np.uint32)), g
            assert np.array_equal(v[length + 1:, g], np.full(M.ROWS - length - 1, 0.5, np.float32))


# ---------------------------------------------------------------- 4. play() and stream() against the model
def _assert_batches_equal(got, want, what=""):
    for f in M.FIELDS:
        assert torch.equal(getattr(got, f), getattr(want, f)), (what, f)


@pytest.mark.parametrize("kw", [dict(), dict(forced_playouts=2.0, root_noise=NOISE, sample_plies=2),
                                dict(root_noise=NOISE, value_mix=0.5, exact_targets=7, compact=True)], ids=str)
def test_play_is_the_models_composition_of_the_existing_entries(kw):
    G, cap = 6, (0.5, 4)
    sp = _selfplay(G, playout_cap=cap, **kw)
    got = sp.play(seed=11)
    assert sp.playout_cap == cap
    m = M.CapModel(G, 11, cap, **{k: getattr(sp, k) for k in ("n_rollouts", "net", "leaf_eval", "leaves", "compact")},
                   seed=7, device=DEV, value_targets=(1.0, -1.0),
                   **{k: v for k, v in kw.items() if k not in ("exact_targets", "compact")})
    want = m.play()
    if "exact_targets" in kw:
        want.exact = want.exact_targets(kw["exact_targets"], True)
    if "value_mix" in kw:
        want.value_targets("mix", kw["value_mix"], exact=getattr(want, "exact", None))
    _assert_batches_equal(got, want, kw)
    length = got.length.cpu().numpy()
    plies = (M.state_words(got.states, G)[0].cpu().numpy().view(np.uint64)[length - 1, np.arange(G)] >> np.uint64(40)) & np.uint64(15)
    assert (length >= 1).all() and (length <= plies + 1).all() and (length < plies + 1).any()     # plies went unrecorded
    done = got.done.cpu().numpy()
    assert all(done[length[g] - 1, g] == 1 and not done[:length[g] - 1, g].any() for g in range(G))
    # v: the outcome seen by the side to move of every recorded state
    if "value_mix" not in kw:
        P, v = M.state_words(got.states, G)[0].cpu().numpy().view(np.uint64), got.v.cpu().numpy()
        for g in range(G):
            n = length[g]
            assert np.array_equal(v[:n, g], M.backfill(P[:n, g], v[n - 1, g] * (-1.0 if M.moves_played(P[n - 1, g]) & np.uint64(1) else 1.0)))


def test_a_game_whose_plies_were_all_fast_yields_its_terminal_row_alone():
    G = 6
    sp = _selfplay(G, playout_cap=(0.5, 4))
    got = sp.play(seed=11)
    # the same games with a draw that makes no ply full: p so small that no hash is below it
    sp2 = _selfplay(G, playout_cap=(2.0 ** -60, 4))
    alone = sp2.play(seed=11)
    assert bool((alone.length == 1).all()) and bool((alone.done[0] == 1).all()) and bool((alone.done[1:] == 0).all())
    assert bool((alone.action36[0] == 255).all()) and bool((alone.pi[0] == 1.0 / 36.0).all())
    P = M.state_words(alone.states, G)[0].cpu().numpy().view(np.uint64)
    w = alone.winner.cpu().numpy()
    v0 = np.where(w > 0, 1.0, np.where(w == 0, -1.0, 0.0)).astype(np.float32)
    for g in range(G):
        assert np.array_equal(alone.v[:1, g].cpu().numpy().view(np.uint32), M.backfill(P[:1, g], v0[g]).view(np.uint32)), g
    assert bool((alone.v[1:] == 0).all()) and int(got.length.sum()) > G


def test_a_stream_fills_the_ring_as_the_models_composition_does():
    G, cap, plies = 6, (0.5, 4), 14
    kw = dict(forced_playouts=2.0, root_noise=NOISE, sample_plies=2)
    sp = _selfplay(G, playout_cap=cap, **kw)
    ring = ReplayBuffer(64, device=DEV, seed=3)
    stats = sp.stream(ring, plies, seed=5)
    m = M.CapModel(G, 5, cap, n_rollouts=12, net=_net(), seed=7, device=DEV, leaf_eval="value", leaves=3,
                   value_targets=(1.0, -1.0), **kw)
    model_ring = ReplayBuffer(64, device=DEV, seed=3)
    for _ in range(plies):
        m.stream_ply(model_ring)
    a, b = ring.views(), model_ring.views()
    written = int(a["written"].item())
    assert written == int(b["written"].item()) == int(stats.samples) > 0
    for k in ("P", "Q", "pi", "mask", "v", "done"):
        assert torch.equal(a[k], b[k]), k                        # the ring's contents
    _assert_batches_equal(sp._stream["batch"], m.batch, "staging")
    assert torch.equal(sp._stream["games_done"], m.st["games_done"]) and torch.equal(sp._stream["tally"], m.st["tally"])
    a, b = sp.tree.root_stats(), m.tree.root_stats()
    assert all(torch.equal(a[k], b[k]) for k in ("N", "W", "P", "Ntot", "nodes_used")) and int(stats.games.sum()) > 0
    assert written < int(stats.games.sum()) * 10                 # fewer rows than plies: plies went unrecorded


# ---------------------------------------------------------------- 5. equivalences
@pytest.mark.parametrize("kw", [dict(), dict(forced_playouts=2.0, root_noise=NOISE, sample_plies=2, value_mix=0.5)], ids=str)
def test_every_ply_full_is_the_batch_without_the_keyword(kw):
    plain = _selfplay(**kw)
    want = plain.play(seed=11)
    capped = _selfplay(playout_cap=(1.0, 12), **kw)
    got = capped.play(seed=11)
    _assert_batches_equal(got, want)
    a, b = capped.tree.root_stats(), plain.tree.root_stats()
    assert all(torch.equal(a[k], b[k]) for k in ("N", "W", "P", "Ntot", "nodes_used"))
    # and the streams fill their rings alike
    rings = []
    for cap in (None, (1.0, 3)):
        sp = _selfplay(playout_cap=cap, **kw)
        ring = ReplayBuffer(64, device=DEV, seed=3)
        sp.stream(ring, 12, seed=5)
        rings.append(ring.views())
    for k in ("P", "Q", "pi", "mask", "v", "done", "written"):
        assert torch.equal(rings[0][k], rings[1][k]), k


def test_none_is_the_call_sequence_without_the_keyword(monkeypatch):
    kw = dict(forced_playouts=2.0, root_noise=NOISE, sample_plies=2)
    calls = {}
    for name, extra in (("omitted", {}), ("none", dict(playout_cap=None))):
        sp = _selfplay(**kw, **extra)
        log = calls[name] = []
        for obj in (SelfPlay, TreeSearch, VecEnv):
            orig = obj._call
            monkeypatch.setattr(obj, "_call", lambda self, entry, *a, _o=orig, _l=log: (_l.append(entry), _o(self, entry, *a))[1])
        batch = sp.play(seed=11)
        ring = ReplayBuffer(64, device=DEV, seed=3)
        sp.stream(ring, 3, seed=5)
        monkeypatch.undo()
        calls[name + " bytes"] = (batch, sp.tree.root_stats(), ring.views())
    assert calls["omitted"] == calls["none"] and len(calls["none"]) > 100
    assert not any("subset" in c or "capped" in c for c in calls["none"])
    (b0, t0, r0), (b1, t1, r1) = calls["omitted bytes"], calls["none bytes"]
    _assert_batches_equal(b0, b1)
    assert all(torch.equal(t0[k], t1[k]) for k in ("N", "W", "P", "Ntot", "nodes_used"))
    assert all(torch.equal(r0[k], r1[k]) for k in ("P", "Q", "pi", "v", "written"))


# ---------------------------------------------------------------- 6. the rows of the network launch
def test_the_network_launch_of_a_capped_ply_has_the_groups_rows(monkeypatch):
    G, K = 40, 8
    sp = _selfplay(G, playout_cap=(0.25, 4), leaves=K, n_rollouts=17)
    seen = []
    orig = VecEnv.evaluate
    monkeypatch.setattr(VecEnv, "evaluate", lambda self, net, **kw: (seen.append(self.num_envs), orig(self, net, **kw))[1])
    ring = ReplayBuffer(64, device=DEV, seed=3)
    sp.stream(ring, 1, seed=5)
    full = M.full_mask(2 * 5 + 1, 0, G, 0, 0.25)
    n_full, n_fast = int(full.sum()), G - int(full.sum())
    assert 0 < n_full < n_fast
    # the fast group: 3 rollouts in one round of 3; the full group: 16 in two rounds of 8
    assert seen == [n_fast * 3, n_full * 8, n_full * 8]
    assert sp.tree.rollout_idx == 17 and (n_full, 8) in sp.tree._subset_rounds and (n_fast, 3) in sp.tree._subset_rounds
    assert sp.tree._subset_rounds[(n_full, 8)]["leaf"].num_envs == n_full * 8
    # refusals of the subset search on a tree that cannot do it
    for bad in (dict(root_policy="gumbel"), dict(exact_from=7), dict(exact_from=7, prove=True)):
        t = TreeSearch(4, capacity=64, net=_net(), device=DEV, leaf_eval="value", **bad)
        t.reset(VecEnv(4, device=DEV))
        with pytest.raises(ValueError, match="index their records by game"):
            t.contemplate(2, games=[True, False, True, False])
    t = TreeSearch(4, capacity=64, net=_net(), device=DEV, leaf_eval="value", leaves=2)
    t.reset(VecEnv(4, device=DEV))
    with pytest.raises(ValueError, match="ascending, distinct"):
        t.contemplate(2, games=torch.tensor([2, 1], dtype=torch.int32))
    with pytest.raises(ValueError, match="mask of shape"):
        t.contemplate(2, games=[True, False])
    base = t.tree.clone()
    t.contemplate(3, games=[False] * 4)                          # nobody listed: not a byte, but the index moves on
    assert torch.equal(t.tree, base) and t.rollout_idx == 3
    assert _native.SELFPLAY_CAP_BASE == 0xA0000000
