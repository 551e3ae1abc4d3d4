"""qtttgym_amd.SelfPlay on the MI355X (include/qttt_selfplay.h): whole games bit for bit against the Python model
(tests/selfplay_model.py), play() against a hand loop of the public calls it replaces (uniform and network search), the
batch's invariants, compaction, seeds, flat(), and the alpha != 1 targets against the reference's numpy expression."""
import numpy as np
import pytest
import torch

import selfplay_model
import tree_layout
from tree_harness import DEV, env_from_arrays, export, random_positions
from tree_harness import net as _net

from qtttgym_amd import SelfPlay, TreeSearch, VecEnv
from qtttgym_amd.actions import action36_to_pairs, legal_mask_to_bool

pytestmark = pytest.mark.gpu
ROWS = 10
KEYS = ("pi", "mask", "done", "v", "action36", "length", "winner", "actions")


def _host(batch):
    out = {k: getattr(batch, k).cpu().numpy() for k in KEYS}
    out["states"] = batch.states.cpu().numpy()
    return out


def _planes(states, G):
    """u8[rows, qttt_state_bytes(G)] -> the games' plane words u64[rows, 2, G] and the padding u64[rows, 2, stride - G]."""
    w = np.ascontiguousarray(states).view(np.uint64).reshape(states.shape[0], 2, -1)
    return w[:, :, :G], w[:, :, G:]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same_bytes(a, b):
    ha, hb = _host(a), _host(b)
    return all(np.array_equal(_bits(ha[k]), _bits(hb[k])) for k in ha)


# ---------------------------------------------------------------- whole games against the model
@pytest.mark.parametrize("G", [1, 3, 65])
def test_whole_games_match_the_model_bit_for_bit(G):
    R, S, seed = 8, 2, 7
    sp = SelfPlay(G, n_rollouts=R, num_simulations=S, seed=seed, device=DEV)
    dev = _host(sp.play())
    ref, ref_env = selfplay_model.play(G, R, S, seed=seed)
    for k in KEYS:
        assert np.array_equal(_bits(dev[k]), _bits(ref[k])), (k, np.argwhere(_bits(dev[k]) != _bits(ref[k]))[:6])
    words, padding = _planes(dev["states"], G)
    assert not padding.any()
    for t in range(ROWS):
        live = [g for g in range(G) if ref["recs"][t][g] is not None]
        assert live == [g for g in range(G) if ref["length"][g] > t]
        if live:
            P, Q = tree_layout.pack_positions([ref["recs"][t][g] for g in live], DEV)
            assert np.array_equal(words[t, 0, live], P) and np.array_equal(words[t, 1, live], Q), t
        rest = [g for g in range(G) if g not in live]
        assert not words[t][:, rest].any(), t
    ex = export(sp.env)
    for key, val in (("board", ref_env.board), ("moves", ref_env.moves), ("n_moves", ref_env.n_moves),
                     ("qmask", ref_env.qmask), ("n_q", ref_env.n_q)):
        assert np.array_equal(ex[key], val.astype(ex[key].dtype)), key
    assert 5 <= int(ref["length"].min()) - 1 and int(ref["length"].max()) <= ROWS


# ---------------------------------------------------------------- play() against the calls it replaces
def _hand_loop(G, R, S, net, seed):
    """play_game with the public calls that existed before SelfPlay: a list of per-ply dicts and the final env."""
    env = VecEnv(G, device=DEV, seed=seed)
    tree = TreeSearch(G, capacity=1 + ROWS * (2 * R + 1), num_simulations=S, net=net, seed=2 * seed + 1, device=DEV)
    tree.reset(env)
    finished = torch.zeros(G, dtype=torch.bool, device=DEV)
    rows = []
    for ply in range(ROWS):
        if ply < ROWS - 1:
            tree.contemplate(R)
        info = env.node_info(python_key=False)
        st = tree.root_stats()
        choose = tree.choose()
        live, terminal = ~finished, info["terminal"].clone()
        act = torch.where(live & ~terminal, choose, torch.full_like(choose, 255))
        rows.append({"state": env.state.clone(), "N": st["N"], "legal": info["legal"].clone(), "live": live,
                     "terminal": terminal, "action36": act})
        env.step_raw(action36_to_pairs(act).contiguous())
        finished = finished | terminal
        tree.sync(env)
    return rows, env


def _assert_play_is_the_hand_loop(G, R, S, net, seed):
    sp = SelfPlay(G, n_rollouts=R, num_simulations=S, net=net, seed=seed, device=DEV)
    batch = sp.play()
    rows, env = _hand_loop(G, R, S, net, seed)
    dev = _host(batch)
    words, _ = _planes(dev["states"], G)
    length = np.zeros(G, dtype=np.int64)
    for t, row in enumerate(rows):
        live = row["live"].cpu().numpy()
        terminal = row["terminal"].cpu().numpy()
        length += live
        ref_words, _ = _planes(row["state"].cpu().numpy()[None], G)
        assert np.array_equal(words[t][:, live], ref_words[0][:, live]), t
        assert not words[t][:, ~live].any(), t
        assert np.array_equal(dev["action36"][t][live], row["action36"].cpu().numpy()[live]), t
        assert np.array_equal(dev["done"][t], (live & terminal).astype(np.uint8)), t
        N = row["N"].cpu().numpy()
        legal = legal_mask_to_bool(row["legal"]).cpu().numpy()
        for g in np.nonzero(live & ~terminal)[0]:
            pi = selfplay_model.pi_row(N[g], np.nonzero(legal[g])[0].tolist(), R, 1.0)
            assert np.array_equal(_bits(dev["pi"][t, g]), _bits(pi)), (t, g)
            assert np.array_equal(dev["mask"][t, g], legal[g].astype(np.uint8)), (t, g)
    assert np.array_equal(dev["length"], length)
    assert not rows[-1]["live"].cpu().numpy()[~rows[-1]["terminal"].cpu().numpy()].any()       # every game ended
    assert np.array_equal(dev["winner"], env.node_info(python_key=False)["winner"].cpu().numpy())
    assert torch.equal(sp.env.state, env.state)
    return sp, batch


@pytest.fixture(scope="module")
def played_130():
    """One play() of 130 games (R = 6, S = 2, uniform search), checked against the hand loop: (SelfPlay, batch)."""
    return _assert_play_is_the_hand_loop(130, 6, 2, None, 11)


def test_play_is_the_hand_loop_of_the_public_calls(played_130):
    sp, batch = played_130
    assert sp.plays == 1 and int(batch.length.max()) <= ROWS


def test_play_with_the_network_is_the_hand_loop_of_the_public_calls():
    _assert_play_is_the_hand_loop(65, 6, 2, _net(torch.float32), 5)


# ---------------------------------------------------------------- invariants
def test_record_leaves_the_tree_as_it_was():
    G, R = 130, 6
    sp = SelfPlay(G, n_rollouts=R, num_simulations=2, device=DEV)
    env = VecEnv(G, device=DEV, seed=3)
    tree = TreeSearch(G, capacity=sp.capacity, num_simulations=2, seed=7, device=DEV)
    tree.reset(env)
    tree.contemplate(R)
    before = tree.tree.clone()
    batch = sp.new_batch()
    actions = sp.record(tree, 0, batch)
    assert torch.equal(tree.tree, before)
    assert actions is batch.actions and (batch.length == 1).all() and (actions < 9).all()


def test_batch_invariants(played_130):
    sp, batch = played_130
    G = sp.num_games
    b = _host(batch)
    length = b["length"].astype(np.int64)
    rows = np.arange(ROWS)[:, None]
    assert np.array_equal(b["done"], (rows == length[None, :] - 1).astype(np.uint8))       # the terminal row, only
    past = rows >= length[None, :]
    words, _ = _planes(b["states"], G)
    for k in ("pi", "mask", "v", "action36", "done"):
        assert not b[k][past].any(), k
    assert not words.transpose(0, 2, 1)[past].any()
    final = sp.env.export_boards()
    moves, n_moves = final["moves"].cpu().numpy().astype(np.int64), final["n_moves"].cpu().numpy().astype(np.int64)
    # the moves the players made: Board.moves less the autofill entry (board.py:22-25), which names one square twice
    played = ((np.arange(9)[None, :] < n_moves[:, None]) & (moves[:, :, 0] != moves[:, :, 1])).sum(1)
    assert np.array_equal(length - 1, played)
    assert ((n_moves == played) | ((n_moves == 9) & (played == 8))).all()
    info = sp.env.node_info(python_key=False)
    assert info["terminal"].all() and np.array_equal(b["winner"], info["winner"].cpu().numpy())
    live = ~past
    assert np.abs(b["pi"].sum(-1)[live] - 1.0).max() <= 1e-14
    assert not b["pi"][b["mask"] == 0].any()
    for t in range(ROWS):
        _, mask = batch.row_env(t).encode()
        before_end = rows[t] < length - 1
        assert np.array_equal(b["mask"][t][before_end], mask.cpu().numpy()[before_end].astype(np.uint8)), t
    last = (length - 1, np.arange(G))
    assert (b["pi"][last] == 1.0 / 36.0).all() and b["mask"][last].all() and (b["action36"][last] == 255).all()
    assert (b["action36"][rows < length[None, :] - 1] < 36).all() and (b["actions"] == 255).all()


@pytest.mark.parametrize("targets", [(1.0, 0.0), (1.0, -1.0)])
def test_value_targets_follow_the_sign_pattern(played_130, targets):
    sp0, batch0 = played_130
    if targets == (1.0, 0.0):
        batch = batch0
    else:
        batch = SelfPlay(130, n_rollouts=6, num_simulations=2, value_targets=targets, seed=11, device=DEV).play()
        assert torch.equal(batch.states, batch0.states) and torch.equal(batch.pi, batch0.pi)
    b = _host(batch)
    assert set(b["winner"].tolist()) >= {0, 1}                # both players win some games
    for g in range(130):
        n = int(b["length"][g])
        ref = selfplay_model.value_targets(int(b["winner"][g]), n, *targets)
        assert np.array_equal(_bits(b["v"][:n, g]), _bits(ref)), g
    assert not np.signbit(b["v"][b["v"] == 0]).any()


# ---------------------------------------------------------------- compaction, seeds, flat()
def test_compact_returns_the_same_batch(played_130):
    _, batch = played_130
    sp = SelfPlay(130, n_rollouts=6, num_simulations=2, seed=11, compact=True, device=DEV)
    assert sp.capacity == 2 * 6 + 2 * 6 + 2
    assert _same_bytes(sp.play(), batch)
    assert int(sp.tree.nodes_used().max()) <= sp.capacity


def test_seeds(played_130):
    _, batch = played_130
    sp = SelfPlay(130, n_rollouts=6, num_simulations=2, seed=11, device=DEV)
    assert _same_bytes(sp.play(), batch)                     # the first play: seed 11
    nxt = sp.play()                                          # the second: seed 12
    assert sp.plays == 2 and _same_bytes(nxt, SelfPlay(130, n_rollouts=6, num_simulations=2, seed=12, device=DEV).play())
    assert not _same_bytes(nxt, batch) and not torch.equal(nxt.action36, batch.action36)
    assert _same_bytes(sp.play(seed=11), batch)


def test_flat_is_the_reference_batch_in_game_major_order(played_130):
    _, batch = played_130
    s, pi, mask, v, done = batch.flat()
    length = batch.length.cpu().numpy().astype(np.int64)
    n = int(length.sum())
    assert s.shape == (n, 18, 10) and s.dtype == torch.float32 and pi.shape == (n, 36) and pi.dtype == torch.float64
    assert mask.shape == (n, 36) and mask.dtype == torch.bool and v.shape == (n,) and v.dtype == torch.float32
    assert done.shape == (n,) and done.dtype == torch.bool
    enc = torch.stack([batch.row_env(t).encode(with_mask=False) for t in range(ROWS)]).cpu().numpy()
    b = _host(batch)
    s, pi, mask, v, done = (x.cpu().numpy() for x in (s, pi, mask, v, done))
    i = 0
    for g in range(130):
        for t in range(length[g]):
            assert np.array_equal(s[i], enc[t, g]) and np.array_equal(_bits(pi[i]), _bits(b["pi"][t, g])), (g, t)
            assert np.array_equal(mask[i], b["mask"][t, g].astype(bool)) and v[i] == b["v"][t, g], (g, t)
            assert done[i] == (t == length[g] - 1), (g, t)
            i += 1
    assert i == n


# ---------------------------------------------------------------- roots of every depth, alpha
@pytest.fixture(scope="module")
def searched_positions():
    """130 positions 0..7 plies deep, searched with 40 rollouts: (tree, N i32[G,36], legal bool[G,36], terminal[G])."""
    G, R = 130, 40
    env = env_from_arrays(random_positions(G, 130))
    tree = TreeSearch(G, capacity=2 * R + 2, num_simulations=2, seed=9, device=DEV)
    tree.reset(env)
    tree.contemplate(R)
    info = env.node_info(python_key=False)
    return (tree, tree.root_stats()["N"].cpu().numpy(), legal_mask_to_bool(info["legal"]).cpu().numpy(),
            info["terminal"].cpu().numpy())


def test_one_record_of_roots_of_every_depth_matches_the_model(searched_positions):
    tree, N, legal, terminal = searched_positions
    sp = SelfPlay(130, n_rollouts=40, num_simulations=2, device=DEV)
    batch = sp.new_batch()
    sp.record(tree, 0, batch)
    b = _host(batch)
    assert terminal.any() and not terminal.all()
    assert np.array_equal(b["done"][0], terminal.astype(np.uint8)) and not b["done"][1:].any()
    assert np.array_equal(b["action36"][0], np.where(terminal, 255, tree.choose().cpu().numpy()))
    for g in range(130):
        ref = np.full(36, 1.0 / 36.0) if terminal[g] else selfplay_model.pi_row(N[g], np.nonzero(legal[g])[0].tolist(), 40)
        assert np.array_equal(_bits(b["pi"][0, g]), _bits(ref)), g
    assert torch.equal(batch.actions, action36_to_pairs(batch.action36[0]))


def test_alpha_half_against_the_reference_expression(searched_positions):
    tree, N, legal, terminal = searched_positions
    n_rollouts = 40
    sp = SelfPlay(130, n_rollouts=n_rollouts, num_simulations=2, alpha=0.5, device=DEV)
    batch = sp.new_batch()
    sp.record(tree, 0, batch)
    pi = batch.pi[0].cpu().numpy()
    worst = 0.0
    for g in np.nonzero(~terminal)[0]:
        a = np.nonzero(legal[g])[0]
        ref = np.zeros(36)
        ref[a] = (N[g][a] / n_rollouts) ** 0.5                   # self_play.py:210-211
        ref /= np.sum(ref, axis=-1)
        worst = max(worst, float(np.max(np.abs(pi[g] - ref) / np.where(ref > 0, ref, 1.0))))
        # the device pow's error is a few ulps, not derived here: three orders over the summation bound of 8e-15
        np.testing.assert_allclose(pi[g], ref, rtol=1e-12, atol=0.0)
    print("alpha = 0.5: largest relative deviation from the numpy expression %.3g" % worst)
    assert (pi[terminal] == 1.0 / 36.0).all()


def test_an_unvisited_root_gives_the_reference_nan_row():
    G = 3
    sp = SelfPlay(G, n_rollouts=4, num_simulations=2, device=DEV)
    env = VecEnv(G, device=DEV)
    tree = TreeSearch(G, capacity=4, num_simulations=2, device=DEV)
    tree.reset(env)                                          # no rollout: N = 0 everywhere
    batch = sp.new_batch()
    sp.record(tree, 0, batch)
    assert torch.isnan(batch.pi[0]).all() and (batch.mask[0] == 1).all() and not batch.pi[1:].any()
    assert (batch.action36[0] == 0).all()                    # choose: the lowest legal action when none was visited
