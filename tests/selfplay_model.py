"""A plain-Python restatement of the self-play record of include/qttt_selfplay.h (qtttgym_amd.SelfPlay) over the
float64 tree model (tests/tree_model.py) and the C oracle.  Test infrastructure: tests/test_selfplay_cpu.py ties it to
the numpy expressions the reference runs and tests/test_az_reference_cpu.py to whole games of the reference's own
play_game (tests/golden/selfplay_traces.npz); tests/test_selfplay_gpu.py runs the device against it.

What it restates, by line of the reference's self_play.py:
  :43-76   play_game: until the root is terminal, n_rollouts x do_rollout, choose, make_move; the visited roots and the
           winner come back.  Here for G games at once, a finished game riding along with noop moves.
  :193-199 v_target from the winner (the reference's `elif winner:` never fires: (v_first, v_second) = (1, 0)).
  :200-216 one sample per root: to_vector (here: the root's board record), the terminal row's pi = 1 / 36, mask = 1 and
           done = True (:203-206), every other row's pi[a] = (N / n_rollouts) ** alpha normalised over the legal
           actions, the action mask and done = False (:207-214), and v_target alternating in sign down the game
           (:215-216).
The sum of :211 is taken in the order the header documents (wave_sum)."""
import numpy as np

import oracle
import tree_model
from qtttgym_amd import _native

ROWS = _native.SELFPLAY_ROWS
_LANES = np.arange(64)


def wave_sum(x):
    """The header's sum of 36 doubles: 64 terms (28 zeros appended), s[i] = s[i] + s[i ^ m] for m = 1, 2, 4, 8, 16, 32;
    the sum is s[0]."""
    s = np.zeros(64, dtype=np.float64)
    s[:36] = x
    for m in (1, 2, 4, 8, 16, 32):
        s = s + s[_LANES ^ m]
    return s[0]


def pi_row(N, legal, n_rollouts, alpha=1.0):
    """self_play.py:208-211 for one root: N = the 36 visit counts, legal = the legal actions.  f64[36]; NaN on the legal
    actions when none was visited (the reference's 0 / 0)."""
    x = np.zeros(36, dtype=np.float64)
    for a in legal:
        x[a] = float(int(N[a])) / float(n_rollouts)
        if alpha != 1.0:
            x[a] = x[a] ** alpha
    total = wave_sum(x)
    pi = np.zeros(36, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        for a in legal:
            pi[a] = np.float64(x[a]) / total
    return pi


def value_targets(winner, rows, v_first=1.0, v_second=0.0):
    """self_play.py:195-199, 215-216: f32[rows], v0 * (-1)^i with v0 = v_first / v_second / 0 for winner 1 / 0 / -1
    (True / False / None); a zero is +0.0."""
    v0 = np.float32(v_first) if winner == 1 else (np.float32(v_second) if winner == 0 else np.float32(0.0))
    v = np.array([v0 if i % 2 == 0 else -v0 for i in range(rows)], dtype=np.float32)
    v[v == 0] = 0.0
    return v


def new_batch(G):
    return {"recs": [[None] * G for _ in range(ROWS)], "pi": np.zeros((ROWS, G, 36)), "mask": np.zeros((ROWS, G, 36), np.uint8),
            "done": np.zeros((ROWS, G), np.uint8), "v": np.zeros((ROWS, G), np.float32),
            "action36": np.zeros((ROWS, G), np.uint8), "length": np.zeros(G, np.uint8), "winner": np.zeros(G, np.int8),
            "actions": np.zeros((G, 2), np.uint8)}


def record(tree, ply, n_rollouts, alpha, v_first, v_second, out):
    """qttt_selfplay_record on a TreeModel: row `ply` of `out`; returns out["actions"]."""
    for g, st in enumerate(tree.games):
        if ply != 0 and (out["length"][g] != ply or out["done"][ply - 1, g]):        # the terminal row was recorded earlier
            out["actions"][g] = (255, 255)
            continue
        n = st["nodes"][st["root"]]
        out["recs"][ply][g] = n.rec.copy()
        out["length"][g] = ply + 1
        if n.terminal:                                       # self_play.py:203-206
            out["pi"][ply, g] = 1.0 / 36.0
            out["mask"][ply, g] = 1
            out["done"][ply, g] = 1
            out["action36"][ply, g] = 255
            out["actions"][g] = (255, 255)
            out["winner"][g] = n.winner
            out["v"][:ply + 1, g] = value_targets(n.winner, ply + 1, v_first, v_second)
            continue
        out["mask"][ply, g, n.legal] = 1                     # self_play.py:207-214
        out["pi"][ply, g] = pi_row(n.N, n.legal, n_rollouts, alpha)
        out["done"][ply, g] = 0
        a = tree_model.choose(n)                             # self_play.py:68
        out["action36"][ply, g] = a
        out["actions"][g] = oracle.ind2move(a) if a != 255 else (255, 255)
    return out["actions"]


def play(G, n_rollouts, n_sims, seed=0, alpha=1.0, c_puct=1.0, v_first=1.0, v_second=0.0, net=None):
    """SelfPlay.play(seed): (the batch, the final OracleBoards); net = None (MCTS) or the state dict of an exact network
    (TreeModel(net=...)).  The environment's collapse bits are the counter hash of (seed, game, ply); the trees draw
    with 2 * seed + 1."""
    env = oracle.OracleBoards(G)
    tree = tree_model.TreeModel(n_sims, seed=2 * seed + 1, board_offset=0, c_puct=c_puct, net=net)
    tree.reset(env)
    out = new_batch(G)
    for ply in range(ROWS):
        if ply < ROWS - 1:
            for _ in range(n_rollouts):
                tree.rollout()
        actions = record(tree, ply, n_rollouts, alpha, v_first, v_second, out)
        env.step(actions.copy(), None, seed, ply, 0, False)          # self_play.py:69; (255, 255) is a noop
        tree.sync(env)
    return out, env


# ---------------------------------------------------------------- tests/golden/selfplay_traces.npz
def golden_games(path):
    """Per network of the fixture: dict(net, seed, n_rollouts, n_sims, G, and the reference's own s f32[n,18,10],
    pi f64[n,36], mask bool[n,36], v i8[n], done bool[n] in game-major order, length u8[G], winner i8[G],
    actions u8[G,9] (255 past the game's end) and bits u8[G,9])."""
    z = np.load(path)
    out = []
    for name in (str(x) for x in z["nets"]):
        d = {k: z["%s_%s" % (name, k)] for k in ("s", "pi", "mask", "v", "done", "length", "winner", "actions", "bits")}
        d.update(net=name, seed=int(z["seed"]), n_rollouts=int(z["n_rollouts"]), n_sims=int(z["n_sims"]), G=len(d["length"]))
        out.append(d)
    return out


def assert_rows_equal_reference(fx, s, pi, mask, v, done):
    """The batch rows (game-major, as SelfPlayBatch.flat() and the reference's lists) against one network of the
    fixture: everything exact but pi, whose sum the device takes in wave order and numpy in its own: two orders of 36
    non-negative doubles differ by less than 2 * 35 * 2^-53 relative, so rtol = 1e-14 and atol = 0; the illegal
    entries are exactly 0 and the terminal row exactly 1 / 36 under a full mask."""
    assert s.dtype == np.float32 and np.array_equal(s, fx["s"])
    assert np.array_equal(np.asarray(mask, dtype=bool), fx["mask"])
    assert np.array_equal(np.asarray(done, dtype=bool), fx["done"])
    v = np.asarray(v, dtype=np.float32)
    assert np.array_equal(v.view(np.uint32), fx["v"].astype(np.float32).view(np.uint32))
    assert pi.dtype == np.float64 and pi.shape == fx["pi"].shape
    np.testing.assert_allclose(pi, fx["pi"], rtol=1e-14, atol=0.0)
    assert (pi[~fx["mask"]] == 0).all()
    last = fx["done"]
    assert last.sum() == fx["G"] and (pi[last] == 1.0 / 36.0).all() and fx["mask"][last].all()
    assert np.array_equal(np.flatnonzero(last), np.cumsum(fx["length"].astype(np.int64)) - 1)


def assert_games_equal_reference(fx, action36, length, winner):
    """action36 u8[10, G], length[G] and winner[G] of a batch against the games the reference played."""
    assert np.array_equal(length, fx["length"]) and np.array_equal(winner, fx["winner"])
    for g in range(fx["G"]):
        n = int(fx["length"][g])
        assert np.array_equal(action36[:n - 1, g], fx["actions"][g, :n - 1]) and action36[n - 1, g] == 255, g
        assert (fx["actions"][g, n - 1:] == 255).all() and not action36[n:, g].any(), g
