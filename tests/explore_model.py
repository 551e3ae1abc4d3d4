"""A float64 restatement, in numpy, of the two rules of include/qttt_tree_explore.h: the Dirichlet noise that
qttt_tree_root_noise mixes into a root's priors, and the move that qttt_selfplay_record_sampled draws from the visit
counts.  Test infrastructure: tests/test_explore_cpu.py checks it against the analytic moments of the Dirichlet
distribution and a chi-square test of the move frequencies; tests/test_explore_gpu.py runs the device against it.

The hashes are the library's own host-callable qttt_hash.  Besides its result every function reports the MARGIN of each
decision it took: |lhs - rhs| of a Marsaglia-Tsang accept / reject (|1 + c x| where the try is rejected because v <= 0),
and |t - c[a]| / T for every action a sampled move could have flipped to.  The device's log / cos / pow sit a few ulps
from numpy's, so a decision can only differ where its margin is of that order; the tests assert the margins of the cases
they use (CASES below) instead of widening a tolerance.  A plain helper module."""
import numpy as np

import oracle
import selfplay_model
import tree_model
from qtttgym_amd import _native

NOISE_BASE, TRIES, DRAWS = _native.TREE_NOISE_BASE, _native.TREE_NOISE_TRIES, _native.TREE_NOISE_DRAWS
MOVE_BASE = _native.SELFPLAY_MOVE_BASE
TWO_PI = 6.283185307179586
_LANES = np.arange(64)

# ---------------------------------------------------------------- what the GPU tests draw (and the CPU test vouches for)
SEED, OFFSET, G_MAX = 5, 17, 65
BIG_OFFSET = (1 << 32) + 12345
NOISE_PARAMS = ((0.25, 0.3), (0.5, 1.0), (0.25, 2.5))          # (epsilon, alpha)
# every (seed, board_offset, noise_idx, games) the GPU tests compare with the model, for every alpha of NOISE_PARAMS
NOISE_CASES = ((SEED, OFFSET, 0, G_MAX), (SEED, OFFSET, 1, G_MAX), (SEED + 1, OFFSET, 0, G_MAX),
               (SEED, BIG_OFFSET, 0, G_MAX))
# the whole games of the sampled record: (G, n_rollouts, n_sims, seed)
PLAY = (65, 8, 2, 7)


def qhash(seed, board_id, idx):
    return int(_native.lib().qttt_hash(int(seed), int(board_id), int(idx) & 0xFFFFFFFF))


def u53(h):
    """U53 of 64-bit hashes (an int or a uint64 array)."""
    return ((np.asarray(h, dtype=np.uint64) >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53


def u32(w):
    return (np.asarray(w, dtype=np.uint64).astype(np.float64) + 0.5) * 2.0 ** -32


def wave_sum(x):
    return selfplay_model.wave_sum(x)


# ---------------------------------------------------------------- the noise
def _hashes(seed, board_ids, idx):
    return np.array([qhash(seed, b, i) for b, i in zip(board_ids.tolist(), idx.tolist())], dtype=np.uint64)


def gamma_many(seed, board_ids, noise_idx, actions, alpha):
    """(y f64[k], margins f64[k, TRIES]): the Gamma(alpha) variates of the pairs (board_ids[i], actions[i]), and the
    margin of every try's decision (NaN for the tries after the accepted one, which are not made)."""
    board_ids, actions = np.asarray(board_ids, dtype=np.int64), np.asarray(actions, dtype=np.int64)
    alpha = np.float64(alpha)
    a1 = alpha + 1.0 if alpha < 1.0 else alpha
    d = a1 - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * d)
    base = NOISE_BASE + (noise_idx * 36 + actions) * DRAWS
    y = np.full(len(actions), a1, dtype=np.float64)
    margins = np.full((len(actions), TRIES), np.nan)
    pending = np.arange(len(actions))
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(TRIES):
            if not len(pending):
                break
            h0 = _hashes(seed, board_ids[pending], base[pending] + 2 * t)
            h1 = _hashes(seed, board_ids[pending], base[pending] + 2 * t + 1)
            x = np.sqrt(-2.0 * np.log(u53(h0))) * np.cos(TWO_PI * u32(h1 >> np.uint64(32)))
            u = 1.0 + c * x
            v = u * u * u
            lhs, rhs = np.log(u32(h1 & np.uint64(0xFFFFFFFF))), 0.5 * x * x + d - d * v + d * np.log(v)
            positive = v > 0.0
            accept = positive & (lhs < rhs)
            margins[pending, t] = np.where(positive, np.abs(lhs - rhs), np.abs(u))
            y[pending[accept]] = (d * v)[accept]
            pending = pending[~accept]
    if alpha < 1.0:
        y = y * np.power(u53(_hashes(seed, board_ids, base + 2 * TRIES)), 1.0 / alpha)
    return y, margins


def noise_rows(seed, board_offset, noise_idx, legal, alpha):
    """(n f64[G, 36], applied bool[G], margins): the normalised noise of G roots, legal = their lists of legal actions;
    a root whose sum is 0 or not finite (or that has no legal action) has applied False and a zero row."""
    G = len(legal)
    games = np.array([g for g in range(G) for _ in legal[g]], dtype=np.int64)
    actions = np.array([a for g in range(G) for a in legal[g]], dtype=np.int64)
    y = np.zeros((G, 36))
    vals, margins = gamma_many(seed, board_offset + games, noise_idx, actions, alpha)
    y[games, actions] = vals
    n, applied = np.zeros((G, 36)), np.zeros(G, dtype=bool)
    for g in range(G):
        S = wave_sum(y[g])
        if legal[g] and S != 0.0 and np.isfinite(S):
            n[g], applied[g] = y[g] / S, True
    return n, applied, margins[~np.isnan(margins)]


def mix(p, n, legal, epsilon):
    """The root's new prior row f32[36]: p f64[36] = the priors the search read so far."""
    out = np.zeros(36, dtype=np.float32)
    eps = np.float64(epsilon)
    for a in legal:
        out[a] = np.float32((1.0 - eps) * np.float64(p[a]) + eps * n[a])
    return out


# ---------------------------------------------------------------- the sampled move
def sample_move(N, legal, seed, board_id, ply, temperature):
    """(the move or None where the record falls back to choose, margin): N = the 36 visit counts."""
    w = np.zeros(64)
    for a in legal:
        if int(N[a]) > 0:
            w[a] = np.float64(int(N[a])) if temperature == 1.0 else np.power(np.float64(int(N[a])), 1.0 / np.float64(temperature))
    c = w.copy()
    for m in (1, 2, 4, 8, 16, 32):
        nxt = c.copy()
        nxt[m:] = c[m:] + c[:-m]
        c = nxt
    T = c[63]
    if T == 0.0 or not np.isfinite(T):
        return None, np.inf
    t = (np.float64(qhash(seed, board_id, MOVE_BASE + ply) >> 11) * 2.0 ** -53) * T
    hit = [a for a in range(36) if w[a] > 0.0 and t < c[a]]
    margin = min(abs(float(t - c[a])) / float(T) for a in range(36) if w[a] > 0.0)
    return (hit[0] if hit else None), margin


def record_sampled(tree, ply, n_rollouts, alpha, v_first, v_second, out, seed, board_offset, temperature, sample_plies):
    """qttt_selfplay_record_sampled on a TreeModel: selfplay_model.record with the move of the live roots that are not
    terminal drawn by sample_move at ply < sample_plies.  Returns (out["actions"], the margins of the moves drawn)."""
    live = [ply == 0 or (out["length"][g] == ply and not out["done"][ply - 1, g]) for g in range(len(tree.games))]
    selfplay_model.record(tree, ply, n_rollouts, alpha, v_first, v_second, out)
    margins = []
    for g, st in enumerate(tree.games):
        n = st["nodes"][st["root"]]
        if live[g] and not n.terminal and ply < sample_plies:
            a, margin = sample_move(n.N, n.legal, seed, board_offset + g, ply, temperature)
            if a is not None:
                margins.append(margin)
                out["action36"][ply, g] = a
                out["actions"][g] = oracle.ind2move(a)
    return out["actions"], margins


def play(G, n_rollouts, n_sims, seed, temperature=1.0, sample_plies=0):
    """SelfPlay(sample_plies=..., temperature=...).play(seed) under the uniform search: (the batch, the final
    OracleBoards, the margins of every move drawn).  selfplay_model.play with the sampled record."""
    env = oracle.OracleBoards(G)
    tree = tree_model.TreeModel(n_sims, seed=2 * seed + 1, board_offset=0)
    tree.reset(env)
    out = selfplay_model.new_batch(G)
    margins = []
    for ply in range(selfplay_model.ROWS):
        if ply < selfplay_model.ROWS - 1:
            for _ in range(n_rollouts):
                tree.rollout()
        actions, m = record_sampled(tree, ply, n_rollouts, 1.0, 1.0, 0.0, out, 2 * seed + 1, 0, temperature, sample_plies)
        margins += m
        env.step(actions.copy(), None, seed, ply, 0, False)
        tree.sync(env)
    return out, env, margins
