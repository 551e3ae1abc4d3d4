"""The drivers the search and self-play GPU tests share (tests/test_tree_gpu.py, test_tree_whole_gpu.py,
test_tree_compact_gpu.py, test_selfplay_gpu.py): positions as import arrays, a TreeSearch over a sentinel-filled buffer
beside its float64 model (tests/tree_model.py), one rollout and one move of the two in lockstep, and the comparison of
the roots' statistics.  The whole-tree comparison is tests/tree_layout.py's.  A plain helper module."""
import numpy as np
import torch

import oracle
import tree_layout
import tree_model

DEV = "cuda:0"
SENTINEL = 0xA5
TAIL = 4 * tree_layout.NODE_BYTES          # what search() allocates after the tree: four node records


# ---------------------------------------------------------------- positions
def env_from_arrays(arrays, seed=0):
    from qtttgym_amd import VecEnv
    env = VecEnv(len(arrays["n_moves"]), device=DEV, seed=seed)
    env.import_boards(arrays["moves"], arrays["n_moves"], arrays["board"], np.asarray(arrays["qmask"]).astype(np.int16),
                      arrays["n_q"])
    return env


def export(env):
    return {k: v.cpu().numpy() for k, v in env.export_boards().items()}


def boards(arrays):
    return oracle.boards_from_arrays(arrays["board"], arrays["moves"], arrays["n_moves"], arrays["qmask"], arrays["n_q"])


def random_positions(G, seed):
    """G positions 0..7 random plies deep (step_random_many), as import arrays."""
    from qtttgym_amd import VecEnv
    env = VecEnv(G, device=DEV, seed=seed)
    snaps = [export(env)]
    for _ in range(7):
        env.step_random_many(1)
        snaps.append(export(env))
    depth = np.random.default_rng(seed).integers(0, len(snaps), G)
    return {k: np.stack([snaps[d][k][g] for g, d in enumerate(depth)]) for k in snaps[0]}


def two_plies_in(G, seed):
    """G positions two uniform-random plies from the empty board (the oracle's draws), as import arrays."""
    ob = oracle.OracleBoards(G)
    for t in range(2):
        ob.step(ob.sample_actions(seed, t), None, seed, t)
    return {"board": ob.board, "moves": ob.moves, "n_moves": ob.n_moves, "qmask": ob.qmask, "n_q": ob.n_q}


def net(dtype):
    from nn_reference64 import golden_state_dict, load_golden
    from qtttgym_amd import PolicyValueNet
    return PolicyValueNet(golden_state_dict(load_golden()), device=DEV, dtype=dtype)


# ---------------------------------------------------------------- the roots' statistics
def stats(t):
    return {k: v.cpu().numpy() for k, v in t.root_stats().items()}


def assert_stats_equal(dev, ref, keys):
    for k in keys:
        assert np.array_equal(dev[k], ref[k]), (k, np.nonzero(np.any((dev[k] != ref[k]).reshape(len(ref[k]), -1), 1))[0][:8])


# ---------------------------------------------------------------- the device and the model, side by side
def search(arrays, capacity, S, c_puct=1.0, net=None, seed=5, offset=17, model_capacity=None):
    """(t, m, env): a TreeSearch over a buffer of the test's own, filled with SENTINEL and TAIL bytes longer than the
    tree, the model, and the env, all at the positions `arrays`."""
    from qtttgym_amd import TreeSearch
    env = env_from_arrays(arrays)
    G = env.num_envs
    t = TreeSearch(G, capacity=capacity, num_simulations=S, c_puct=c_puct, net=net, seed=seed, board_offset=offset,
                   device=DEV)
    nbytes = int(t._lib.qttt_tree_bytes(G, capacity))
    assert nbytes == tree_layout.tree_bytes(G, capacity)
    t.tree = torch.full((nbytes + TAIL,), SENTINEL, dtype=torch.uint8, device=DEV)
    t.reset(env)
    m = tree_model.TreeModel(S, seed=seed, board_offset=offset, c_puct=c_puct, capacity=model_capacity)
    m.reset(boards(arrays))
    return t, m, env


def rollout(t, m, bounded=True):
    """One rollout in lockstep: the model selects, the device does a whole rollout (bounded=False: without the
    host-side bounds of contemplate), the leaves are compared, the model backs up from the device's playouts (and
    network priors).  Returns (the model's leaves, the device's result)."""
    leaves = m.select()
    if bounded:
        t.contemplate(1)
    else:
        t._rollout()
    ex = export(t.leaf)               # the leaf buffer is only rewritten by the next select
    for key, val in (("board", leaves.board), ("moves", leaves.moves), ("n_moves", leaves.n_moves)):
        assert np.array_equal(ex[key], val), (key, m.k)
    result = (t._out if t.net is None else t._out["result"]).cpu().numpy()
    m.backup(result, None if t.net is None else t._out["probs"].cpu().numpy())
    return leaves, result


def move(t, m, env, act, bits):
    """The games play `act` (action36, 255: no move) with collapse bits `bits`; the tree and the model sync."""
    from qtttgym_amd.actions import action36_to_pairs
    env.step_raw(action36_to_pairs(torch.as_tensor(act, device=DEV)).contiguous(), torch.as_tensor(bits, device=DEV))
    t.sync(env)
    m.sync(boards(export(env)))
