"""The drivers the search and self-play GPU tests share (tests/test_tree_gpu.py, test_tree_whole_gpu.py,
test_tree_compact_gpu.py, test_selfplay_gpu.py): positions as import arrays, a TreeSearch over a sentinel-filled buffer
beside its float64 model (tests/tree_model.py), one rollout and one move of the two in lockstep, and the comparison of
the roots' statistics.  The whole-tree comparison is tests/tree_layout.py's.  Last, the driver of the exact-leaves and
prove tests (tests/test_tree_exact_gpu.py, test_tree_prove_gpu.py; env_of_planes also test_selfplay_exact_gpu.py), by
the model module: tests/exact_leaves_model.py or tests/prove_model.py.  A plain helper module."""
import copy
import functools

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


# ---------------------------------------------------------------- exact leaves and proven nodes: one driver, two models
GUARD = 0xA5


def exact_nets():
    import nn_reference64 as R
    return {"zero": R.zero_state_dict, "greedy": R.greedy_state_dict, "counting": R.counting_state_dict,
            "sharp": R.sharp_counting_state_dict}


@functools.lru_cache(maxsize=None)
def exact_net(name):
    """The f32 network of an exact state dict by name; any other name: the golden network."""
    import nn_reference64 as R
    from qtttgym_amd import PolicyValueNet
    nets = exact_nets()
    sd = nets[name]() if name in nets else R.golden_state_dict(R.load_golden())
    return PolicyValueNet(sd, device=DEV, dtype=torch.float32)


def _evaluate_probs(leaves):
    env = env_from_arrays({"board": leaves.board, "moves": leaves.moves, "n_moves": leaves.n_moves, "qmask": leaves.qmask,
                           "n_q": leaves.n_q})
    return env.evaluate(exact_net("counting"), rows=("probs",))["probs"].cpu().numpy()


@functools.lru_cache(maxsize=None)
def exact_model(MM, net, K, M, capacity):
    """MM.searched's model (MM: exact_leaves_model or prove_model), computed once and left alone."""
    return MM.searched(exact_nets()[net](), K, M, capacity, probs_of=_evaluate_probs if net == "counting" else None)


@functools.lru_cache(maxsize=None)
def exact_stages(MM, net, K, M):
    return MM.searched(exact_nets()[net](), K, M, MM.CAPACITY, stages=True)


def games_view(m, G):
    v = copy.copy(m)
    v.games = m.games[:G]
    return v


def prefix(arrays, G):
    return {k: np.asarray(v)[:G] for k, v in arrays.items()}


def bits32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def exact_search(MM, arrays, capacity, net, **kw):
    """(t, env): a value-leaf TreeSearch with MM's seed and offset over a sentinel-filled buffer, at `arrays`."""
    from qtttgym_amd import TreeSearch
    env = env_from_arrays(arrays)
    G = env.num_envs
    t = TreeSearch(G, capacity=capacity, net=net, seed=MM.SEED, board_offset=MM.OFFSET, device=DEV, leaf_eval="value", **kw)
    t.tree = torch.full((tree_layout.tree_bytes(G, capacity) + TAIL,), SENTINEL, dtype=torch.uint8, device=DEV)
    t.reset(env)
    return t, env


def exact_rounds(t, r):
    """TreeSearch.contemplate's schedule under exact_from (tests/prove_model.py's schedule: one leaf while the tree is
    fresh, rounds of K, the rest), without the host's node bound (the pool that overflows)."""
    import prove_model
    for k in prove_model.schedule(r, t.leaves, t._fresh):
        t._round(k)
        t._fresh = False


def check_exact_tree(t, m, compacted=False, kept_rows=False):
    """The whole tree buffer against the model: the solved bit and the value bits of every live node against the model's
    solved nodes (proven ones included); with kept_rows the priors row that a proven node keeps under its cleared flag
    against the row the model kept; then — those bits taken out of a copy and those rows painted over — every other byte
    by tests/tree_layout.py's comparison (which expects no has-priors flag on a proven node below the root).  Returns
    the number of kept rows compared."""
    import exact_leaves_model as E
    solved_bits = np.uint32(E.NODE_SOLVED | E.NODE_VALUE_MASK)
    G, cap = t.num_games, t.capacity
    buf = t.tree.cpu().numpy().copy()
    games, nodes, priors, _ = tree_layout.decode(buf, G, cap)
    want = np.zeros((G, cap), dtype=np.uint32)
    for g, flags in enumerate(m.solved_flags()):
        for i, f in flags.items():
            want[g, i] = f
    live = np.arange(cap)[None, :] < games["used"][:, None]
    got = nodes["flags"] & solved_bits
    assert np.array_equal(got[live], want[live]), np.argwhere((got != want) & live)[:8].tolist()
    assert np.array_equal(t.solved_count().cpu().numpy(), m.solved_counts())
    kept = 0
    if kept_rows and not compacted:
        for g, st in enumerate(m.games):
            for x, row in st["kept"].items():
                assert np.array_equal(bits32(priors[g, x]), bits32(row)), ("kept priors row", g, x)
                priors[g, x].view(np.uint8)[:] = SENTINEL
                kept += 1
    nodes["flags"][live] &= ~solved_bits
    tree_layout.assert_tree_equals_model(buf, G, cap, m, SENTINEL, DEV, compacted=compacted)
    return kept


def env_of_planes(P, Q):
    """A VecEnv over the state planes P, Q (u64 arrays of one length)."""
    from qtttgym_amd import VecEnv, _native
    n = len(P)
    stride = (n + 63) & ~63
    planes = np.zeros((2, stride), dtype=np.uint64)
    planes[0, :n], planes[1, :n] = P, Q
    state = torch.from_numpy(planes.view(np.uint8).reshape(-1).copy()).to(DEV)
    assert state.numel() == int(_native.lib().qttt_state_bytes(n))
    return VecEnv.from_state(state, n)
