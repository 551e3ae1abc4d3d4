"""The searches that tests/test_gumbel_gpu.py runs on the device and tests/test_gumbel_cpu.py on the model alone: the
root positions, the cases (G, leaves, n, max_considered, capacity), the networks, and the model's side of a whole search:
a contemplate(n + 1) from fresh roots, a move, a sync and a compaction, a second contemplate(n + 1) on the reused
subtrees.  A plain helper module."""
import functools

import numpy as np

import gumbel_model as GM
import nn_reference64 as R
import oracle
import tree_model

SEED, OFFSET, POSITION_SEED = 5, 17, 2031
GAP = 1e-9                   # a root decision whose two best scores are closer than this may be left out (random network only)
LEFT_OUT_CAP = 0.02
OVERFLOW_CAPACITY = 12
# (G, leaves, n, max_considered, capacity or None = a pool that always fits): every G of {1, 5, 67}, every leaves of
# {1, 3, 8}, every n of {2, 16, 33} and every max_considered of {1, 4, 16, 36} occurs
CASES = ((1, 1, 2, 1, None), (5, 3, 16, 4, None), (67, 8, 33, 16, None), (67, 1, 16, 36, None), (5, 8, 2, 36, None),
         (67, 3, 33, 4, None), (1, 8, 16, 16, None), (5, 1, 33, 1, None), (67, 8, 33, 16, OVERFLOW_CAPACITY),
         (5, 3, 16, 36, OVERFLOW_CAPACITY))
RANDOM_CASES = CASES
RANDOM_NET_SEED = 1234


def net_state_dict(name):
    return {"zero": R.zero_state_dict, "greedy": R.greedy_state_dict, "counting": R.counting_state_dict,
            "random": lambda: R.random_state_dict(RANDOM_NET_SEED)}[name]()


def capacity_of(case):
    G, K, n, m, cap = case
    return cap if cap is not None else 2 + 4 * (n + 1)      # two searches of n + 1 rollouts, the first root, a fresh root


@functools.lru_cache(maxsize=None)
def positions(G, seed=POSITION_SEED):
    """G positions 0..7 uniform-random plies from the empty board (the oracle's draws, a finished game staying where it
    ended), as import arrays: what tree_harness.random_positions makes on the device, made without one."""
    ob = oracle.OracleBoards(G)
    snaps = [ob.b.copy()]
    for t in range(7):
        done = oracle.node_info(ob)[1] != 0
        before = ob.b.copy()
        acts = ob.sample_actions(seed, t)
        acts[done] = (0, 1)
        ob.step(acts, None, seed, t)
        ob.b[done] = before[done]
        snaps.append(ob.b.copy())
    depth = np.random.default_rng(seed).integers(0, len(snaps), G)
    pick = oracle.OracleBoards.from_records([snaps[d][g] for g, d in enumerate(depth)])
    return {"board": pick.board.copy(), "moves": pick.moves.copy(), "n_moves": pick.n_moves.copy(),
            "qmask": pick.qmask.copy(), "n_q": pick.n_q.copy()}


def boards(arrays):
    return oracle.boards_from_arrays(arrays["board"], arrays["moves"], arrays["n_moves"], arrays["qmask"], arrays["n_q"])


def new_model(case, net=None):
    G, K, n, m, cap = case
    model = GM.GumbelModel(1, seed=SEED, board_offset=OFFSET, capacity=cap, net=net, leaves=K, max_considered=m)
    model.reset(boards(positions(G)))
    return model


def move_of(model):
    """The move after the first search: even games play the Gumbel choice, odd games their least visited legal action
    (often a child that was never expanded: a fresh root); finished games do not move.  (action36, collapse bits)."""
    act = np.full(len(model.games), 255, dtype=np.uint8)
    for g, (st, f) in enumerate(zip(model.games, model.finals())):
        root = st["nodes"][st["root"]]
        if not root.terminal and root.legal:
            act[g] = f[0] if g % 2 == 0 and f[0] != 255 else min(root.legal, key=lambda a: root.N[a])
    return act, (np.arange(len(model.games)) // 2 % 2).astype(np.uint8)


def model_search(case, net):
    """The whole search of a case on the model alone, under the model's own network and numpy's log and exp."""
    G, K, n, m, cap = case
    model = new_model(case, net)
    model.contemplate_gumbel(n + 1)
    model.final_margins = [f[3] for f in model.finals()]
    act, bits = move_of(model)
    after, _ = tree_model.after_move(model.root_positions(), act, bits)
    model.sync(after)
    model.compact()
    model.contemplate_gumbel(n + 1)
    model.final_margins = [min(a, f[3]) for a, f in zip(model.final_margins, model.finals())]
    return model


def close_calls(model):
    """bool[G]: the games in which some root decision of the model (a descent's, or a final choice) had a top-two gap
    below GAP."""
    return np.minimum(model.min_margin(), np.asarray(getattr(model, "final_margins", np.inf))) < GAP
