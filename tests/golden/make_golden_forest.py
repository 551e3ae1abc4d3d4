#!/usr/bin/env python3
"""Generates tests/golden/step_forest_traces.npz: the UNMODIFIED reference (loaded through ref_shim.py, recorded by
make_golden.run_trace) on episodes that FORCE the forest shapes random play almost never reaches — long paths re-rooted
from their far end, random trees of six to nine squares, four full qstruct slots merged down to one component — each
closed by a cycle and recorded twice, once per collapse bit.

    python tests/golden/make_golden_forest.py             # rewrites step_forest_traces.npz
    python tests/golden/make_golden_forest.py --out DIR   # writes DIR/step_forest_traces.npz instead

Same arrays, dtypes and T as step_traces.npz (make_golden.py), plus
  twin[e]   the row that differs from row e in the closing move's bit only; a pair is two neighbouring rows.
An episode: the shape's moves (none closes a cycle), the closing move, then uniform legal play to T.  The two rows of a
pair play the same actions: the collapsed SQUARES do not depend on the bit, only the rounds that land on them.
Families (288 episodes each, every family its own seed):
  path    a random order of k in {7, 8, 9} squares, the k - 1 path edges in random order and orientation; closed end to
          end, or between two random squares of the path
  tree    a uniform random labelled tree on k in {6..9} squares (Pruefer sequence), closed by a random pair of its squares
          (re-playing an edge included)
  pairs   four disjoint pairs, random unions down to one component, the ninth square, a closing move
  noisy   one of the above with noops of every flavour between the moves (same square, classical square, out of range on
          either side)
Prints the walk histogram (tests/forest_model.py) per family and kind of move."""
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import T, legal_pairs, run_trace  # noqa: E402
from ref_shim import load_reference  # noqa: E402
import forest_model  # noqa: E402

PER_FAMILY = 288
SEEDS = {"path": 20261101, "tree": 20261102, "pairs": 20261103, "noisy": 20261104}


def _oriented(rng, u, v):
    return (u, v) if rng.getrandbits(1) else (v, u)


def shape_path(rng):
    k = rng.choice((7, 8, 9, 9, 9, 9))
    order = rng.sample(range(9), k)
    edges = [(order[i], order[i + 1]) for i in range(k - 1)]
    rng.shuffle(edges)
    close = (order[0], order[-1]) if rng.getrandbits(1) else tuple(rng.sample(order, 2))
    return edges, close


def shape_tree(rng):
    k = rng.randrange(6, 10)
    label = rng.sample(range(9), k)
    prufer = [rng.randrange(k) for _ in range(k - 2)]
    degree = [1] * k
    for v in prufer:
        degree[v] += 1
    edges = []
    for v in prufer:
        leaf = min(i for i in range(k) if degree[i] == 1)
        edges.append((label[leaf], label[v]))
        degree[leaf] -= 1
        degree[v] -= 1
    u, w = (i for i in range(k) if degree[i] == 1)
    edges.append((label[u], label[w]))
    rng.shuffle(edges)
    return edges, tuple(rng.sample(label, 2))


def shape_pairs(rng):
    sq = rng.sample(range(9), 9)
    comps = [[sq[2 * i], sq[2 * i + 1]] for i in range(4)]
    edges = [tuple(c) for c in comps]
    while len(comps) > 1:
        i, j = rng.sample(range(len(comps)), 2)
        edges.append((rng.choice(comps[i]), rng.choice(comps[j])))
        comps[i] = comps[i] + comps[j]
        comps.pop(j)
    edges.append((sq[8], rng.choice(comps[0])))
    return edges, tuple(rng.sample(range(9), 2))


SHAPES = {"path": shape_path, "tree": shape_tree, "pairs": shape_pairs}


def noop_action(rng, board):
    classical = [i for i in range(9) if board[i] != -1]
    while True:
        f = rng.randrange(5)
        if f == 0:
            a = b = rng.randrange(0, 9)                              # same square
        elif f == 1:
            if not classical:
                continue
            a, b = rng.choice(classical), rng.randrange(0, 9)        # a classical square (or the same one twice)
            if rng.getrandbits(1):
                a, b = b, a
        elif f == 2:
            a, b = rng.randrange(9, 256), rng.randrange(0, 9)        # IndexError first
        elif f == 3:
            a, b = rng.randrange(0, 9), rng.randrange(9, 256)        # IndexError second
        else:
            a = b = rng.randrange(9, 256)                            # same square, out of range
        return a, b


def gen_episode(family, rng, qtttgym, src):
    """(actions, bits, closing step) of one episode, chosen on a scratch reference Env."""
    shape = family if family != "noisy" else rng.choice(("path", "path", "tree", "pairs"))
    edges, close = SHAPES[shape](rng)
    plan = [_oriented(rng, u, v) for u, v in edges] + [_oriented(rng, *close)]
    closing = len(plan) - 1
    if family == "noisy":
        for _ in range(rng.randint(1, T - len(plan))):
            at = rng.randrange(0, len(plan) + 1)
            plan.insert(at, None)
            closing += at <= closing
    env = qtttgym.Env()
    env.reset()
    acts, bits = [], []
    for t in range(T):
        board = env._gameboard.board
        bit = rng.getrandbits(1)
        if t < len(plan):
            a, b = plan[t] if plan[t] is not None else noop_action(rng, board)
        else:
            legal = legal_pairs(board)
            if legal:
                a, b = _oriented(rng, *rng.choice(legal))
            else:
                a, b = rng.randrange(0, 9), rng.randrange(0, 9)
        n_before, calls = len(env._gameboard.moves), src.calls
        src.bit = bit
        env.step((a, b))
        if t < len(plan) and plan[t] is not None:                    # the plan is legal, and only its last move collapses
            assert len(env._gameboard.moves) > n_before and (src.calls > calls) == (t == closing), (family, t)
        acts.append((a, b))
        bits.append(bit)
    return acts, bits, closing


def generate():
    qtttgym, src = load_reference()
    episodes, names, twin = [], [], []
    for family in ("path", "tree", "pairs", "noisy"):
        rng = random.Random(SEEDS[family])
        for _ in range(PER_FAMILY):
            acts, bits, closing = gen_episode(family, rng, qtttgym, src)
            other = list(bits)
            other[closing] ^= 1
            e = len(episodes)
            episodes += [(acts, bits), (acts, other)]
            names += [family, family]
            twin += [e + 1, e]
    cols = {}
    for acts, bits in episodes:
        for k, v in run_trace(qtttgym, src, acts, bits).items():
            cols.setdefault(k, []).append(v)
    E = len(episodes)
    dtypes = {"board": np.int8, "moves": np.uint8, "n_moves": np.uint8, "qmask": np.uint16, "n_q": np.uint8,
              "q_p1": np.uint8, "q_p1_len": np.uint8, "q_p2": np.uint8, "q_p2_len": np.uint8, "turn": np.uint8,
              "reward": np.float64, "terminated": np.uint8, "p1_round": np.int8, "p2_round": np.int8, "consumed": np.uint8}
    data = {"actions": np.array([a for a, _ in episodes], dtype=np.uint8).reshape(E, T, 2),
            "bits": np.array([b for _, b in episodes], dtype=np.uint8).reshape(E, T)}
    data.update({k: np.array(cols[k], dtype=dt) for k, dt in dtypes.items()})
    data["kind"] = np.array(names)
    data["twin"] = np.array(twin, dtype=np.int32)
    assert set(np.unique(data["consumed"])) <= {0, 1}
    return data


def print_histogram(data):
    print("walk length              0     1     2     3     4     5     6     7     8")
    for (fam, kind), h in forest_model.histogram(data).items():
        print("%-8s %-6s %s" % (fam, kind, "".join("%6d" % x for x in h)))


def main(argv):
    out_dir = argv[argv.index("--out") + 1] if "--out" in argv else HERE
    data = generate()
    out = os.path.join(out_dir, "step_forest_traces.npz")
    np.savez_compressed(out, **data)
    E = data["bits"].shape[0]
    print("wrote %s: %d episodes x %d steps; collapses=%d wins=%d terminated=%d size=%d B"
          % (out, E, T, int(data["consumed"].sum()), int((data["reward"] == -1.0).sum()),
             int(data["terminated"].sum()), os.path.getsize(out)))
    print_histogram(data)


if __name__ == "__main__":
    main(sys.argv[1:])
