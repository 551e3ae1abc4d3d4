#!/usr/bin/env python3
"""Times one contemplate(--rollouts) of the device search trees with the resident search off and on, on one
device, with device events, the two routes interleaved in one process: the median of --reps with min .. max, and whether the
spreads separate the two.

Every route is a TreeSearch of its own with the same seed, leaves = --leaves and leaf_eval="value" over the same random
opening positions (two random plies from the empty board).  A warm move comes first, untimed: contemplate, the chosen move,
sync, one more contemplate (so the timed search starts from a root with priors and statistics, and every kernel and buffer
has been used).  Rep i of every route then times its next contemplate(--rollouts) on the tree as it stands: the trees of the
two routes hold the same bytes throughout (tests/test_tree_resident_gpu.py), so they time the same work.  Routes:
  launches   resident=False: the reference, the code path the library had before the keyword, 3 launches a round
  resident   resident=True: the rounds inside qttt_tree_search_resident
One JSON line per (games, precision, route) and one per comparison.

    python tools/residentbench.py [--games 4096,65536] [--rollouts 32] [--leaves 8] [--reps 9] [--out-dir profiles/resident_search]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from qtttgym_amd import PolicyValueNet, TreeSearch, VecEnv, recommended_env  # noqa: E402
from qtttgym_amd.actions import action36_to_pairs  # noqa: E402
recommended_env(apply=True)


def golden_net(dtype):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from nn_reference64 import golden_state_dict, load_golden
    return PolicyValueNet(golden_state_dict(load_golden()), device="cuda", dtype=dtype)


def timed(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", default="4096,65536")
    ap.add_argument("--rollouts", type=int, default=32)
    ap.add_argument("--leaves", type=int, default=8)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out-dir", default=None)
    args = ap.parse_args()
    R, rows = args.rollouts, []
    for G in (int(x) for x in args.games.split(",")):
        for prec, dtype in (("f32", torch.float32), ("bf16", torch.bfloat16)):
            net = golden_net(dtype)
            routes = {}
            for name, resident in (("launches", False), ("resident", True)):
                env = VecEnv(G, device="cuda", seed=args.seed)
                env.step_random_many(2)
                tree = TreeSearch(G, capacity=4 + 2 * R * (args.reps + 3), net=net, seed=args.seed, device="cuda",
                                  leaf_eval="value", leaves=args.leaves, resident=resident)
                tree.reset(env)
                tree.contemplate(R)                              # the warm move
                env.step_raw(action36_to_pairs(tree.choose()).contiguous())
                tree.sync(env)
                tree.contemplate(R)
                routes[name] = tree
            same = bool(torch.equal(routes["launches"].tree, routes["resident"].tree))
            ms = {name: [] for name in routes}
            for _ in range(args.reps):
                for name, tree in routes.items():
                    ms[name].append(timed(lambda: tree.contemplate(R)))
            same = same and bool(torch.equal(routes["launches"].tree, routes["resident"].tree))
            for name in routes:
                rows.append({"games": G, "precision": prec, "rollouts": R, "leaves": args.leaves, "route": name,
                             "ms": statistics.median(ms[name]), "ms_min": min(ms[name]), "ms_max": max(ms[name]), "reps": args.reps})
                print(json.dumps(rows[-1]), flush=True)
            a, b = ms["launches"], ms["resident"]
            rows.append({"games": G, "precision": prec, "compare": ["launches", "resident"],
                         "medians_ms": [statistics.median(a), statistics.median(b)],
                         "ratio": statistics.median(b) / statistics.median(a),
                         "separated_beyond_both_spreads": bool(max(a) < min(b) or max(b) < min(a)),
                         "trees_identical": same})
            print(json.dumps(rows[-1]), flush=True)
            del routes
            torch.cuda.empty_cache()
    if args.out_dir:
        os.makedirs(args.out_dir, exist_ok=True)
        with open(os.path.join(args.out_dir, "residentbench.jsonl"), "w") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
