#!/usr/bin/env python3
"""Times one leaf-parallel round of the device search trees with and without exact leaves, on one device,
with device events, the routes interleaved in one process: the median of --reps rounds with min .. max.

The trees are in mid-game: --games boards after --plies moves of the uniform-legal policy (finished boards stay), reset,
then 1 + --warm rounds of --leaves rollouts; every route searches its own copy of those trees, and every timed round
goes on from where the route's last one ended (a round changes the tree it searches), so round i of every route sees a
tree of the same age.  Routes:
  a        select_batch -> evaluate -> backup_batch                        (no exact leaves: the search as it was)
  b6, b7   select_batch -> evaluate -> solve_leaves -> backup_batch_exact  (exact_from = 6, 7)
  c6, c7   select_batch -> evaluate -> VecEnv.solve over the round's leaf_state + torch.where -> backup_batch
           (the composition that qttt_tree_solve_leaves replaces; it keeps nothing in the nodes, so it enumerates every
           eligible row of every round again, and its leaves still get priors)
  p6, p7   the b route -> qttt_tree_prove                                  (exact_from = 6, 7 with prove=True, DESIGN.md §26;
           with --prove)
For the p routes the share of the round's records that ended on a proven interior node (a solved leaf node with an
expanded child) is reported, and the difference of the medians to the b route with whether both spreads separate them.
For the b routes the share of the round's records that were eligible and the share that were enumerated (new solved
nodes per record) are reported.  One JSON line per (games, route).

    python tools/exactbench.py [--games 4096,65536] [--leaves 8] [--reps 9] [--out profiles/exact/exactbench.jsonl]
    python tools/exactbench.py --prove --out profiles/prove/exactbench.jsonl"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from qtttgym_amd import PolicyValueNet, TreeSearch, VecEnv, recommended_env  # noqa: E402
recommended_env(apply=True)


def golden_net():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from nn_reference64 import golden_state_dict, load_golden
    return PolicyValueNet(golden_state_dict(load_golden()), device="cuda", dtype=torch.float32)


def composed_round(t, k, min_ply):
    """Route c: the parent's round with the exact values composed in by VecEnv.solve and torch.where."""
    b = t._round_buffers(k)
    G, cap, tree = t.num_games, t.capacity, t.tree.data_ptr()
    t._call("qttt_tree_select_batch", tree, G, cap, t.seed, t.rollout_idx, k, t.board_offset, t.c_puct, t.virtual_loss,
            b["paths"].data_ptr(), b["leaf"].state.data_ptr())
    b["leaf"].evaluate(t.net, out=b["out"])
    sol = b["leaf"].solve(min_ply=min_ply, out=b.get("sol"))
    b["sol"] = sol
    value = torch.where(sol.solved, sol.value, b["out"]["value"])
    t._call("qttt_tree_backup_batch", tree, G, cap, k, b["paths"].data_ptr(), value.data_ptr(), b["out"]["probs"].data_ptr())
    t.rollout_idx += k


def ended_on_proven_share(t, k):
    """The share of the last round's records of depth >= 1 whose leaf is a solved node with an expanded child."""
    from qtttgym_amd import _native
    G, cap, gb, nb = t.num_games, t.capacity, _native.TREE_GAME_BYTES, _native.TREE_NODE_BYTES
    rec = t._rounds[k]["paths"][:G * k * 64].view(G * k, 64)
    leaf = rec[:, :4].contiguous().view(torch.int32).view(-1).long().clamp(0, cap - 1)
    game = torch.arange(G, device=leaf.device).repeat_interleave(k)
    node = t.tree[G * gb:G * gb + G * cap * nb].view(G * cap, nb)[game * cap + leaf]
    flags = node[:, 28:32].contiguous().view(torch.int32).view(-1)
    child = node[:, 32:].reshape(-1, 36, 16)[:, :, 12:16].contiguous().view(torch.int32).view(-1, 36)
    hit = (rec[:, 4] >= 1) & ((flags & _native.TREE_NODE_SOLVED) != 0) & (child >= 0).any(1)
    return float(hit.float().mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prove", action="store_true", help="add the p6 / p7 routes (prove=True)")
    ap.add_argument("--games", default="4096,65536")
    ap.add_argument("--leaves", type=int, default=8)
    ap.add_argument("--plies", type=int, default=5)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    net, K = golden_net(), args.leaves
    rows = []
    for G in (int(x) for x in args.games.split(",")):
        env = VecEnv(G, seed=args.seed)
        env.step_random_many(args.plies)
        rounds = args.warm + 1 + args.reps
        capacity = 2 + 2 * (1 + K * rounds)
        routes = {"a": None, "b6": 6, "b7": 7, "c6": 6, "c7": 7}
        if args.prove:
            routes.update(p6=6, p7=7)
        trees = {}
        for name, M in routes.items():
            t = TreeSearch(G, capacity=capacity, net=net, seed=2 * args.seed + 1, leaf_eval="value", leaves=K,
                           exact_from=M if name[0] in "bp" else None, prove=name.startswith("p"))
            t.reset(env)
            t._round(1)
            for _ in range(args.warm + 1):               # the last of them warms the route's own launches up
                composed_round(t, K, M) if name.startswith("c") else t._round(K)
            trees[name] = t
        torch.cuda.synchronize()
        ms = {name: [] for name in routes}
        eligible = {name: [] for name in routes}
        enumerated = {name: [] for name in routes}
        on_proven = {name: [] for name in routes}
        for _ in range(args.reps):
            for name, M in routes.items():
                t = trees[name]
                before = int(t.solved_count().sum()) if name[0] in "bp" else 0
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                composed_round(t, K, M) if name.startswith("c") else t._round(K)
                b.record()
                b.synchronize()
                ms[name].append(a.elapsed_time(b))
                if name.startswith("p"):
                    on_proven[name].append(ended_on_proven_share(t, K))
                if name[0] in "bp":
                    eligible[name].append(float(t._rounds[K]["exact"].float().mean()))
                    enumerated[name].append((int(t.solved_count().sum()) - before) / (G * K))
        for name in routes:
            row = {"games": G, "leaves": K, "route": name, "ms": statistics.median(ms[name]), "ms_min": min(ms[name]),
                   "ms_max": max(ms[name]), "reps": args.reps, "plies": args.plies, "warm_rounds": args.warm}
            if name.startswith("p"):
                b = "b" + name[1]
                row.update(ended_on_proven_share=float(np.mean(on_proven[name])),
                           added_to_b_ms=row["ms"] - statistics.median(ms[b]),
                           separated_from_b_beyond_both_spreads=bool(max(ms[b]) < min(ms[name]) or max(ms[name]) < min(ms[b])))
            if name[0] in "bp":
                row.update(eligible_share=float(np.mean(eligible[name])), enumerated_share=float(np.mean(enumerated[name])),
                           added_to_a_ms=row["ms"] - statistics.median(ms["a"]))
            rows.append(row)
            print(json.dumps(row), flush=True)
        for M in (6, 7):
            b, c = "b%d" % M, "c%d" % M
            separated = max(ms[b]) < min(ms[c]) or max(ms[c]) < min(ms[b])
            print(json.dumps({"games": G, "compare": [b, c], "medians_ms": [statistics.median(ms[b]), statistics.median(ms[c])],
                              "separated_beyond_both_spreads": bool(separated)}), flush=True)
        del trees
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
