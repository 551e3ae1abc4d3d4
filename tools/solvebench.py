#!/usr/bin/env python3
"""Times VecEnv.solve on the device: us per board at min_ply 5, 6 and 7 for 64 and 4 096 boards of the
uniform-legal policy's positions with exactly that many moves played, and the worst boards — the fixture's largest
board with five and with four moves played, and the largest of --search random boards of each depth — alone and as one
full occupancy round of copies, from which the boards_per_launch defaults follow.  Device events, the median of --reps
launches after a warm-up, with the spread (min .. max).  One JSON line per measurement.

    python tools/solvebench.py [--reps 9] [--search 256] [--resident 1280] [--out profiles/solve/solvebench.jsonl]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from qtttgym_amd import VecEnv, recommended_env  # noqa: E402
recommended_env(apply=True)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def unfinished_at(k, n, seed):
    """n unfinished boards with exactly k moves played, from the uniform-legal policy (repeated if too few survive)."""
    env = VecEnv(max(4 * n, 1024), seed=seed)
    env.step_random_many(k)
    info = env.node_info(python_key=False)
    sel = (~info["terminal"].bool() & (info["legal"] != 0)).nonzero(as_tuple=True)[0]
    return env.take(sel[torch.arange(n, device=sel.device) % sel.numel()])


def fixture_board(k):
    with np.load(os.path.join(ROOT, "tests", "golden", "solve_positions.npz")) as d:
        g = {key: d[key] for key in d.files}
    idx = np.flatnonzero(g["played"] == k)
    i = idx[np.argmax(g["nodes"][idx])]
    env = VecEnv(1)
    env.import_boards(*(torch.from_numpy(g[key][i:i + 1].copy()) for key in ("moves", "n_moves", "board")),
                      torch.from_numpy(g["qmask"][i:i + 1].view(np.int16).copy()), torch.from_numpy(g["n_q"][i:i + 1].copy()))
    return env, int(g["nodes"][i])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--search", type=int, default=256, help="random boards per depth among which the largest is looked for")
    ap.add_argument("--resident", type=int, default=1280, help="boards of one occupancy round: CUs x workgroups per CU")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = []

    def emit(**row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    for k in (5, 6, 7):
        for n in (64, 4096):
            env = unfinished_at(k, n, seed=k)
            per = None if k >= 6 else n                     # one launch: this measures the kernel, not the split
            res = env.solve(min_ply=k, boards_per_launch=per)
            med, lo, hi = timed(lambda: env.solve(min_ply=k, out=res, boards_per_launch=per), args.reps)
            emit(what="batch", min_ply=k, boards=n, ms=med, ms_min=lo, ms_max=hi, us_per_board=1e3 * med / n,
                 nodes_mean=float(res.nodes.double().mean()), nodes_max=int(res.nodes.max()))
    for k in (5, 4):
        fix, fix_nodes = fixture_board(k)
        cand = unfinished_at(k, args.search, seed=100 + k)
        nodes = cand.solve(min_ply=k, boards_per_launch=64).nodes
        worst = cand.take(nodes.argmax()[None])
        for name, env, nn in (("fixture", fix, fix_nodes), ("largest of %d" % args.search, worst, int(nodes.max()))):
            res = env.solve(min_ply=k, boards_per_launch=1)
            assert int(res.nodes[0]) == nn
            med, lo, hi = timed(lambda: env.solve(min_ply=k, out=res, boards_per_launch=1), min(args.reps, 5))
            emit(what="one board alone", board=name, min_ply=k, nodes=nn, ms=med, ms_min=lo, ms_max=hi,
                 nodes_per_us=nn / (1e3 * med))
            full = env.take(torch.zeros(args.resident, dtype=torch.int64, device=env.device))
            out = full.solve(min_ply=k, boards_per_launch=args.resident)
            med, lo, hi = timed(lambda: full.solve(min_ply=k, out=out, boards_per_launch=args.resident), min(args.reps, 3))
            emit(what="one occupancy round of copies", board=name, min_ply=k, nodes=nn, boards=args.resident, ms=med,
                 ms_min=lo, ms_max=hi)
    if args.out:
        with open(args.out, "w") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
