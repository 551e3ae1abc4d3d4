#!/usr/bin/env python3
"""Times one stream ply of self-play with and without playout cap randomisation, on one device, with device
events, the routes interleaved in one process: the median of --reps with min .. max, and whether the spreads separate a route
from the reference.

Every route is a SelfPlay of its own with the same seed, n_rollouts = --rollouts, leaves = --leaves, root noise (0.25, 0.3)
and compact=False, streaming into a ring of its own; --warm plies run untimed first (the first plies of a stream are all
opening positions), then rep i of every route times its next ply, so the routes see streams of the same age.  Routes:
  uncapped   playout_cap=None: the reference, the code path the library had before the keyword
  capped     playout_cap=(--p, --n-fast): KataGo's setting, 0.25 and a quarter of the rollouts
  all-full   playout_cap=(1.0, --rollouts): every game full, every round through the subset entries: what the indirection costs
One JSON line per (games, route) and one per comparison with the reference.

    python tools/capbench.py [--games 4096,65536] [--rollouts 32] [--leaves 8] [--reps 9] [--out profiles/cap/capbench.jsonl]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from qtttgym_amd import PolicyValueNet, ReplayBuffer, SelfPlay, recommended_env  # noqa: E402
recommended_env(apply=True)


def golden_net():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from nn_reference64 import golden_state_dict, load_golden
    return PolicyValueNet(golden_state_dict(load_golden()), device="cuda", dtype=torch.float32)


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
    ap.add_argument("--p", type=float, default=0.25)
    ap.add_argument("--n-fast", type=int, default=8)
    ap.add_argument("--warm", type=int, default=6)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    net, rows = golden_net(), []
    for G in (int(x) for x in args.games.split(",")):
        caps = {"uncapped": None, "capped": (args.p, args.n_fast), "all-full": (1.0, args.rollouts)}
        routes = {}
        for name, cap in caps.items():
            sp = SelfPlay(G, n_rollouts=args.rollouts, net=net, seed=args.seed, leaf_eval="value", leaves=args.leaves,
                          root_noise=(0.25, 0.3), value_targets=(1.0, -1.0), playout_cap=cap)
            ring = ReplayBuffer(max(4 * G, 1024), seed=args.seed)
            sp.stream(ring, args.warm, seed=args.seed)
            routes[name] = (sp, ring)
        ms = {name: [] for name in routes}
        for _ in range(args.reps):
            for name, (sp, ring) in routes.items():
                ms[name].append(timed(lambda: sp.stream(ring, 1)))
        for name in routes:
            rows.append({"games": G, "rollouts": args.rollouts, "leaves": args.leaves, "route": name, "playout_cap": caps[name],
                         "ms": statistics.median(ms[name]), "ms_min": min(ms[name]), "ms_max": max(ms[name]), "reps": args.reps})
            print(json.dumps(rows[-1]), flush=True)
        ref = ms["uncapped"]
        for name in ("capped", "all-full"):
            x = ms[name]
            rows.append({"games": G, "compare": ["uncapped", name], "medians_ms": [statistics.median(ref), statistics.median(x)],
                         "ratio": statistics.median(x) / statistics.median(ref),
                         "separated_beyond_both_spreads": bool(max(ref) < min(x) or max(x) < min(ref))})
            print(json.dumps(rows[-1]), flush=True)
        samples = {name: int(sp._stream["tally"][:, 3].sum()) for name, (sp, _) in routes.items()}
        rows.append({"games": G, "rows_harvested_after_%d_plies" % (args.warm + args.reps): samples})
        print(json.dumps(rows[-1]), flush=True)
        del routes
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
