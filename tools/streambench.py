#!/usr/bin/env python3
"""Samples harvested per second: lockstep self-play (batch = sp.play(); ring.add(batch)) against continuous self-play
(sp.stream(ring, T)), interleaved in one process.  T is chosen so that both routes harvest about the same
number of samples: a lockstep round harvests G games of mean length m rows, a stream ply G / (m - 1) of them.  Device
events around every round; medians of --rounds rounds after --warmup, min - max beside them; the histogram of the
lockstep games' lengths, which bounds the gain (9 searched plies per game against m - 1).  One JSON line per size.

    python tools/streambench.py [--games 4096,65536] [--rollouts 32] [--leaves 8] [--rounds 9] [--warmup 2] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from qtttgym_amd import PolicyValueNet, ReplayBuffer, SelfPlay, recommended_env  # noqa: E402
recommended_env(apply=True)


def golden_net(dev):
    from nn_reference64 import golden_state_dict, load_golden
    return PolicyValueNet(golden_state_dict(load_golden()), device=dev, dtype=torch.float32)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3, out


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", default="4096,65536")
    ap.add_argument("--rollouts", type=int, default=32)
    ap.add_argument("--leaves", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    net = golden_net(dev)
    lines = []
    for G in (int(x) for x in args.games.split(",")):
        kw = dict(n_rollouts=args.rollouts, net=net, leaf_eval="value", leaves=args.leaves, value_targets=(1.0, -1.0), device=dev)
        lock, cont = SelfPlay(G, seed=1, **kw), SelfPlay(G, seed=1 << 20, **kw)
        ring_l, ring_c = ReplayBuffer(1 << 22, device=dev), ReplayBuffer(1 << 22, device=dev)
        # the lengths of this network's games (rows: the terminal one included), and T from their mean
        length = lock.play().length.to(torch.int64)
        hist = torch.bincount(length, minlength=11).tolist()
        m = float(length.double().mean())
        T = max(1, round(m - 1.0))                               # the plies in which a slot harvests one game on average
        cont.stream(ring_c, 9)                                   # past the first incarnations, which all start together

        def lockstep():
            batch = lock.play()
            ring_l.add(batch)
            return batch.length.sum()
        t_l, t_c, n_l, n_c, before = [], [], [], [], int(cont.stream(ring_c, 0).samples)
        for r in range(args.warmup + args.rounds):
            dt_l, rows = timed(lockstep)
            dt_c, stats = timed(lambda: cont.stream(ring_c, T))
            now = int(stats.samples)
            if r >= args.warmup:
                t_l.append(dt_l)
                t_c.append(dt_c)
                n_l.append(int(rows))
                n_c.append(now - before)
            before = now
        rate_l = [n / t for n, t in zip(n_l, t_l)]
        rate_c = [n / t for n, t in zip(n_c, t_c)]
        line = {"games": G, "rollouts": args.rollouts, "leaves": args.leaves, "rounds": args.rounds, "stream_plies": T,
                "mean_rows_per_game": m, "length_histogram_rows_0_to_10": hist,
                "bound_9_over_moves": 9.0 / (m - 1.0),
                "lockstep": {"seconds": spread(t_l), "samples": spread(n_l), "samples_per_second": spread(rate_l)},
                "stream": {"seconds": spread(t_c), "samples": spread(n_c), "samples_per_second": spread(rate_c)},
                "ratio_of_medians": statistics.median(rate_c) / statistics.median(rate_l)}
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
