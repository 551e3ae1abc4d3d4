#!/usr/bin/env python3
"""Times the two launches of include/qttt_selfplay_value.h beside the compositions they replace, on the
golden network with value leaves:

  record_value   one qttt_selfplay_record_value launch on searched roots (8 rollouts), beside root_stats() (all of its
                 rows) plus Reanalyser's torch lines that turn N and Q into the searched value and store a row of q;
  value_targets  one qttt_selfplay_value_targets launch (TD, lambda 0.8) over a play() batch, v restored before every
                 repeat, beside a torch backward loop over the ten rows (f64, the same recursion);
  play_ply       wall time of a play() ply at 32 rollouts without the keywords, and the share of it that one
                 record_value launch is.

The two of a pair alternate in one process; device events; medians of --repeats after two warm-up rounds, with min - max
and whether the spreads separate.  One JSON line each.

    python tools/valuebench.py [--games 4096,65536] [--repeats 9] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from qtttgym_amd import PolicyValueNet, SelfPlay, recommended_env  # noqa: E402
recommended_env(apply=True)

ROWS, SEED, DEV, LAM = 10, 2026, "cuda:0", 0.8


def golden_net():
    import nn_reference64 as R
    return PolicyValueNet(R.golden_state_dict(R.load_golden()), device=DEV, dtype=torch.float32)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3                       # us


def summary(xs):
    return {"median_us": round(statistics.median(xs), 2), "min_us": round(min(xs), 2), "max_us": round(max(xs), 2)}


def separate(a, b):
    return max(a) < min(b) or max(b) < min(a)


def composed_record(tree, q_row, v_row):
    """root_stats() and Reanalyser.run's lines: the searched value of every root, into one row of q."""
    st = tree.root_stats()
    N = st["N"].double()
    total = N.sum(1)
    searched = torch.where(N > 0, N * st["Q"], torch.zeros_like(N)).sum(1) / total.clamp(min=1.0)
    q_row.copy_(torch.where(total > 0, searched.float(), v_row))


def composed_td(batch, lam):
    """The backward pass of QTTT_VALUE_TD as torch ops over the ten rows, in f64."""
    v, q, done, L = batch.v, batch.q, batch.done, batch.length.long()
    g = torch.zeros(batch.num_games, dtype=torch.float64, device=v.device)
    for t in range(ROWS - 1, -1, -1):
        if t < ROWS - 1:
            b = torch.where(done[t + 1] != 0, v[t + 1], q[t + 1]).double()
            new = 0.0 - ((1.0 - lam) * b + lam * g)
        else:
            new = g
        inside = t < L - 1
        g = torch.where(L - 1 == t, v[t].double(), torch.where(inside, new, g))
        v[t] = torch.where(inside, g.float(), v[t])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", default="4096,65536")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    net = golden_net()
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    for G in (int(x) for x in args.games.split(",")):
        kw = dict(net=net, seed=SEED, device=DEV, leaf_eval="value", value_targets=(1.0, -1.0))
        # ---- record_value on searched roots
        sp = SelfPlay(G, n_rollouts=8, td_lambda=1.0, **kw)          # lambda 1: v stays the outcome, q is recorded
        env, tree = sp._new_game_objects(SEED)
        sp._search(tree)
        probe = sp.new_batch()
        other = torch.zeros_like(probe.q)
        a, b = [], []
        for rep in range(args.repeats + 2):
            ta = timed(lambda: sp.record_value(tree, 0, probe))
            tb = timed(lambda: composed_record(tree, other[0], probe.v[0]))
            assert float((probe.q[0] - other[0]).abs().max()) <= 1e-6
            if rep >= 2:
                a.append(ta), b.append(tb)
        record_us = statistics.median(a)
        emit({"what": "record_value", "games": G, "route": "launch", **summary(a)})
        emit({"what": "record_value", "games": G, "route": "root_stats+torch", **summary(b), "spreads_separate": separate(a, b)})
        del env, tree, probe, other
        # ---- value_targets on a play() batch
        batch = sp.play(SEED)
        sp.tree = sp.env = None
        v0 = batch.v.clone()
        a, b = [], []
        for rep in range(args.repeats + 2):
            batch.v.copy_(v0)
            ta = timed(lambda: batch.value_targets("td", LAM))
            got = batch.v.clone()
            batch.v.copy_(v0)
            tb = timed(lambda: composed_td(batch, LAM))
            assert float((batch.v - got).abs().max()) <= 1e-6
            if rep >= 2:
                a.append(ta), b.append(tb)
        emit({"what": "value_targets", "games": G, "mode": "td", "lambda": LAM, "route": "launch",
              "rows_changed": int((got.view(torch.int32) != v0.view(torch.int32)).sum()), **summary(a)})
        emit({"what": "value_targets", "games": G, "mode": "td", "lambda": LAM, "route": "torch loop", **summary(b),
              "spreads_separate": separate(a, b)})
        del batch, v0, got, sp
        torch.cuda.empty_cache()
        # ---- a play() ply at 32 rollouts, without the keywords
        sp = SelfPlay(G, n_rollouts=32, **kw)
        times = []
        for rep in range(4):                                         # one warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sp.play(SEED)
            torch.cuda.synchronize()
            if rep:
                times.append((time.perf_counter() - t0) / ROWS * 1e6)
        ply_us = statistics.median(times)
        emit({"what": "play_ply", "games": G, "n_rollouts": 32, **summary(times), "record_value_median_us": round(record_us, 2),
              "share_of_ply": round(record_us / ply_us, 5)})
        sp.tree = sp.env = None
        del sp
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
