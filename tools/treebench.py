#!/usr/bin/env python3
"""Times qtttgym_amd.TreeSearch's rollout (select -> playouts -> backup) on the MI355X and prints one JSON line per
(games, mode): microseconds per rollout split into select / playouts / backup (HIP events around each launch, summed
over the measured rollouts), the playouts alone re-run on the same leaves as the floor, and the nodes used.

    python tools/treebench.py [--games 4096,65536,262144] [--modes uniform,f32,bf16] [--sims 10] [--rollouts 32]
                              [--warmup 4] [--out profiles/tree/treebench.jsonl]

--value-games 4096,65536,262144 adds the value-rollout leg (TreeSearch(leaf_eval="value")) per dtype of
--value-modes f32,bf16: medians over --value-reps repetitions, the legs interleaved within each repetition, of a value
rollout (select + the fused launch), a playout rollout at --sims, the fused launch alone, and qttt_evaluate (value +
probs) and qttt_tree_backup alone on the same leaves.

--leaves 1,8,32 turns the --value-games legs into the leaf-parallel comparison (TreeSearch(leaves=K)) per
dtype of --value-modes: one value search per K on the same positions, the legs interleaved within each of --value-reps
repetitions after one that warms up.  Every repetition resets each tree, contemplates 8 rollouts and then times 32
rollouts back to back (K = 1: today's select + fused launch; K > 1: rounds of K through select_batch / evaluate /
backup_batch), HIP events around the lot, and once more with events between the launches for the breakdown.  A row per K:
microseconds per rollout (= round time / K), median, min and max, its parts, and the factor over the K = 1 leg of the
same run with that leg's own max - min spread beside it.

    python tools/treebench.py --games "" --value-games 256,4096,65536 --leaves 1,8,32 [--out profiles/tree_leaves/treebench_leaves.jsonl]

--compact-games 4096,65536 adds the compaction leg (uniform playouts): per move contemplate(R) -> choose -> step ->
sync -> compact(), timed with HIP events around contemplate and around compact (its launch alone; the read-back of the
bound comes after the second event), medians over the moves of --compact-reps games from the empty board, with the
mean nodes used before and after each compaction.

    python tools/treebench.py --games "" --compact-games 4096,65536 [--compact-rollouts 300] [--compact-reps 3]

--explore adds the root-exploration leg at --explore-games 4096,65536: microseconds per launch of
qttt_tree_root_noise, of qttt_selfplay_record_sampled and, beside them in the same process, of qttt_selfplay_record and
qttt_tree_root, on searched uniform trees two plies in; HIP events around --explore-launches back-to-back launches, the
legs interleaved, medians of --explore-reps repetitions after one that warms up.

    python tools/treebench.py --games "" --explore [--out profiles/explore/treebench_explore.jsonl]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from qtttgym_amd import PolicyValueNet, TreeSearch, VecEnv, recommended_env  # noqa: E402
from qtttgym_amd import _native  # noqa: E402
recommended_env(apply=True)


def _net(dtype):
    import numpy as np
    from qtttgym_amd.policy_value import SHAPES
    with np.load(os.path.join(ROOT, "tests", "golden", "model_eval.npz")) as d:
        sd = {k: torch.from_numpy(d[k.replace(".", "_")]) for k in SHAPES}
    return PolicyValueNet(sd, device="cuda", dtype=dtype)


def run(G, mode, sims, rollouts, warmup):
    net = None if mode == "uniform" else _net(torch.float32 if mode == "f32" else torch.bfloat16)
    env = VecEnv(G, seed=1)
    env.step_random_many(2)                                  # positions two plies in: most games open
    t = TreeSearch(G, capacity=1 + 2 * (rollouts + warmup), num_simulations=sims, net=net, seed=2)
    t.reset(env)
    t.contemplate(warmup)
    L, stream = t._lib, torch.cuda.current_stream()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(rollouts)]
    tree, leaf = t.tree.data_ptr(), t.leaf.state.data_ptr()
    stride = sims * _native.SIM_STRIDE
    torch.cuda.synchronize()
    for r in range(rollouts):
        k = t.rollout_idx
        e = ev[r]
        e[0].record(stream)
        _native.check(L.qttt_tree_select(tree, G, t.capacity, t.seed, k, t.board_offset, t.c_puct, leaf,
                                         stream.cuda_stream), "select")
        e[1].record(stream)
        if net is None:
            t.leaf.rollout_many(sims, step_idx0=k * stride, out=t._out)
            res, probs = t._out.data_ptr(), None
        else:
            t.leaf.rollout_policy(net, sims, step_idx0=k * stride, out=t._out)
            res, probs = t._out["result"].data_ptr(), t._out["probs"].data_ptr()
        e[2].record(stream)
        _native.check(L.qttt_tree_backup(tree, G, t.capacity, res, sims, probs, stream.cuda_stream), "backup")
        e[3].record(stream)
        t.rollout_idx, t._bound = k + 1, t._bound + 2
    torch.cuda.synchronize()
    sel = sum(e[0].elapsed_time(e[1]) for e in ev) * 1e3 / rollouts
    play = sum(e[1].elapsed_time(e[2]) for e in ev) * 1e3 / rollouts
    back = sum(e[2].elapsed_time(e[3]) for e in ev) * 1e3 / rollouts
    total = sum(e[0].elapsed_time(e[3]) for e in ev) * 1e3 / rollouts
    # the floor: the same playouts on the same (last) leaves, back to back
    f0, f1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    f0.record(stream)
    for r in range(rollouts):
        if net is None:
            t.leaf.rollout_many(sims, step_idx0=r * stride, out=t._out)
        else:
            t.leaf.rollout_policy(net, sims, step_idx0=r * stride, out=t._out)
    f1.record(stream)
    torch.cuda.synchronize()
    used = t.nodes_used().float()
    return {"games": G, "mode": mode, "n_sims": sims, "rollouts": rollouts, "us_per_rollout": round(total, 2),
            "us_select": round(sel, 2), "us_playouts": round(play, 2), "us_backup": round(back, 2),
            "us_playouts_alone": round(f0.elapsed_time(f1) * 1e3 / rollouts, 2),
            "nodes_used_mean": round(float(used.mean()), 2), "nodes_used_max": int(used.max())}


def run_value(G, mode, sims, reps, rollouts=6, warmup=4):
    """One JSON row: medians over `reps` interleaved repetitions of `rollouts` launches per leg."""
    import statistics
    net = _net(torch.float32 if mode == "f32" else torch.bfloat16)
    env = VecEnv(G, seed=1)
    env.step_random_many(2)
    cap = 1 + 2 * (warmup + (reps + 1) * rollouts * 2)
    tv = TreeSearch(G, capacity=cap, net=net, seed=2, leaf_eval="value")
    tp = TreeSearch(G, capacity=1 + 2 * (warmup + (reps + 1) * rollouts), num_simulations=sims, net=net, seed=2)
    for t in (tv, tp):
        t.reset(env)
        t.contemplate(warmup)
    stream = torch.cuda.current_stream()
    ev_out = tv.leaf.evaluate(net, rows=("value", "probs"))
    res = torch.zeros((G, sims), dtype=torch.int8, device=env.device)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(rollouts):
            fn()
        b.record(stream)
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / rollouts

    def fused():                                 # the leaves of the last select again: the tree keeps its shape
        tv._call("qttt_tree_value_rollout", tv.tree.data_ptr(), G, tv.capacity, tv.leaf.state.data_ptr(),
                 net.blob.data_ptr(), net.precision, None, None)

    legs = {"value_rollout": lambda: tv.contemplate(1), "playout_rollout": lambda: tp.contemplate(1), "fused": fused,
            "evaluate": lambda: tv.leaf.evaluate(net, out=ev_out),
            "backup": lambda: tv._call("qttt_tree_backup", tv.tree.data_ptr(), G, tv.capacity, res.data_ptr(), sims,
                                       ev_out["probs"].data_ptr())}
    us = {k: [] for k in legs}
    for rep in range(reps + 1):
        for k, fn in legs.items():
            x = timed(fn)
            if rep:                              # the first repetition warms every leg up
                us[k].append(x)
    row = {"games": G, "mode": mode, "leg": "value", "n_sims": sims, "reps": reps, "launches_per_rep": rollouts}
    for k, xs in us.items():
        row["us_%s_median" % k] = round(statistics.median(xs), 2)
        row["us_%s_min_max" % k] = [round(min(xs), 2), round(max(xs), 2)]
    row["us_evaluate_plus_backup_median"] = round(row["us_evaluate_median"] + row["us_backup_median"], 2)
    return row


def run_leaves(G, mode, Ks, reps, rollouts=32, warmup=8):
    """One JSON row per K: medians over `reps` interleaved repetitions of `rollouts` rollouts per leg."""
    import statistics
    net = _net(torch.float32 if mode == "f32" else torch.bfloat16)
    env = VecEnv(G, seed=1)
    env.step_random_many(2)
    stream = torch.cuda.current_stream()
    cap = 1 + 2 * (warmup + 2 * rollouts + 2 * max(Ks))
    trees = {K: TreeSearch(G, capacity=cap, net=net, seed=2, leaf_eval="value", leaves=K) for K in Ks}
    event = lambda: torch.cuda.Event(enable_timing=True)

    def launches(t, K):
        """The launches of one round of K (one rollout at K = 1), as callables in order."""
        tree = t.tree.data_ptr()
        if K == 1:
            leaf = t.leaf.state.data_ptr()
            return (lambda: t._call("qttt_tree_select", tree, G, cap, t.seed, t.rollout_idx, t.board_offset, t.c_puct, leaf),
                    lambda: t._call("qttt_tree_value_rollout", tree, G, cap, leaf, net.blob.data_ptr(), net.precision, None, None))
        b = t._round_buffers(K)
        paths, out = b["paths"].data_ptr(), b["out"]
        return (lambda: t._call("qttt_tree_select_batch", tree, G, cap, t.seed, t.rollout_idx, K, t.board_offset, t.c_puct,
                                t.virtual_loss, paths, b["leaf"].state.data_ptr()),
                lambda: b["leaf"].evaluate(net, out=out),
                lambda: t._call("qttt_tree_backup_batch", tree, G, cap, K, paths, out["value"].data_ptr(), out["probs"].data_ptr()))

    us = {K: {"total": [], "parts": []} for K in Ks}
    for rep in range(reps + 1):
        for K in Ks:
            t = trees[K]
            t.reset(env)
            t.contemplate(warmup)
            rounds = max(1, rollouts // K)
            torch.cuda.synchronize()
            a, b = event(), event()
            a.record(stream)
            for _ in range(rounds):
                t._rollout() if K == 1 else t._round(K)
            b.record(stream)
            torch.cuda.synchronize()
            total = a.elapsed_time(b) * 1e3 / (rounds * K)
            fns = launches(t, K)
            ev = [[event() for _ in range(len(fns) + 1)] for _ in range(rounds)]
            for e in ev:
                e[0].record(stream)
                for i, fn in enumerate(fns):
                    fn()
                    e[i + 1].record(stream)
                t.rollout_idx += K
            torch.cuda.synchronize()
            parts = [sum(e[i].elapsed_time(e[i + 1]) for e in ev) * 1e3 / (rounds * K) for i in range(len(fns))]
            if rep:                              # the first repetition warms every leg up
                us[K]["total"].append(total)
                us[K]["parts"].append(parts)
    rows = []
    for K in Ks:
        xs = us[K]["total"]
        row = {"games": G, "mode": mode, "leg": "leaves", "leaves": K, "reps": reps, "rollouts_per_rep": max(1, rollouts // K) * K,
               "us_per_rollout_median": round(statistics.median(xs), 2), "us_per_rollout_min_max": [round(min(xs), 2), round(max(xs), 2)]}
        names = ("select", "fused") if K == 1 else ("select_batch", "evaluate", "backup_batch")
        for i, name in enumerate(names):
            row["us_%s_per_rollout_median" % name] = round(statistics.median(p[i] for p in us[K]["parts"]), 2)
        rows.append(row)
    base = next((r for r in rows if r["leaves"] == 1), None)
    for row in rows:
        if base is not None and row is not base:
            row["k1_us_per_rollout_median"] = base["us_per_rollout_median"]
            row["k1_spread_us"] = round(base["us_per_rollout_min_max"][1] - base["us_per_rollout_min_max"][0], 2)
            row["factor_over_k1"] = round(base["us_per_rollout_median"] / row["us_per_rollout_median"], 3)
    return rows


def run_explore(G, reps, launches, rollouts=8):
    """One JSON row: medians over `reps` interleaved repetitions of `launches` launches per leg."""
    import statistics
    from qtttgym_amd import SelfPlay
    from qtttgym_amd._host import out_rows
    env = VecEnv(G, seed=1)
    env.step_random_many(2)
    t = TreeSearch(G, capacity=1 + 2 * rollouts, num_simulations=2, seed=2)
    t.reset(env)
    t.contemplate(rollouts)                      # every root has priors and visits
    sp = SelfPlay(G, n_rollouts=rollouts, num_simulations=2)
    batch = sp.new_batch()
    root = out_rows(TreeSearch._ROOT_ROWS, G, t.device)
    noise = torch.empty((G, 36), dtype=torch.float64, device=t.device)
    applied = torch.empty(G, dtype=torch.uint8, device=t.device)
    rec = (t.tree.data_ptr(), G, t.capacity, 0, sp.n_rollouts, sp.alpha, sp.v_first, sp.v_second, batch.states.data_ptr(),
           batch.pi.data_ptr(), batch.mask.data_ptr(), batch.done.data_ptr(), batch.v.data_ptr(), batch.action36.data_ptr(),
           batch.length.data_ptr(), batch.winner.data_ptr(), batch.actions.data_ptr())
    stream = torch.cuda.current_stream()

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(launches):
            fn()
        b.record(stream)
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / launches

    legs = {"root_noise": lambda: t.add_root_noise(0.25, 0.3, noise=noise, applied=applied),      # mixes again each time
            "root_noise_alpha_2.5": lambda: t.add_root_noise(0.25, 2.5, noise=noise, applied=applied),
            "record_sampled": lambda: sp._call("qttt_selfplay_record_sampled", *rec, t.seed, t.board_offset, 1.0, 10),
            "record_sampled_temperature_0.5": lambda: sp._call("qttt_selfplay_record_sampled", *rec, t.seed,
                                                                t.board_offset, 0.5, 10),
            "record": lambda: sp._call("qttt_selfplay_record", *rec),
            "tree_root": lambda: t._root(**root)}
    us = {k: [] for k in legs}
    for rep in range(reps + 1):
        for k, fn in legs.items():
            x = timed(fn)
            if rep:
                us[k].append(x)
    row = {"games": G, "leg": "explore", "reps": reps, "launches_per_rep": launches, "applied": int(applied.sum())}
    for k, xs in us.items():
        row["us_%s_median" % k] = round(statistics.median(xs), 2)
        row["us_%s_min_max" % k] = [round(min(xs), 2), round(max(xs), 2)]
    return row


def run_compact(G, sims, R, reps, moves=4):
    """contemplate(R) + a move + sync + compact(), `moves` times per game from the empty board, `reps` games (the
    first one more as warm-up).  One JSON row: medians over every timed (game, move)."""
    import statistics
    from qtttgym_amd.actions import action36_to_pairs
    stream = torch.cuda.current_stream()
    t = TreeSearch(G, capacity=4 * R + 2, num_simulations=sims, seed=2)
    us_c, us_k, before, after = [], [], [], []
    for rep in range(reps + 1):
        env = VecEnv(G, seed=1 + rep)
        t.reset(env)
        for mv in range(moves):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            e[0].record(stream)
            t.contemplate(R)
            e[1].record(stream)
            env.step_raw(action36_to_pairs(t.choose()).contiguous())
            t.sync(env)
            b = t.nodes_used().float().mean()
            e[2].record(stream)
            t.compact(update_bound=False)
            e[3].record(stream)
            torch.cuda.synchronize()
            t.compact()                              # already compact: only the bound is read back
            if rep:
                us_c.append(e[0].elapsed_time(e[1]) * 1e3)
                us_k.append(e[2].elapsed_time(e[3]) * 1e3)
                before.append(float(b))
                after.append(float(t.nodes_used().float().mean()))
    return {"games": G, "mode": "uniform", "leg": "compact", "n_sims": sims, "rollouts": R, "moves": moves, "reps": reps,
            "us_contemplate_median": round(statistics.median(us_c), 1),
            "us_compact_median": round(statistics.median(us_k), 1),
            "us_compact_min": round(min(us_k), 1), "us_compact_max": round(max(us_k), 1),
            "us_compact_by_move": [round(statistics.median(us_k[m::moves]), 1) for m in range(moves)],
            "nodes_used_before_mean_by_move": [round(statistics.mean(before[m::moves]), 1) for m in range(moves)],
            "nodes_used_after_mean_by_move": [round(statistics.mean(after[m::moves]), 1) for m in range(moves)],
            "nodes_used_before_mean": round(statistics.mean(before), 1),
            "nodes_used_after_mean": round(statistics.mean(after), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", default="4096,65536,262144")
    ap.add_argument("--modes", default="uniform,f32,bf16")
    ap.add_argument("--sims", type=int, default=10)
    ap.add_argument("--rollouts", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--value-games", default="")
    ap.add_argument("--value-modes", default="f32,bf16")
    ap.add_argument("--value-reps", type=int, default=7)
    ap.add_argument("--leaves", default="", help="e.g. 1,8,32: the --value-games legs compare leaves per round")
    ap.add_argument("--compact-games", default="")
    ap.add_argument("--compact-rollouts", type=int, default=300)
    ap.add_argument("--compact-reps", type=int, default=3)
    ap.add_argument("--explore", action="store_true")
    ap.add_argument("--explore-games", default="4096,65536")
    ap.add_argument("--explore-reps", type=int, default=5)
    ap.add_argument("--explore-launches", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = []
    for G in [int(x) for x in args.games.split(",") if x]:
        for mode in args.modes.split(","):
            row = run(G, mode, args.sims, args.rollouts, args.warmup)
            print(json.dumps(row), flush=True)
            rows.append(row)
    for G in [int(x) for x in args.value_games.split(",") if x]:
        for mode in args.value_modes.split(","):
            Ks = [int(x) for x in args.leaves.split(",") if x]
            for row in (run_leaves(G, mode, Ks, args.value_reps) if Ks else [run_value(G, mode, args.sims, args.value_reps)]):
                print(json.dumps(row), flush=True)
                rows.append(row)
    for G in [int(x) for x in args.compact_games.split(",") if x]:
        row = run_compact(G, args.sims, args.compact_rollouts, args.compact_reps)
        print(json.dumps(row), flush=True)
        rows.append(row)
    for G in [int(x) for x in args.explore_games.split(",") if x and args.explore]:
        row = run_explore(G, args.explore_reps, args.explore_launches)
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
