#!/usr/bin/env python3
"""Network-guided playouts, one per lane: the fused VecEnv.rollout_policy (ONE kernel) against the composed route a user
has without it — up to 9 x (VecEnv.evaluate(rows=("probs",)), inverse-CDF sampling in torch on the same u, step_raw(actions,
bits)), finished lanes frozen (node_info per ply) — same draws, same dtype, same process, alternating, timed with device
events after warm-up (median of --reps).  One JSON line per (dtype, lanes) with both times, the plies played per lane,
the plies computed per tile (a tile runs until its last lane finishes: the difference is the rows the tile loop wastes),
the kernel's FLOP/s counting 373 248 FLOP per COMPUTED lane-ply and its share of the dtype's MFMA peak,
and how often the two routes end in the same result (they differ only where f32 rounding moves u across a CDF boundary).

    python tools/policy_rollout_bench.py [--sizes 4096,65536,1048576] [--dtypes f32,bf16] [--reps 7] [--out FILE]

Kernel time alone: run it with --fused-only under `rocprofv3 --kernel-trace --stats` (a separate run).
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from qtttgym_amd import recommended_env  # noqa: E402
recommended_env(apply=True)
from qtttgym_amd import PolicyValueNet, VecEnv  # noqa: E402
from qtttgym_amd.actions import action36_to_pairs  # noqa: E402
from nn_reference64 import golden_state_dict, load_golden  # noqa: E402

FLOP_PER_LANE_PLY = 2 * (180 * 256 + 2 * 256 * 256 + 256 * 37)        # 373 248
PEAK = {"f32": 157.3e12, "bf16": 2.5e15}                                # MI355X MFMA peaks (f32 = vector rate)
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
TILE = {"f32": 64, "bf16": 128}
M64 = (1 << 64) - 1


def _splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def _lowbias32(x):
    with np.errstate(over="ignore"):
        x = x ^ (x >> np.uint32(16))
        x = x * np.uint32(0x7FEB352D)
        x = x ^ (x >> np.uint32(15))
        x = x * np.uint32(0x846CA68B)
        return x ^ (x >> np.uint32(16))


def draws(seed, n, step_idx0, dev):
    """(u f32[9, n], bits u8[9, n]) of qttt_hash(seed, i, step_idx0 + p) for boards i < 2^32 (include/qttt_policy_rollout.h)."""
    ids = np.arange(n, dtype=np.uint32)
    us, bits = [], []
    for p in range(9):
        key = _splitmix64(seed ^ (((step_idx0 + p) * 0xD1B54A32D192ED03) & M64))
        h1 = _lowbias32(ids ^ np.uint32(key & 0xFFFFFFFF))
        h2 = _lowbias32(h1 ^ np.uint32(key >> 32))
        us.append((h2 >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24))
        bits.append((h1 >> np.uint32(31)).astype(np.uint8))
    return torch.from_numpy(np.stack(us)).to(dev), torch.from_numpy(np.stack(bits)).to(dev)


class Composed:
    """The route without the fused kernel, on a work copy of the boards (the leaves are not changed)."""

    def __init__(self, env, net, u, bits):
        self.env, self.net, self.u, self.bits = env, net, u, bits
        self.work = VecEnv.from_state(env.state.clone(), env.num_envs, seed=env.seed)
        self.ev = self.work.evaluate(net, rows=("probs",))
        self.info = self.work.node_info(python_key=False)
        self.info.pop("state_key")

    def __call__(self):
        w = self.work
        w.state.copy_(self.env.state)
        for p in range(9):
            info = w.node_info(out=self.info)
            live = (~info["terminal"]) & (info["legal"] != 0)
            pr = torch.nan_to_num(w.evaluate(self.net, out=self.ev)["probs"], nan=0.0)
            cdf = pr.cumsum(1)
            a = (cdf <= (self.u[p] * cdf[:, -1])[:, None]).sum(1)
            last = 35 - (pr > 0).flip(1).to(torch.int8).argmax(1)
            a = torch.minimum(a, last)
            pairs = action36_to_pairs(a.to(torch.uint8))
            pairs = torch.where(live[:, None], pairs, torch.full_like(pairs, 255))
            w.step_raw(pairs.contiguous(), self.bits[p])
        return w


def timed(fn, calls=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,65536,1048576")
    ap.add_argument("--dtypes", default="f32,bf16")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--fused-only", action="store_true", help="the fused kernel only (for a kernel trace)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("policy_rollout_bench needs an MI355X")
    dev = torch.device("cuda", 0)
    sd = golden_state_dict(load_golden())
    lines = []
    for name in args.dtypes.split(","):
        net = PolicyValueNet(sd, device=dev, dtype=DTYPES[name])
        for n in (int(s) for s in args.sizes.split(",")):
            env = VecEnv(n, device=dev, seed=11, auto_reset=True)
            env.step_random_many(3)                          # leaves at mixed depths, a few of them finished
            env = VecEnv.from_state(env.state.clone(), n, seed=5)
            t0 = 0
            out = env.rollout_policy(net, step_idx0=t0, with_plies=True)
            comp = None if args.fused_only else Composed(env, net, *draws(env.seed, n, t0, dev))
            for _ in range(args.warmup):
                env.rollout_policy(net, step_idx0=t0, out=out)
                if comp:
                    comp()
            torch.cuda.synchronize()
            fused, route = [], []
            for _ in range(args.reps):                       # alternate the two routes
                fused.append(timed(lambda: env.rollout_policy(net, step_idx0=t0, out=out)))
                if comp:
                    route.append(timed(comp))
            us = statistics.median(fused)
            plies = out["plies"][:, 0].to(torch.int64)
            M = TILE[name]
            pad = (-n) % M
            per_tile = torch.cat([plies, plies.new_zeros(pad)]).view(-1, M).max(1).values
            computed = int(per_tile.sum()) * M                # lane-plies the tiles ran
            played = int(plies.sum())
            rec = {"dtype": name, "lanes": n, "fused_us": round(us, 2), "fused_us_min": round(min(fused), 2),
                   "plies_played_per_lane": round(played / n, 3), "plies_computed_per_tile": round(float(per_tile.float().mean()), 3),
                   "wasted_row_fraction": round(1 - played / max(computed, 1), 4),
                   "flops_computed": FLOP_PER_LANE_PLY * computed / (us * 1e-6),
                   "share_of_mfma_peak": FLOP_PER_LANE_PLY * computed / (us * 1e-6) / PEAK[name]}
            if comp:
                w = comp()
                win = w.node_info(python_key=False)["winner"].to(torch.int64)
                res = torch.where(win < 0, 0, torch.where(win > 0, 1, -1))
                rec.update({"composed_us": round(statistics.median(route), 2), "composed_us_min": round(min(route), 2),
                            "speedup": round(statistics.median(route) / us, 2),
                            "same_result_fraction": round(float((res == out["result"][:, 0]).float().mean()), 5)})
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            del env, out, comp
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
