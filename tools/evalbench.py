#!/usr/bin/env python3
"""Microseconds per policy/value evaluation of N boards (VecEnv.evaluate: one kernel) against the torch route a user has
without it (VecEnv.encode() + an F.linear chain + masked_fill), same dtype, same process, alternating, timed with device
events after warm-up.  Both produce value f32[N] and masked logits [N,36].  Prints one JSON line per (dtype, N) with the
median µs of each route, the kernel's FLOP/s (373 248 FLOP per board, the dense count) and its share of the MFMA peak of
the dtype, and — first — the largest deviation of each dtype from the reference outputs in tests/golden/model_eval.npz.

    python tools/evalbench.py [--sizes 4096,65536,1048576] [--reps 7] [--calls 20] [--out FILE]

Kernel time alone: run it with --no-torch under `rocprofv3 --kernel-trace --stats` (a separate run).
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from qtttgym_amd import recommended_env  # noqa: E402
recommended_env(apply=True)
from qtttgym_amd import PolicyValueNet, VecEnv  # noqa: E402
from nn_reference64 import golden_state_dict, load_golden  # noqa: E402

FLOP_PER_BOARD = 2 * (180 * 256 + 2 * 256 * 256 + 256 * 37)            # 373 248
PEAK = {"f32": 157.3e12, "bf16": 2.5e15}                                # MI355X MFMA peaks (f32 = vector rate)
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}


def parity(g, sd, dev):
    env = VecEnv(len(g["value"]), device=dev)
    env.import_boards(g["moves"], g["n_moves"], g["board"], g["qmask"].astype("int16"), g["n_q"])
    res = {}
    for name, dt in DTYPES.items():
        out = env.evaluate(PolicyValueNet(sd, device=dev, dtype=dt), rows=("value", "logits", "probs"))
        rv, rl, rp = (torch.from_numpy(g[k]).to(dev).double() for k in ("value", "logits", "probs"))
        fin, ok = torch.isfinite(rl), ~torch.isnan(rp)
        res[name] = {"max_abs_dvalue": (out["value"].double() - rv).abs().max().item(),
                     "max_abs_dlogit": (out["logits"].double()[fin] - rl[fin]).abs().max().item(),
                     "max_abs_dprob": (out["probs"].double()[ok] - rp[ok]).abs().max().item(),
                     "mask_identical": bool(torch.equal(torch.isneginf(out["logits"]), torch.isneginf(rl))),
                     "nan_rows_identical": bool(torch.equal(torch.isnan(out["probs"]), torch.isnan(rp)))}
    return res


def torch_route(env, W, vec_mask):
    vec, mask = env.encode(out=vec_mask)
    x = vec.view(env.num_envs, 180).to(W["dtype"])
    for i in (0, 2, 4):
        x = F.relu(F.linear(x, W["fc.%d.weight" % i], W["fc.%d.bias" % i]))
    v = F.linear(x, W["V_head.1.weight"], W["V_head.1.bias"])
    lg = F.linear(x, W["pi_head.1.weight"], W["pi_head.1.bias"]).masked_fill(~mask, -float("inf"))
    return v, lg


def timed(fn, calls):
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
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true", help="the fused kernel only (for a kernel trace)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("evalbench needs an MI355X")
    dev = torch.device("cuda", 0)
    g = load_golden()
    sd = golden_state_dict(g)
    lines = [{"parity_vs_reference": parity(g, sd, dev), "positions": int(len(g["value"]))}]
    print(json.dumps(lines[0]), flush=True)
    for name in args.dtypes.split(","):
        dt = DTYPES[name]
        net = PolicyValueNet(sd, device=dev, dtype=dt)
        W = {k: t.to(dev, dt) for k, t in sd.items()}
        W["dtype"] = dt
        for n in (int(s) for s in args.sizes.split(",")):
            env = VecEnv(n, device=dev, seed=11, auto_reset=True)
            env.step_random_many(5)
            out = env.evaluate(net)
            vm = env.encode()
            fused, route = [], []
            for _ in range(args.warmup):
                env.evaluate(net, out=out)
                if not args.no_torch:
                    torch_route(env, W, vm)
            torch.cuda.synchronize()
            for _ in range(args.reps):                  # alternate the two routes
                fused.append(timed(lambda: env.evaluate(net, out=out), args.calls))
                if not args.no_torch:
                    route.append(timed(lambda: torch_route(env, W, vm), args.calls))
            us = statistics.median(fused)
            rec = {"dtype": name, "boards": n, "fused_us": round(us, 2), "fused_us_min": round(min(fused), 2),
                   "flops": FLOP_PER_BOARD * n / (us * 1e-6), "share_of_mfma_peak": FLOP_PER_BOARD * n / (us * 1e-6) / PEAK[name]}
            if route:
                rec.update({"torch_route_us": round(statistics.median(route), 2), "torch_route_us_min": round(min(route), 2),
                            "speedup": round(statistics.median(route) / us, 2)})
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            del env, out, vm
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
