#!/usr/bin/env python3
"""Microseconds per policy/value evaluation of N boards (VecEnv.evaluate: one kernel) against the torch route a user has
without it (VecEnv.encode() + an F.linear chain + masked_fill), same dtype, same process, alternating, timed with device
events after warm-up.  Both produce value f32[N] and masked logits [N,36].  Prints one JSON line per (dtype, N) with the
median µs of each route, the kernel's FLOP/s (373 248 FLOP per board, the dense count) and its share of the MFMA peak of
the dtype, and — first — the largest deviation of each dtype from the reference outputs in tests/golden/model_eval.npz.

    python tools/evalbench.py [--sizes 4096,65536,1048576] [--reps 7] [--calls 20] [--out FILE]

Kernel time alone: run it with --no-torch under `rocprofv3 --kernel-trace --stats` (a separate run).

--symmetries: the evaluation averaged over the eight images of every board instead: the fused call
(VecEnv.evaluate(symmetries="all"), one kernel), the composed route a caller had without it (eight transformed(k), eight
evaluate, a gather through tau_k each and the pairwise sum, every buffer allocated beforehand) and plain evaluate at the same
board count, alternating in one process with the same repetition scheme, rows value and probs (what the search reads).
One JSON line per (dtype, N): the medians, the composed route's spread over its repetitions (max - min), and the ratios.

    python tools/evalbench.py --symmetries [--sizes 4096,65536,1048576] [--out profiles/nn_symmetric/evalbench_symmetries.jsonl]
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


class ComposedSymmetric:
    """The composed route over the eight symmetries, with every buffer of its own: images, their rows, the result."""

    def __init__(self, env, net, rows):
        from qtttgym_amd import symmetry
        self.env, self.net = env, net
        self.images = [VecEnv(env.num_envs, device=env.device) for _ in range(8)]
        self.outs = [env.evaluate(net, rows=rows) for _ in range(8)]
        self.tau = torch.tensor(symmetry.tables()[1], dtype=torch.int64, device=env.device)

    def __call__(self):
        terms = []
        for k in range(8):
            out = self.env.transformed(k, out=self.images[k]).evaluate(self.net, out=self.outs[k])
            terms.append({r: (t if t.dim() == 1 else t[:, self.tau[k]]) for r, t in out.items()})
        while len(terms) > 1:
            terms = [{r: a[r] + b[r] for r in a} for a, b in zip(terms[0::2], terms[1::2])]
        return {r: t * 0.125 for r, t in terms[0].items()}


def symmetries_mode(args, dev, sd):
    rows, lines = ("value", "probs"), []
    for name in args.dtypes.split(","):
        net = PolicyValueNet(sd, device=dev, dtype=DTYPES[name])
        for n in (int(s) for s in args.sizes.split(",")):
            env = VecEnv(n, device=dev, seed=11, auto_reset=True)
            env.step_random_many(5)
            out, plain_out = env.evaluate(net, rows=rows, symmetries="all"), env.evaluate(net, rows=rows)
            composed = ComposedSymmetric(env, net, rows)
            routes = {"fused": lambda: env.evaluate(net, out=out, symmetries="all"), "composed": composed,
                      "plain": lambda: env.evaluate(net, out=plain_out)}
            for _ in range(args.warmup):
                for fn in routes.values():
                    fn()
            torch.cuda.synchronize()
            want = composed()
            agree = all(bool(((out[r] == want[r]) | (torch.isnan(out[r]) & torch.isnan(want[r]))).all()) for r in rows)
            us = {k: [] for k in routes}
            for _ in range(args.reps):                  # alternate the three routes
                for k, fn in routes.items():
                    us[k].append(timed(fn, args.calls))
            med = {k: statistics.median(v) for k, v in us.items()}
            rec = {"mode": "symmetries", "dtype": name, "boards": n, "n_sym": 8, "rows": list(rows),
                   "fused_equals_composed": agree,
                   "fused_us": round(med["fused"], 2), "fused_us_min": round(min(us["fused"]), 2),
                   "fused_us_max": round(max(us["fused"]), 2),
                   "composed_us": round(med["composed"], 2), "composed_us_min": round(min(us["composed"]), 2),
                   "composed_us_max": round(max(us["composed"]), 2),
                   "composed_spread_us": round(max(us["composed"]) - min(us["composed"]), 2),
                   "plain_us": round(med["plain"], 2), "plain_us_min": round(min(us["plain"]), 2),
                   "composed_over_fused": round(med["composed"] / med["fused"], 2),
                   "fused_over_plain": round(med["fused"] / med["plain"], 2),
                   "share_of_mfma_peak": 8 * FLOP_PER_BOARD * n / (med["fused"] * 1e-6) / PEAK[name]}
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            del env, out, plain_out, composed, routes, want
            torch.cuda.empty_cache()
    return lines


def write_lines(path, lines):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        for r in lines:
            f.write(json.dumps(r) + "\n")


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
    ap.add_argument("--symmetries", action="store_true",
                    help="time evaluate(symmetries='all') beside the composed route and plain evaluate instead")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("evalbench needs an MI355X")
    dev = torch.device("cuda", 0)
    g = load_golden()
    sd = golden_state_dict(g)
    if args.symmetries:
        lines = symmetries_mode(args, dev, sd)
        if args.out:
            write_lines(args.out, lines)
        return
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
        write_lines(args.out, lines)


if __name__ == "__main__":
    main()
