#!/usr/bin/env python3
"""One training step of the policy/value network, two routes on the same minibatch, interleaved in one process:

  fused   qtttgym_amd.Trainer.step: six HIP launches on the packed weights the search reads
  torch   the step of examples/selfplay_train.py without --device-train: loss_terms + backward + Adam(amsgrad).step +
          PolicyValueNet.load_state_dict (the repack the search needs before it can use the new weights)

    python tools/trainbench.py [--sizes 1024,4096,65536] [--reps 9] [--warmup 3] [--out profiles/train/trainbench.jsonl]

Device events around each step after warm-up; the two routes alternate, and the medians of the repetitions are reported
with each route's min-max spread.  One JSON line per size, appended to --out.  The torch route's boolean indexing waits
for the host inside the timed region, as it does in the example."""
import argparse
import importlib.util
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from qtttgym_amd import PolicyValueNet, Trainer, recommended_env  # noqa: E402
recommended_env(apply=True)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from nn_reference64 import random_play_env  # noqa: E402


def example_module():
    spec = importlib.util.spec_from_file_location("selfplay_train", os.path.join(ROOT, "examples", "selfplay_train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def batch(n, dev, net):
    env = random_play_env(n, 7, str(dev))
    s = env.encode(with_mask=False)
    mask = ~torch.isneginf(env.evaluate(net, rows=("logits",))["logits"])
    gen = torch.Generator(device=dev).manual_seed(n)
    pi = torch.rand((n, 36), generator=gen, dtype=torch.float64, device=dev) * mask
    pi = pi / pi.sum(1, keepdim=True).clamp_min(1e-300)
    v = torch.randint(-1, 2, (n,), generator=gen, device=dev).float()
    done = ~mask.any(1) | (torch.rand(n, generator=gen, device=dev) < 0.2)
    return s, pi, mask, v, done


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3                                       # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096,65536")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train", "trainbench.jsonl"))
    args = ap.parse_args()
    if args.reps < 7:
        ap.error("--reps >= 7: the medians are of at least seven alternating repetitions")
    ex = example_module()
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(0)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for n in (int(x) for x in args.sizes.split(",")):
        model = ex.Net().to(dev)
        optim = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-3, amsgrad=True)
        net_torch, net_fused = PolicyValueNet(model, device=dev), PolicyValueNet(model, device=dev)
        trainer = Trainer(model, device=dev, net=net_fused)
        samples = batch(n, dev, net_torch)

        def torch_step():
            ex.train(model, optim, (samples,))
            net_torch.load_state_dict(model)

        def fused_step():
            trainer.step(*samples)

        for _ in range(args.warmup):
            torch_step()
            fused_step()
        torch.cuda.synchronize()
        t_torch, t_fused = [], []
        for _ in range(args.reps):
            t_torch.append(timed(torch_step))
            t_fused.append(timed(fused_step))
        line = {"tool": "trainbench", "device": torch.cuda.get_device_name(dev), "samples": n, "reps": args.reps,
                "warmup": args.warmup,
                "fused_us_median": round(statistics.median(t_fused), 1), "fused_us_min": round(min(t_fused), 1),
                "fused_us_max": round(max(t_fused), 1),
                "torch_us_median": round(statistics.median(t_torch), 1), "torch_us_min": round(min(t_torch), 1),
                "torch_us_max": round(max(t_torch), 1),
                "speedup_of_medians": round(statistics.median(t_torch) / statistics.median(t_fused), 2)}
        print(json.dumps(line), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
