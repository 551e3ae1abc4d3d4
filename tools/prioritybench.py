#!/usr/bin/env python3
"""Timing of prioritised replay (include/qttt_replay_priority.h) beside the uniform draw and beside what a
caller could compose from torch, not the judged line.  tools/replaybench.py's method: HIP events around CALLS back-to-back
calls of each route, one warm-up round, medians of nine rounds with min-max, the routes of a row interleaved in one
process; per call, Python included.  Prints one JSON object per row and writes them to profiles/priority/prioritybench.jsonl
(QTTT_PRIORITYBENCH_OUT names another directory).

  sample   n draws from a ring of 2^20 samples, n = 4 096 and 65 536: sync + the prioritised draw (ReplayBuffer.sample of a
           prioritised ring), the uniform ReplayBuffer.sample, and the composed torch route: torch.multinomial over the
           float priorities, then the same slots through the existing path (gather, transformed().encode(), scatter)
  update   ReplayBuffer.update_priorities of 4 096 draws
  step     one Trainer.step of 4 096 samples with and without weights
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
from qtttgym_amd import ReplayBuffer, Trainer, VecEnv, recommended_env, symmetry  # noqa: E402
from qtttgym_amd.policy_value import SHAPES  # noqa: E402
from replaybench import interleaved, stepped_batch  # noqa: E402
recommended_env(apply=True)


def main():
    dev = torch.device("cuda", torch.cuda.current_device())
    G, CAP = 65536, 1 << 20
    batch = stepped_batch(G, 1, dev)
    pr, un = ReplayBuffer(CAP, device=dev, seed=7, prioritized=True), ReplayBuffer(CAP, device=dev, seed=7)
    while un.size() < CAP:
        pr.add(batch)
        un.add(batch)
    pr.sample(4096)
    # priorities that differ: a write-back of random values over 2^18 draws
    gen = torch.Generator(device=dev).manual_seed(3)
    for _ in range(4):
        pr.sample(65536)
        pr.update_priorities(torch.rand(65536, device=dev, generator=gen) * 4 + 0.01)
    v = un.views()
    tau_all = torch.tensor(symmetry.ACTIONS, dtype=torch.int64, device=dev)
    shifts = torch.arange(36, device=dev)
    rows = []
    for N, calls in ((4096, 200), (65536, 40)):
        stride = (N + 63) // 64 * 64
        fprio = (pr.priority_views()["q"].to(torch.int64) & 0xFFFFFFFF).to(torch.float32)

        def composed():
            idx = torch.multinomial(fprio, N, replacement=True)
            k = torch.randint(0, 8, (N,), device=dev, dtype=torch.uint8)
            st = torch.zeros(2 * stride, dtype=torch.int64, device=dev)
            st[:N], st[stride:stride + N] = v["P"][idx], v["Q"][idx]
            s = VecEnv.from_state(st.view(torch.uint8), N).transformed(k).encode(with_mask=False)
            tau = tau_all[k.to(torch.int64)]
            pi = torch.zeros((N, 36), dtype=torch.float64, device=dev).scatter_(1, tau, v["pi"][idx])
            bits = (v["mask"][idx][:, None] >> shifts) & 1
            mask = torch.zeros_like(bits).scatter_(1, tau, bits).bool()
            return s, pi, mask, v["v"][idx], v["done"][idx] != 0

        (t_pr, t_un, t_co), spread = interleaved([lambda: pr.sample(N, "random"), lambda: un.sample(N, "random"), composed], calls)
        rows.append({"row": "sample", "n": N, "ring_samples": CAP, "us_sync_and_prioritized": t_pr, "us_uniform": t_un,
                     "us_composed_torch": t_co, "min_max_us_sync_and_prioritized": spread[0], "min_max_us_uniform": spread[1],
                     "min_max_us_composed_torch": spread[2], "sum_levels": pr.priority_levels,
                     "spreads_separate": {"prioritized_vs_uniform": spread[0][0] > spread[1][1] or spread[0][1] < spread[1][0],
                                          "prioritized_vs_composed": spread[0][0] > spread[2][1] or spread[0][1] < spread[2][0]},
                     "note": "the sync rebuilds every sum of the 2^20 priorities on each call; torch.multinomial draws from f32"})

    N = 4096
    pr.sample(N, "random")
    p = torch.rand(N, device=dev, generator=gen) + 0.01
    (t_up, t_sync), spread = interleaved([lambda: pr.update_priorities(p), pr.sync_priorities], 200)
    rows.append({"row": "update", "n": N, "ring_samples": CAP, "us_update_priorities": t_up, "us_sync_alone": t_sync,
                 "min_max_us_update_priorities": spread[0], "min_max_us_sync_alone": spread[1]})

    sgen = torch.Generator().manual_seed(11)
    sd = {k: torch.randn(shp, generator=sgen) * 0.05 for k, shp in SHAPES.items()}
    a, b = Trainer(sd, device=dev), Trainer(sd, device=dev)
    samples = un.sample(N, "random")
    w = torch.rand(N, device=dev, generator=gen) * 0.9 + 0.1
    (t_plain, t_w), spread = interleaved([lambda: a.step(*samples), lambda: b.step(*samples, weight=w)], 100)
    rows.append({"row": "step", "n": N, "us_step": t_plain, "us_step_weighted": t_w, "min_max_us_step": spread[0],
                 "min_max_us_step_weighted": spread[1],
                 "spreads_separate": spread[0][0] > spread[1][1] or spread[0][1] < spread[1][0]})

    path = os.environ.get("QTTT_PRIORITYBENCH_OUT", os.path.join(ROOT, "profiles", "priority"))
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "prioritybench.jsonl"), "w") as f:
        for r in rows:
            print(json.dumps(r), flush=True)
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
