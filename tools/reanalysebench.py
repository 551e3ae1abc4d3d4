#!/usr/bin/env python3
"""Timing of reanalysis (include/qttt_replay_reanalyse.h) beside what a caller had before it, not the
judged line.  HIP events around CALLS back-to-back calls of each formulation, one warm-up round, medians of REPS rounds
with min - max, the two formulations of a row interleaved in one process.  Prints one JSON object per row and writes
them to profiles/reanalyse/reanalysebench.jsonl (QTTT_REANALYSEBENCH_OUT names another directory).

  window   ReplayBuffer.gather(n) + ReplayBuffer.update(window, pi, v) of n = 4 096 and 65 536 samples on a ring of 2^20,
           beside the composed torch route: read `written` back, index views() by the slots, copy the words into a
           VecEnv, then the guarded index_copy_ of pi and v (the read-back is part of that route's cost)
  run      a whole Reanalyser.run() of 4 096 positions at 32 rollouts (a random network, value leaves), and the share of
           it that the two new launches take
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from qtttgym_amd import PolicyValueNet, Reanalyser, ReplayBuffer, SelfPlay, SelfPlayBatch, VecEnv, recommended_env  # noqa: E402
from qtttgym_amd.policy_value import SHAPES  # noqa: E402
recommended_env(apply=True)

REPS = 9
ROWS = 10


def interleaved(fns, calls):
    """Median microseconds per call of each of `fns`: rounds of `calls` back-to-back calls, run in turn REPS times after
    one warm-up round of each."""
    times = [[] for _ in fns]
    for rep in range(REPS + 1):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if rep:
                times[i].append(e0.elapsed_time(e1) * 1e3 / calls)
    return [statistics.median(t) for t in times], [(min(t), max(t)) for t in times]


def separate(a, b):
    """Whether two (min, max) spreads do not overlap."""
    return a[1] < b[0] or b[1] < a[0]


def stepped_batch(G, seed, dev):
    """A SelfPlayBatch of reachable states: G boards stepped at random, row t = the boards after t plies, random policy
    targets and lengths 1..10; done is 0, so that every sample of a window is refreshed."""
    gen = torch.Generator(device=dev).manual_seed(seed)
    env = VecEnv(G, device=dev, seed=seed)
    b = SelfPlayBatch(G, dev, env.state.numel())
    for t in range(ROWS):
        b.states[t].copy_(env.state)
        b.mask[t].copy_(env.encode()[1])
        env.step_random_many(1)
    b.pi.copy_(torch.rand(b.pi.shape, dtype=torch.float64, device=dev, generator=gen))
    b.v.copy_(torch.rand(b.v.shape, device=dev, generator=gen) * 2 - 1)
    b.length.copy_(torch.randint(1, ROWS + 1, (G,), device=dev, generator=gen).to(torch.uint8))
    return b


def main():
    dev = torch.device("cuda", torch.cuda.current_device())
    G, CAP = 65536, 1 << 20
    batch = stepped_batch(G, 1, dev)
    rb = ReplayBuffer(CAP, device=dev, seed=7)
    while rb.size() < CAP:                                      # fill the ring (three or four appends)
        rb.add(batch)
    views = rb.views()
    rows = []

    # ---- window: gather + update beside the composed torch route
    for n in (4096, 65536):
        gen = torch.Generator(device=dev).manual_seed(n)
        pi = torch.rand((n, 36), dtype=torch.float64, device=dev, generator=gen)
        v = torch.rand(n, device=dev, generator=gen)
        env = VecEnv(n, device=dev)
        stride = (n + 63) // 64 * 64
        start = CAP - n // 2                                    # a window that crosses the wrap

        def native():
            rb.update(rb.gather(n, start, env=env), pi=pi, v=v)

        def composed():
            written = int(views["written"].item())              # the read-back the guard needs
            F = min(written, CAP)
            slot = (start % F + torch.arange(n, device=dev)) % F
            number = written - 1 - (written - 1 - slot) % CAP
            st = env.state.view(torch.int64)
            st[:n], st[stride:stride + n] = views["P"][slot], views["Q"][slot]
            # ... the search would run here, and appends may have moved `written` on: read it again
            written = int(views["written"].item())
            ok = (written - 1 - (written - 1 - slot) % CAP == number) & (views["done"][slot] == 0)
            to = slot[ok]
            views["pi"].index_copy_(0, to, pi[ok])
            views["v"].index_copy_(0, to, v[ok])
            return ok

        before = rb.buffer.clone()
        native()
        after_native = rb.buffer.clone()
        rb.buffer.copy_(before)
        composed()
        assert torch.equal(rb.buffer, after_native)
        (t_new, t_old), spread = interleaved([native, composed], 200 if n == 4096 else 50)
        moved = n * (16 + 16 + 4 + 8 + 4 + 1) + n * (4 + 8 + 1 + 288 + 288 + 4 + 4 + 1)
        rows.append({"row": "window", "n": n, "ring_samples": CAP, "us_gather_update": t_new, "us_composed_torch": t_old,
                     "min_max_us_gather_update": spread[0], "min_max_us_composed_torch": spread[1],
                     "spreads_separate": separate(*spread), "bytes_moved": moved, "GBps": moved / t_new / 1e3, "launches": 2,
                     "note": "per call, Python and allocation included; the composed route reads `written` back twice"})

    # ---- run: a whole Reanalyser.run() and the share of the two launches
    n, R = 4096, 32
    gen = torch.Generator().manual_seed(3)
    net = PolicyValueNet({k: torch.randn(shp, generator=gen) * 0.05 for k, shp in SHAPES.items()}, device=dev)
    sp = SelfPlay(n, n_rollouts=R, net=net, leaf_eval="value", value_targets=(1.0, -1.0), device=dev)
    ra = Reanalyser(sp, rb, n)
    pi = torch.rand((n, 36), dtype=torch.float64, device=dev)

    def two_launches():
        rb.update(rb.gather(n, None, env=ra.env), pi=pi)

    (t_run, t_two), spread = interleaved([ra.run, two_launches], 5)
    rows.append({"row": "run", "n": n, "rollouts": R, "us_run": t_run, "us_gather_update": t_two, "min_max_us_run": spread[0],
                 "min_max_us_gather_update": spread[1], "share_of_run": t_two / t_run,
                 "note": "leaf_eval=value, leaves=1, a random f32 network; the rest of a run is reset, contemplate and record"})

    path = os.environ.get("QTTT_REANALYSEBENCH_OUT", os.path.join(ROOT, "profiles", "reanalyse"))
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "reanalysebench.jsonl"), "w") as f:
        for r in rows:
            print(json.dumps(r), flush=True)
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
