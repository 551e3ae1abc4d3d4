#!/usr/bin/env python3
"""Timing of the replay ring (include/qttt_replay.h) beside what a caller had before it, not the judged
line.  HIP events around CALLS back-to-back calls of each formulation, one warm-up round, medians of REPS rounds, the two
formulations of a row interleaved in one process.  Prints one JSON object per row and writes them to
profiles/replay/replaybench.jsonl (QTTT_REPLAYBENCH_OUT names another directory).

  sample   ReplayBuffer.sample(4096, "random") from a ring of 2^20 samples, beside the composed route: gather the drawn
           slots, VecEnv.transformed(sym).encode(), torch scatter of pi / mask by tau (given the same slots and symmetries)
  add      ReplayBuffer.add() of a 65 536-game batch, beside SelfPlayBatch.flat(), which is what made trainer-shaped
           samples before (it encodes every row and synchronises with the host; add() stores packed states and does not)
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from qtttgym_amd import ReplayBuffer, SelfPlayBatch, VecEnv, recommended_env, symmetry  # noqa: E402
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


def stepped_batch(G, seed, dev):
    """A SelfPlayBatch of reachable states: G boards stepped at random, row t = the boards after t plies, random targets
    and lengths 1..10."""
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
    G, CAP, N = 65536, 1 << 20, 4096
    batch = stepped_batch(G, 1, dev)
    samples = int(batch.length.sum())
    rb = ReplayBuffer(CAP, device=dev, seed=7)
    while rb.size() < CAP:                                      # fill the ring (three or four appends)
        rb.add(batch)
    rows = []

    # ---- sample
    out = rb.sample(N, "random")
    v = rb.views()
    tau_all = torch.tensor(symmetry.ACTIONS, dtype=torch.int64, device=dev)
    shifts = torch.arange(36, device=dev)
    stride = (N + 63) // 64 * 64

    def composed():
        idx, k = rb.last_index.to(torch.int64), rb.last_symmetry
        st = torch.zeros(2 * stride, dtype=torch.int64, device=dev)
        st[:N], st[stride:stride + N] = v["P"][idx], v["Q"][idx]
        s = VecEnv.from_state(st.view(torch.uint8), N).transformed(k).encode(with_mask=False)
        tau = tau_all[k.to(torch.int64)]
        pi = torch.zeros((N, 36), dtype=torch.float64, device=dev).scatter_(1, tau, v["pi"][idx])
        bits = (v["mask"][idx][:, None] >> shifts) & 1
        mask = torch.zeros_like(bits).scatter_(1, tau, bits).bool()
        return s, pi, mask, v["v"][idx], v["done"][idx] != 0

    ref = composed()
    assert all(torch.equal(a.view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8)) for a, b in zip(out, ref))
    (t_new, t_into, t_old), spread = interleaved([lambda: rb.sample(N, "random"), lambda: rb.sample(N, "random", out=out), composed], 400)
    moved = N * (16 + 288 + 8 + 4 + 1) + N * (720 + 288 + 36 + 4 + 1 + 4 + 1)
    rows.append({"row": "sample", "n": N, "ring_samples": CAP, "symmetries": "random", "us": t_new, "us_out_given": t_into,
                 "us_composed_torch": t_old, "min_max_us": spread[0], "min_max_us_out_given": spread[1],
                 "min_max_us_composed_torch": spread[2], "bytes_moved": moved, "GBps": moved / t_new / 1e3,
                 "note": "the composed route is handed the slots and symmetries; sample() also allocates its outputs unless out= is given"})

    # ---- add
    def by_flat():
        return batch.flat()

    (t_add, t_flat), spread = interleaved([lambda: rb.add(batch), by_flat], 50)
    moved = samples * ((16 + 288 + 36 + 4 + 1) + (16 + 288 + 8 + 4 + 1))        # read with the mask as 36 bytes, stored as a word
    rows.append({"row": "add", "games": G, "samples": samples, "us": t_add, "us_flat": t_flat, "min_max_us": spread[0],
                 "min_max_us_flat": spread[1], "bytes_moved": moved, "GBps": moved / t_add / 1e3,
                 "launches": 3, "note": "flat() encodes all 10 x G rows, gathers five tensors and reads length back"})

    path = os.environ.get("QTTT_REPLAYBENCH_OUT", os.path.join(ROOT, "profiles", "replay"))
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "replaybench.jsonl"), "w") as f:
        for r in rows:
            print(json.dumps(r), flush=True)
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
