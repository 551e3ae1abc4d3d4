#!/usr/bin/env python3
"""Timing of the symmetry kernels (include/qttt_symmetry.h) beside what a caller had before them, not
the judged line.  HIP events around each call, one warm-up, medians of five, the two formulations of a row interleaved
in one process.  Prints one JSON object per row and writes them to profiles/symmetry/symbench.json.

  transform   qttt_transform at 65 536 and 1 048 576 boards, beside export -> torch permutation -> import (which gives
              the permuted qstructs order, not the mirrored game's)
  augment     qttt_selfplay_augment at G = 1 024 and 65 536 with K = 8, beside the torch restatement of the tests
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from qtttgym_amd import SelfPlay, VecEnv, recommended_env, symmetry  # noqa: E402
recommended_env(apply=True)

REPS = 5


def interleaved(fns):
    """Median milliseconds of each of `fns`, run in turn REPS times after one warm-up of each."""
    times = [[] for _ in fns]
    for rep in range(REPS + 1):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if rep:
                times[i].append(e0.elapsed_time(e1))
    return [statistics.median(t) for t in times]


def transform_rows():
    rows = []
    for n in (65536, 1 << 20):
        env = VecEnv(n, seed=1)
        env.step_random_many(5)
        ks = (torch.arange(n, device=env.device) % 8).to(torch.uint8)
        out, imp = env._like(), env._like()
        cells, _ = symmetry.device_tables(env.device)
        sig = cells.to(torch.int64)[ks.to(torch.int64)]                              # [n, 9]
        inv = torch.argsort(sig, 1)
        bits = torch.arange(9, device=env.device)
        ex = env.export_boards()

        def by_torch():
            env.export_boards(out=ex)
            board = torch.gather(ex["board"], 1, inv)
            mv = ex["moves"].to(torch.int64)
            mapped = torch.where(mv < 9, torch.gather(sig, 1, mv.clamp(max=8).flatten(1)).view_as(mv), mv)
            moves = mapped.sort(-1).values.to(torch.uint8)
            q = ((ex["qmask"].to(torch.int64)[:, :, None] >> bits) & 1)               # [n, 4, 9]
            qmask = (q << sig[:, None, :]).sum(-1).to(torch.int16)
            imp.import_boards(moves, ex["n_moves"], board, qmask, ex["n_q"])

        t_new, t_old = interleaved([lambda: env.transformed(ks, out=out), by_torch])
        rows.append({"row": "transform", "boards": n, "us": t_new * 1e3, "us_export_torch_import": t_old * 1e3,
                     "bytes_moved": 33 * n, "GBps": 33 * n / (t_new * 1e-3) / 1e9})
    return rows


def augment_rows():
    rows = []
    for G in (1024, 65536):
        batch = SelfPlay(G, n_rollouts=2, num_simulations=1, seed=3).play()
        samples = int(batch.length.sum())
        live = torch.arange(10, device=batch.device)[:, None] < batch.length.to(torch.int64)[None, :]
        taus = [torch.tensor(symmetry.ACTIONS[k], device=batch.device) for k in range(8)]

        def by_torch():
            out = {"pi": [], "mask": [], "action36": [], "states": []}
            for k in range(8):
                pi, mask = torch.zeros_like(batch.pi), torch.zeros_like(batch.mask)
                pi[:, :, taus[k]] = batch.pi
                mask[:, :, taus[k]] = batch.mask
                out["pi"].append(pi)
                out["mask"].append(mask)
                out["action36"].append(torch.where(live, symmetry.transform_action36(batch.action36, k),
                                                   torch.zeros_like(batch.action36)))
                out["states"].append([batch.row_env(t).transformed(k).state for t in range(10)])
            return [torch.cat(out[f], 1) for f in ("pi", "mask", "action36")] + [batch.done.repeat(1, 8), batch.v.repeat(1, 8)]

        t_new, t_old = interleaved([lambda: batch.augment(), by_torch])
        written = 346 * 8 * samples
        rows.append({"row": "augment", "games": G, "K": 8, "samples_in": samples, "us": t_new * 1e3, "us_torch": t_old * 1e3,
                     "bytes_written": written, "GBps_written": written / (t_new * 1e-3) / 1e9,
                     "note": "both sides include the allocation and zero fill of their outputs"})
    return rows


def main():
    rows = transform_rows() + augment_rows()
    for r in rows:
        print(json.dumps(r), flush=True)
    path = os.path.join(ROOT, "profiles", "symmetry")
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(os.environ.get("QTTT_SYMBENCH_OUT", path), "symbench.json"), "w") as f:
        json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
