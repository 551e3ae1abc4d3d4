#!/usr/bin/env python3
"""Generates tests/golden/policy_playout_stats.npz from the UNMODIFIED reference's AlphaZero._simulate (alphazero.py:192-205)
on its trained weights (`model.pt`), loaded through ref_shim.py.  Build container only; the .npz is data.

Positions: 32 non-terminal positions of model_eval.npz, 8 from each band of moves played (0-2, 3-4, 5-6, 7-8), the band's
positions with the most pending quantum moves first (the collapse-heavy ones).  For each, N_SIMS calls of
AlphaZero._simulate on a fresh leaf built from the Board attributes (turn, winner and terminal as AlphaZero.reset derives
them): every ply runs Model.forward, samples from Categorical(logits) and picks a collapse child with np.random.choice,
with the reference's own random sources (qeval.py's `random` module included, seeded).  Records the frequencies of
_reward = +1 / -1 / 0.  The GPU test compares VecEnv.rollout_policy's frequencies with these.

Takes about two minutes on one CPU core (32 x 1 000 simulations).
"""
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from ref_shim import load_reference, REFERENCE_ROOT  # noqa: E402

N_SIMS = 1000
PER_BAND = 8
BANDS = ((0, 2), (3, 4), (5, 6), (7, 8))


def main():
    qtttgym, _ = load_reference()
    qtttgym.qeval.random = random                # the reference's own collapse source, not the shim's pinned bit
    sys.path.insert(0, REFERENCE_ROOT)
    import torch
    import alphazero as ref_az                   # the reference's alphazero.py / nn.py, unmodified
    torch.set_num_threads(1)
    random.seed(2024)
    np.random.seed(2024)
    torch.manual_seed(2024)
    az = ref_az.AlphaZero(rollouts=1, num_simulations=1, filepath=os.path.join(REFERENCE_ROOT, "model.pt"))
    GS = ref_az.AlphaZero.GameState

    g = np.load(os.path.join(HERE, "model_eval.npz"))
    nm, nq = g["n_moves"].astype(int), g["n_q"].astype(int)
    alive = ~np.isneginf(g["logits"]).all(1)

    def leaf(i):
        gs = GS([int(x) for x in g["board"][i]], [(int(m[0]), int(m[1]), t) for t, m in enumerate(g["moves"][i][:nm[i]])],
                int(nm[i]) % 2 == 0, None, False)
        gs.qstructs = [{v for v in range(9) if int(g["qmask"][i][k]) >> v & 1} for k in range(int(nq[i]))]
        gs.update_winner()
        return gs

    picked = []
    for lo, hi in BANDS:
        cand = [i for i in range(len(nm)) if lo <= nm[i] <= hi and alive[i] and not leaf(i).terminal]
        cand.sort(key=lambda i: (-(int(nm[i]) - int((g["board"][i] >= 0).sum())), i))   # pending quantum moves first
        picked += cand[:PER_BAND]
    counts = np.zeros((len(picked), 3), dtype=np.int32)              # +1, -1, 0
    for r, i in enumerate(picked):
        node = leaf(i)
        for _ in range(N_SIMS):
            counts[r, {1: 0, -1: 1, 0: 2}[az._simulate(node)]] += 1
        print(i, int(nm[i]), counts[r], flush=True)

    idx = np.array(picked)
    out = {"index": idx.astype(np.int32), "board": g["board"][idx], "moves": g["moves"][idx], "n_moves": g["n_moves"][idx],
           "qmask": g["qmask"][idx], "n_q": g["n_q"][idx], "counts": counts, "n_sims": np.int32(N_SIMS)}
    path = os.path.join(HERE, "policy_playout_stats.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d positions x %d simulations, %d B" % (path, len(idx), N_SIMS, os.path.getsize(path)))


if __name__ == "__main__":
    main()
