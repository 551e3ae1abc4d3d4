#!/usr/bin/env python3
"""Generates tests/golden/selfplay_exact_plain.npz on an MI355X: the plain self-play batches that
tests/test_selfplay_exact_gpu.py relabels, recorded so that tests/test_selfplay_exact_cpu.py can assert without a GPU, with
tests/selfplay_exact_model.py alone, that they are not vacuous inputs.  Per G of selfplay_exact_model.PLAIN_GAMES:
SelfPlay(G, n_rollouts=8, net=the golden network in f32, leaf_eval="value", value_targets=(1, -1)).play(SEED), stored as
the ten rows' boards (export_boards()), length, done, mask, pi, v and winner.  The GPU test asserts that the device still
plays these very batches, bit for bit.

    python tests/golden/make_golden_selfplay_exact.py [OUT.npz]"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import nn_reference64 as R  # noqa: E402
import selfplay_exact_model as M  # noqa: E402
from qtttgym_amd import PolicyValueNet, SelfPlay  # noqa: E402

MAX_BYTES = 160000


def main(out):
    net = PolicyValueNet(R.golden_state_dict(R.load_golden()), device="cuda:0", dtype=torch.float32)
    arrays = {}
    for G in M.PLAIN_GAMES:
        sp = SelfPlay(G, n_rollouts=M.ROLLOUTS, net=net, seed=M.SEED, device="cuda:0", leaf_eval="value",
                      value_targets=(1.0, -1.0))
        b = sp.play(M.SEED)
        for k in ("length", "done", "mask", "pi", "v", "winner"):
            arrays["g%d_%s" % (G, k)] = getattr(b, k).cpu().numpy()
        rows = [{k: v.cpu().numpy() for k, v in b.row_env(t).export_boards().items()} for t in range(M.ROWS)]
        for k in M.ARRAYS:
            arrays["g%d_%s" % (G, k)] = np.stack([r[k] for r in rows])
    np.savez_compressed(out, **arrays)
    size = os.path.getsize(out)
    assert size <= MAX_BYTES, size
    print("%s: %d bytes" % (out, size))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else M.PLAIN)
