"""examples/selfplay_train.py --replay: two runs append their games to a ReplayBuffer and train minibatch steps drawn
from it with random symmetries; the path without --replay still runs as it did."""
import math
import os
import re
import subprocess
import sys

import pytest
import torch

from qtttgym_amd import PolicyValueNet, ReplayBuffer  # noqa: F401  (the example's --replay path is built on ReplayBuffer)
from qtttgym_amd.policy_value import SHAPES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMMON = ["--games", "16", "--rollouts", "8", "--runs", "2"]


def run_example(tmp_path, *extra):
    out_path = tmp_path / "model.pt"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "selfplay_train.py"), *COMMON, *extra, "--out", str(out_path)],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    sd = torch.load(out_path, map_location="cpu")
    assert {k: tuple(v.shape) for k, v in sd.items()} == SHAPES and all(torch.isfinite(v).all() for v in sd.values())
    return out.stdout, sd


def test_selfplay_train_with_a_replay_ring_trains_minibatches_with_finite_losses(tmp_path):
    stdout, sd = run_example(tmp_path, "--replay", "4096", "--batch", "64", "--steps", "3")
    held = []
    for run in range(2):
        m = re.search(r"run %d: 16 games appended, the ring holds (\d+) samples; 3 steps of 64 .*L: (\S+), J: (\S+)" % run, stdout)
        assert m, stdout
        L, J = float(m.group(2)), float(m.group(3))
        assert math.isfinite(L) and math.isfinite(J) and L >= 0.0, stdout
        held.append(int(m.group(1)))
    assert 16 * 6 <= held[0] <= 16 * 10 and held[0] + 16 * 6 <= held[1] <= held[0] + 16 * 10      # the ring keeps the first run's games
    PolicyValueNet(sd, device="cuda:0")


def test_selfplay_train_without_replay_still_runs(tmp_path):
    stdout, _ = run_example(tmp_path, "--sims", "2", "--epochs", "2")
    for run in range(2):
        m = re.search(r"run %d: (\d+) samples of 16 games .*L: (\S+), J: (\S+)" % run, stdout)
        assert m and math.isfinite(float(m.group(2))) and math.isfinite(float(m.group(3))), stdout
