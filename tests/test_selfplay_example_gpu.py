"""examples/selfplay_train.py runs one small run to the end: finite losses, and a state dict that the search loads."""
import math
import os
import re
import subprocess
import sys

import pytest
import torch

from qtttgym_amd import PolicyValueNet, SelfPlay  # noqa: F401  (the example is built on SelfPlay)
from qtttgym_amd.policy_value import SHAPES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_selfplay_train_example_runs_and_writes_weights_the_search_loads(tmp_path):
    out_path = tmp_path / "model.pt"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "selfplay_train.py"), "--games", "64",
                          "--rollouts", "8", "--sims", "2", "--epochs", "2", "--runs", "1", "--out", str(out_path)],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    m = re.search(r"run 0: (\d+) samples of 64 games .*L: (\S+), J: (\S+)", out.stdout)
    assert m, out.stdout
    n, L, J = int(m.group(1)), float(m.group(2)), float(m.group(3))
    assert 64 * 6 <= n <= 64 * 10 and math.isfinite(L) and math.isfinite(J) and L >= 0.0, out.stdout
    sd = torch.load(out_path, map_location="cpu")
    assert {k: tuple(v.shape) for k, v in sd.items()} == SHAPES
    assert all(torch.isfinite(v).all() for v in sd.values())
    PolicyValueNet(sd, device="cuda:0")
