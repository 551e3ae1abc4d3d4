"""examples/selfplay_train.py --prioritized ALPHA,BETA on the MI355X: the example trains from a prioritised ring (sample,
weighted step, priorities written back), and refuses the flag without --device-train."""
import math
import os
import re
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLE = os.path.join(ROOT, "examples", "selfplay_train.py")


def test_selfplay_train_example_with_prioritised_replay(tmp_path):
    from qtttgym_amd.policy_value import SHAPES
    out_path = tmp_path / "model.pt"
    out = subprocess.run([sys.executable, EXAMPLE, "--games", "64", "--rollouts", "8", "--sims", "2", "--runs", "2",
                          "--device-train", "--replay", "4096", "--batch", "257", "--steps", "3", "--prioritized", "0.5,1",
                          "--out", str(out_path)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    runs = re.findall(r"run (\d): .*L: (\S+), J: (\S+)", out.stdout)
    assert [r[0] for r in runs] == ["0", "1"], out.stdout
    assert all(math.isfinite(float(x)) for r in runs for x in r[1:]), out.stdout
    sd = torch.load(out_path, map_location="cpu")
    assert {k: tuple(v.shape) for k, v in sd.items()} == SHAPES
    assert all(torch.isfinite(v).all() for v in sd.values())


def test_the_flag_needs_the_device_trainer():
    out = subprocess.run([sys.executable, EXAMPLE, "--replay", "4096", "--prioritized", "0.5,1"], capture_output=True, text=True,
                         timeout=120, cwd=ROOT)
    assert out.returncode == 2 and "--prioritized needs --replay and --device-train" in out.stderr
