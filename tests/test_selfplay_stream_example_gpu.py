"""examples/selfplay_train.py --stream: every run is PLIES plies of continuous self-play that feed the ReplayBuffer, then
the run's minibatch steps, with torch autograd and with --device-train."""
import math
import os
import re
import subprocess
import sys

import pytest
import torch

from qtttgym_amd import PolicyValueNet, SelfPlay  # noqa: F401  (the example's --stream path is SelfPlay.stream)
from qtttgym_amd.policy_value import SHAPES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMMON = ["--replay", "4096", "--stream", "12", "--games", "64", "--rollouts", "8", "--runs", "2"]


@pytest.mark.parametrize("extra", [(), ("--device-train",)], ids=["autograd", "device-train"])
def test_selfplay_train_streams_games_into_the_ring(tmp_path, extra):
    out_path = tmp_path / "model.pt"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "selfplay_train.py"), *COMMON, *extra, "--sims", "2",
                          "--batch", "64", "--steps", "3", "--out", str(out_path)],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    total_games = total_samples = 0
    for run in range(2):
        m = re.search(r"run %d: 12 plies: (\d+) games harvested, (\d+) samples appended, the ring holds (\d+); 3 steps of 64 "
                      r"\(first player won (\d+), lost (\d+), drew (\d+)\); L: (\S+), J: (\S+)" % run, out.stdout)
        assert m, out.stdout
        games, samples, held, won, lost, drew = (int(x) for x in m.groups()[:6])
        # 64 slots, 12 plies, games of 5 to 9 moves: every slot finishes at least one game per run and at most three
        assert games > 0 and 64 <= games <= 3 * 64 and won + lost + drew == games
        assert 6 * games <= samples <= 10 * games
        total_games, total_samples = total_games + games, total_samples + samples
        assert held == min(total_samples, 4096)
        assert math.isfinite(float(m.group(7))) and math.isfinite(float(m.group(8))) and float(m.group(7)) >= 0.0
    sd = torch.load(out_path, map_location="cpu")
    assert {k: tuple(v.shape) for k, v in sd.items()} == SHAPES and all(torch.isfinite(v).all() for v in sd.values())
    PolicyValueNet(sd, device="cuda:0")


def test_stream_needs_a_replay_ring():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "selfplay_train.py"), "--stream", "12"],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 2 and "--replay" in out.stderr
