"""examples/tree_tournament.py runs to the end at a small batch and its counts add up."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tree_tournament_finishes_and_counts_add_up():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "tree_tournament.py"), "--p1", "az:8",
                          "--p2", "mcts:16", "--games", "64", "--sims", "4"],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    m = re.search(r"(\d+) games.*wins (\d+), losses (\d+), draws (\d+)", out.stdout)
    assert m, out.stdout
    n, w, l, d = map(int, m.groups())
    assert n == 64 and w + l + d == n, out.stdout
