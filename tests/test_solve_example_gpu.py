"""examples/endgame_report.py runs one small report to the end with the golden weights, and the searched player does not
give away more than the uniform policy on the positions it is measured on."""
import math
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_endgame_report_runs_and_a_random_policy_regrets_no_less_than_the_search():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "endgame_report.py"), "--games", "32",
                          "--player", "azv:8", "--rollouts", "8"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    n = int(re.search(r"^(\d+) unfinished positions with >= 6 moves played from 32 games", out.stdout, flags=re.M).group(1))
    assert 16 <= n <= 32 * 3
    mae, bias = map(float, re.search(r"value head: mean absolute error (\S+), bias (\S+)", out.stdout).groups())
    p_opt, p_reg = map(float, re.search(r"policy: argmax optimal (\S+), expected regret (\S+)", out.stdout).groups())
    s_opt, s_reg = map(float, re.search(r"search azv:8: move optimal (\S+), regret (\S+)", out.stdout).groups())
    u_opt, u_reg = map(float, re.search(r"uniform policy: move optimal (\S+), expected regret (\S+)", out.stdout).groups())
    assert all(math.isfinite(x) for x in (mae, bias, p_reg, s_reg, u_reg))
    assert 0.0 <= mae <= 2.0 and abs(bias) <= mae + 1e-4
    assert all(0.0 <= x <= 1.0 for x in (p_opt, s_opt, u_opt)) and all(0.0 <= x <= 2.0 for x in (p_reg, s_reg, u_reg))
    assert u_reg >= s_reg                                        # searching beats moving at random
    hist = re.search(r"exact values: (.*)", out.stdout).group(1)
    counts = [int(c) for c in re.findall(r"x (\d+)", hist)]
    assert sum(counts) == n and all(float(v) * 16 == round(float(v) * 16) for v in re.findall(r"([+-]\d\.\d+) x", hist))
