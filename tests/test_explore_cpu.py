"""CPU tests of root exploration (include/qttt_tree_explore.h, TreeSearch.add_root_noise, SelfPlay(root_noise=...,
sample_plies=...)): the header, the binding table, every argument error of both entries in order, the constructors'
checks, and the numpy model (tests/explore_model.py) against what does not come from it: the analytic moments of the
Dirichlet distribution, a chi-square test of the move frequencies, and the margin condition of the cases the GPU tests
compare with the model.  No GPU."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "qttt_tree_explore.h")

import explore_model as E  # noqa: E402
from qtttgym_amd import SelfPlay, TreeSearch, _native  # noqa: E402

ERR_NULL, ERR_SIZE, ERR_ACTION = -1, -2, -3
NOISE, SAMPLED = "qttt_tree_root_noise", "qttt_selfplay_record_sampled"


# ---------------------------------------------------------------- header, binding table
def test_header_is_plain_c99_included_by_qttt_h_last_and_its_constants_are_the_bindings():
    src = open(os.path.join(ROOT, "include", "qttt.h")).read()
    assert src.index('#include "qttt_tree_value.h"') < src.index('#include "qttt_tree_explore.h"')
    consts = ("QTTT_TREE_NOISE_BASE == %du && QTTT_TREE_NOISE_TRIES == %d && QTTT_TREE_NOISE_DRAWS == %d && "
              "QTTT_SELFPLAY_MOVE_BASE == %du && QTTT_TREE_MAX_NOISE == %du && QTTT_ABI_VERSION == %d"
              % (_native.TREE_NOISE_BASE, _native.TREE_NOISE_TRIES, _native.TREE_NOISE_DRAWS, _native.SELFPLAY_MOVE_BASE,
                 _native.TREE_MAX_NOISE, _native.ABI_VERSION))
    prog = ('#include "qttt.h"\ntypedef char constants_agree[(%s) ? 1 : -1];\nint main(void){\n'
            'int (*f)(void *, int64_t, int64_t, uint64_t, uint32_t, int64_t, double, double, double *, uint8_t *, void *)'
            ' = qttt_tree_root_noise;\n'
            'int (*r)(const void *, int64_t, int64_t, int, uint32_t, double, double, double, void *, double *, uint8_t *, '
            'uint8_t *, float *, uint8_t *, uint8_t *, int8_t *, uint8_t *, uint64_t, int64_t, double, int, void *)'
            ' = qttt_selfplay_record_sampled;\nreturn f == 0 || r == 0 || sizeof(constants_agree) != 1;}\n' % consts)
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-x", "c",
                          "-I" + os.path.join(ROOT, "include"), "-"], input=prog, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    wrong = subprocess.run(["gcc", "-std=c99", "-fsyntax-only", "-x", "c", "-I" + os.path.join(ROOT, "include"), "-"],
                           input=prog.replace("QTTT_TREE_NOISE_TRIES == ", "QTTT_TREE_NOISE_TRIES == 1 + "),
                           capture_output=True, text=True)
    assert wrong.returncode != 0                             # the comparison is really made


def test_the_draw_ranges_are_disjoint():
    base, draws, top = _native.TREE_NOISE_BASE, _native.TREE_NOISE_DRAWS, _native.TREE_MAX_NOISE
    assert draws == 2 * _native.TREE_NOISE_TRIES + 1 == 33 and top == 451911
    assert base >= _native.TREE_SELECT_BASE + _native.TREE_MAX_ROLLOUTS          # above select's range
    last = base + ((top - 1) * 36 + 35) * draws + draws - 1                     # the last index a noise call can use
    assert last < _native.SELFPLAY_MOVE_BASE <= base + (top * 36 + 35) * draws + draws - 1      # and top is the largest
    assert _native.SELFPLAY_MOVE_BASE + _native.SELFPLAY_ROWS - 1 < 1 << 32


def test_binding_header_exports_and_build_list_agree():
    import __graft_entry__ as entry
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = set(re.findall(r"^(?:int|int64_t)\s+(qttt_\w+)\s*\(", src, flags=re.M))
    assert names == set(_native.TREE_EXPLORE_SIGNATURES) == {NOISE, SAMPLED}
    assert not names & (set(_native.SIGNATURES) | set(_native.TREE_SIGNATURES) | set(_native.SELFPLAY_SIGNATURES)
                        | set(_native.TREE_VALUE_SIGNATURES))
    assert HEADER in entry.HEADERS
    L = _native.lib()
    for name in names:
        assert getattr(ctypes.CDLL(_native.LIB_PATH), name)
        assert getattr(L, name).argtypes == _native.TREE_EXPLORE_SIGNATURES[name][1]
    # the sampled record takes the record's arguments, then its own four, then the stream
    assert _native.TREE_EXPLORE_SIGNATURES[SAMPLED][1][:17] == _native.SELFPLAY_SIGNATURES["qttt_selfplay_record"][1][:17]
    assert L.qttt_abi_version() == _native.ABI_VERSION == 6             # additive entries: the ABI number stays
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert NOISE in text and SAMPLED in text, doc


# ---------------------------------------------------------------- argument errors
def _noise(L, tree=0x1000, games=1, capacity=8, seed=1, noise_idx=0, board_offset=0, epsilon=0.25, alpha=0.3, noise=0x2000,
           applied=0x3001):
    """The entry with fake addresses (never dereferenced: every call of this file fails its checks first)."""
    return L.qttt_tree_root_noise(tree, games, capacity, seed, noise_idx, board_offset, epsilon, alpha, noise, applied, None)


def test_root_noise_return_codes_in_documented_order_without_device_work():
    L = _native.lib()
    inf, nan = float("inf"), float("nan")
    for kw in (dict(games=-1), dict(capacity=0), dict(capacity=(1 << 30) + 1), dict(board_offset=-1),
               dict(noise_idx=_native.TREE_MAX_NOISE), dict(noise_idx=(1 << 32) - 1), dict(epsilon=-1e-9),
               dict(epsilon=1.0 + 1e-9), dict(epsilon=nan), dict(epsilon=inf), dict(alpha=0.0), dict(alpha=-0.3),
               dict(alpha=nan), dict(alpha=inf)):
        assert _noise(L, **kw) == ERR_SIZE, kw
        assert _noise(L, tree=None, **kw) == ERR_SIZE, kw                       # sizes first, even with a null
        assert _noise(L, tree=0x1001, noise=0x2001, **kw) == ERR_SIZE, kw       # or misaligned pointers
        assert _noise(L, **{"games": 0, **kw}) == ERR_SIZE or "games" in kw     # and before the empty batch
    assert _noise(L, games=0, tree=None, noise=0x2001) == 0                     # games == 0: no pointer looked at
    assert _noise(L, tree=None) == ERR_NULL
    assert _noise(L, tree=None, noise=0x2001) == ERR_NULL                       # null before alignment
    assert _noise(L, tree=0x1008) == ERR_ACTION
    assert _noise(L, noise=0x2004) == ERR_ACTION and _noise(L, noise=0x2001) == ERR_ACTION
    # the largest noise_idx and the ends of epsilon's range pass the size checks (and then stop at the null tree)
    assert _noise(L, tree=None, noise_idx=_native.TREE_MAX_NOISE - 1, epsilon=0.0) == ERR_NULL
    assert _noise(L, tree=None, epsilon=1.0, noise=None, applied=None) == ERR_NULL


def _sampled(L, tree=0x1000, games=1, capacity=8, ply=0, n_rollouts=4, alpha=1.0, v_first=1.0, v_second=0.0, bufs=None, seed=1,
             board_offset=0, temperature=1.0, sample_plies=10):
    bufs = [0x2000 + 0x100 * k for k in range(9)] if bufs is None else bufs
    return L.qttt_selfplay_record_sampled(tree, games, capacity, ply, n_rollouts, alpha, v_first, v_second, *bufs, seed,
                                          board_offset, temperature, sample_plies, None)


def test_sampled_record_return_codes_in_documented_order_without_device_work():
    L = _native.lib()
    nothing = [None] * 9
    inf, nan = float("inf"), float("nan")
    for kw in (dict(games=-1), dict(capacity=0), dict(capacity=(1 << 30) + 1), dict(ply=-1), dict(ply=10),
               dict(n_rollouts=0), dict(alpha=0.0), dict(alpha=-1.0), dict(alpha=nan), dict(alpha=inf),
               dict(v_first=nan), dict(v_first=-inf), dict(v_second=inf), dict(v_second=nan),
               dict(board_offset=-1), dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=nan),
               dict(temperature=inf), dict(sample_plies=-1), dict(sample_plies=11)):
        assert _sampled(L, **kw) == ERR_SIZE, kw
        assert _sampled(L, tree=None, bufs=nothing, **kw) == ERR_SIZE, kw
        assert _sampled(L, tree=0x1001, bufs=[0x2001] * 9, **kw) == ERR_SIZE, kw
    assert _sampled(L, games=0, tree=None, bufs=nothing) == 0
    assert _sampled(L, games=0, tree=0x1001, bufs=[0x2001] * 9, ply=9, sample_plies=0) == 0
    assert _sampled(L, games=0, temperature=0.0) == ERR_SIZE
    assert _sampled(L, tree=None) == ERR_NULL
    assert _sampled(L, tree=None, bufs=[0x2001] * 9) == ERR_NULL
    for k in range(9):
        bufs = [0x2001] * 9
        bufs[k] = None
        assert _sampled(L, bufs=bufs) == ERR_NULL, k
        assert _sampled(L, tree=0x1008, bufs=bufs) == ERR_NULL, k
    odd = [0x2000, 0x3000, 0x4001, 0x4003, 0x5000, 0x6001, 0x6003, 0x6005, 0x6007]
    assert _sampled(L, tree=0x1008, bufs=odd) == ERR_ACTION
    for k, off in ((0, 8), (0, 1), (1, 4), (1, 1), (4, 2), (4, 1)):         # states, pi, v
        bufs = list(odd)
        bufs[k] += off
        assert _sampled(L, bufs=bufs) == ERR_ACTION, (k, off)


# ---------------------------------------------------------------- the constructors
def test_selfplay_checks_the_exploration_arguments_before_it_asks_for_a_device():
    nan, inf = float("nan"), float("inf")
    for kw in (dict(root_noise=(0.25,)), dict(root_noise=(0.25, 0.3, 1.0)), dict(root_noise=(-0.1, 0.3)),
               dict(root_noise=(1.1, 0.3)), dict(root_noise=(nan, 0.3)), dict(root_noise=(0.25, 0.0)),
               dict(root_noise=(0.25, -1.0)), dict(root_noise=(0.25, inf)), dict(root_noise=(0.25, nan)),
               dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=nan), dict(temperature=inf),
               dict(sample_plies=-1), dict(sample_plies=11)):
        with pytest.raises(ValueError):
            SelfPlay(**{"num_games": 4, **kw})
    with pytest.raises(_native.QtttNativeError):             # valid arguments get as far as the device: there is no CPU path
        SelfPlay(4, root_noise=(0.25, 0.3), temperature=0.5, sample_plies=10, device="cpu")


class _Calls:
    """A TreeSearch that was never opened on a device: add_root_noise's own checks, and what it would launch."""

    def __init__(self):
        t = TreeSearch.__new__(TreeSearch)
        t.num_games, t.capacity, t.seed, t.board_offset, t.device = 4, 8, 3, 9, "nowhere"
        t.tree = type("Buf", (), {"data_ptr": staticmethod(lambda: 0x1000)})()
        t.noise_idx, t._bound, self.calls = 0, None, []
        t._call = lambda name, *args: self.calls.append((name, args))
        self.t = t


def test_add_root_noise_checks_counts_and_stops_at_the_bound():
    c = _Calls()
    t = c.t
    with pytest.raises(RuntimeError):
        t.add_root_noise()                                   # reset() first
    t._bound = 1
    for kw in (dict(epsilon=-0.1), dict(epsilon=1.5), dict(epsilon=float("nan")), dict(alpha=0.0), dict(alpha=-1.0),
               dict(alpha=float("inf")), dict(alpha=float("nan"))):
        with pytest.raises(ValueError):
            t.add_root_noise(**kw)
    assert not c.calls and t.noise_idx == 0
    t.add_root_noise()
    t.add_root_noise(0.5, 1.0)
    assert t.noise_idx == 2
    assert c.calls == [(NOISE, (0x1000, 4, 8, 3, 0, 9, 0.25, 0.3, 0, 0)), (NOISE, (0x1000, 4, 8, 3, 1, 9, 0.5, 1.0, 0, 0))]
    t.noise_idx = _native.TREE_MAX_NOISE - 1
    t.add_root_noise()
    with pytest.raises(ValueError):
        t.add_root_noise()                                   # would pass QTTT_TREE_MAX_NOISE
    assert len(c.calls) == 3 and t.noise_idx == _native.TREE_MAX_NOISE


# ---------------------------------------------------------------- the model against the Dirichlet distribution
@pytest.mark.parametrize("alpha", [0.3, 1.0, 2.5])
@pytest.mark.parametrize("m", [36, 21, 3])
def test_model_noise_has_the_moments_of_the_symmetric_dirichlet(m, alpha):
    """4 096 games with m legal actions.  Every action's marginal is Beta(alpha, (m - 1) alpha): mean 1 / m, variance
    (1 / m)(1 - 1 / m) / (m alpha + 1).  The mean is asserted per action, within 5 standard errors.  The variance is the
    one variance all m marginals share, estimated from all of them (the mean of the per-action sample variances), within
    10 %: a single action's sample variance over 4 096 draws of Beta(0.3, 10.5) has a standard error of some 7 % by
    itself, the estimate over 36 actions of about 1 %."""
    games = 4096
    legal = sorted(np.random.default_rng(m).choice(36, m, replace=False).tolist())
    n, applied, _ = E.noise_rows(E.SEED, E.OFFSET, 0, [legal] * games, alpha)
    assert applied.all() and not n[:, [a for a in range(36) if a not in legal]].any()
    np.testing.assert_allclose(n.sum(1), 1.0, rtol=0, atol=1e-14)
    assert (n[:, legal] > 0).all()
    var = (1.0 / m) * (1.0 - 1.0 / m) / (m * alpha + 1.0)
    z = np.abs(n[:, legal].mean(0) - 1.0 / m) / np.sqrt(var / games)
    ratio = n[:, legal].var(0).mean() / var
    print("m = %d, alpha = %g: largest |mean - 1/m| = %.2f standard errors, variance / analytic = %.4f" % (m, alpha, z.max(), ratio))
    assert z.max() < 5.0
    assert abs(ratio - 1.0) < 0.10


def test_model_noise_of_a_root_without_legal_actions_or_with_a_vanishing_sum_is_not_applied():
    n, applied, _ = E.noise_rows(E.SEED, E.OFFSET, 0, [[], [0, 5]], 0.3)
    assert applied.tolist() == [False, True] and not n[0].any()
    n, applied, _ = E.noise_rows(E.SEED, E.OFFSET, 0, [[0, 5]], 1e-8)      # u ** 1e8 underflows: S = 0
    assert not applied[0] and not n.any()


def test_model_mix():
    n = np.zeros(36)
    n[[1, 4]] = (0.75, 0.25)
    p = np.zeros(36)
    p[[1, 4]] = 0.5
    out = E.mix(p, n, [1, 4], 0.25)
    assert out.dtype == np.float32 and out[1] == np.float32(0.5625) and out[4] == np.float32(0.4375) and out.sum() == 1.0
    third = np.full(36, 1.0 / 3.0)
    kept = E.mix(third, n, [1, 4, 7], 0.0)[7]                # epsilon = 0 still rounds 1 / m to f32
    assert kept == np.float32(1.0 / 3.0) and float(kept) != 1.0 / 3.0


# ---------------------------------------------------------------- the model's moves against N / sum N
def test_model_move_frequencies_pass_a_chi_square_test():
    """20 000 draws at temperature 1 for one N vector with zeros in it: legal actions with N = 0 and illegal actions with
    N > 0 are never drawn, the other six follow N / sum N.  Chi-square with 5 degrees of freedom at the 0.1 % level: the
    critical value is 20.515 (tables of the chi-square distribution)."""
    N = np.zeros(36, dtype=np.int64)
    N[[2, 3, 9, 17, 30, 35]] = (5, 1, 12, 2, 7, 3)
    N[20] = 4                                                # not legal: never drawn
    legal = [0, 2, 3, 9, 10, 17, 30, 35]
    draws = 20000
    count = np.zeros(36)
    for g in range(draws):
        a, _ = E.sample_move(N, legal, E.SEED, E.OFFSET + g, 0, 1.0)
        count[a] += 1
    live = [2, 3, 9, 17, 30, 35]
    assert count.sum() == draws == count[live].sum()
    expected = draws * N[live] / N[live].sum()
    chi2 = float(((count[live] - expected) ** 2 / expected).sum())
    print("chi-square %.3f (5 degrees of freedom, critical 20.515)" % chi2)
    assert chi2 < 20.515


def test_model_move_falls_back_without_a_visit_and_sharpens_with_a_low_temperature():
    legal = [0, 2, 3]
    assert E.sample_move(np.zeros(36, dtype=np.int64), legal, 1, 2, 0, 1.0) == (None, np.inf)
    N = np.zeros(36, dtype=np.int64)
    N[[0, 2, 3]] = (1, 100, 1)
    cold = [E.sample_move(N, legal, 1, g, 3, 0.1)[0] for g in range(200)]
    assert set(cold) == {2}                                  # 100 ** 10 against 1
    warm = [E.sample_move(N, legal, 1, g, 3, 1.0)[0] for g in range(2000)]
    assert set(warm) == {0, 2, 3}


# ---------------------------------------------------------------- the margin condition of the GPU tests' cases
def test_every_decision_of_the_gpu_tests_cases_has_a_margin():
    """A condition on the inputs of tests/test_explore_gpu.py, not a tolerance: the device's log, cos and pow are a few
    ulps from numpy's, so a decision whose two sides are 1e-9 apart or more comes out the same on both.  Every Gamma
    decision of every noise case (all 36 actions of every game: a superset of any root's legal ones), and every move
    drawn at temperature 0.5 in the whole games, none left out."""
    decisions, narrowest = 0, np.inf
    for seed, offset, noise_idx, games in E.NOISE_CASES:
        for _, alpha in E.NOISE_PARAMS:
            _, applied, margins = E.noise_rows(seed, offset, noise_idx, [list(range(36))] * games, alpha)
            assert applied.all() and len(margins) >= games * 36
            assert margins.min() > 1e-9, (seed, offset, noise_idx, alpha, margins.min())
            decisions, narrowest = decisions + len(margins), min(narrowest, float(margins.min()))
    _, _, margins = E.play(*E.PLAY, temperature=0.5, sample_plies=10)
    assert len(margins) >= 5 * E.PLAY[0] and min(margins) > 1e-9, min(margins)
    print("%d Gamma decisions, the narrowest margin %.3g; %d moves, the narrowest margin %.3g"
          % (decisions, narrowest, len(margins), min(margins)))
