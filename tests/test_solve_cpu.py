"""CPU tests of the exact endgame solver (include/qttt_solve.h, qtttgym_amd.solve): the header, the binding table and the
exports; every documented argument error, in order, with no device; the Python model of the definition
(tests/solve_model.py) against the recorded fixture (tests/golden/solve_positions.npz, from the C oracle), its
denominator bound, hand-built positions, and the definition's invariants on the fixture.  No GPU."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "qttt_solve.h")

import oracle  # noqa: E402
import solve_model as M  # noqa: E402
from qtttgym_amd import _native, move2ind  # noqa: E402

ERR_NULL, ERR_SIZE, ERR_ACTION = -1, -2, -3


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "solve_positions.npz")))


@pytest.fixture(scope="module")
def solver():
    return M.Solver()


@pytest.fixture(scope="module")
def modelled(golden, solver):
    """The model's solution of every fixture board with five or more moves played, computed once."""
    keep = np.flatnonzero(golden["played"] >= 5)
    ob = oracle.boards_from_arrays(*(golden[k][keep] for k in ("board", "moves", "n_moves", "qmask", "n_q")))
    return keep, M.solve_boards(ob, solver)


# ---------------------------------------------------------------- header, binding table, exports
def test_binding_header_exports_and_build_list_agree():
    import __graft_entry__ as entry
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = set(re.findall(r"^(?:int|int64_t)\s+(qttt_\w+)\s*\(", src, flags=re.M))
    assert names == set(_native.SOLVE_SIGNATURES) == {"qttt_solve"}
    assert not names & set(_native.SIGNATURES)                   # qttt.h's own table does not grow
    assert HEADER in entry.HEADERS
    assert os.path.join(ROOT, "qtttgym_amd", "csrc", "qttt_solve_kernels.h") in entry.HEADERS
    L = _native.lib()
    assert getattr(ctypes.CDLL(_native.LIB_PATH), "qttt_solve")
    assert L.qttt_solve.argtypes == _native.SOLVE_SIGNATURES["qttt_solve"][1]
    assert L.qttt_abi_version() == _native.ABI_VERSION == 6            # an additive entry: the ABI number stays
    for const, want in (("MIN_PLY", 4), ("MAX_PLY", 9), ("DENOMINATOR", 16)):
        m = re.search(r"#define QTTT_SOLVE_%s (\d+)" % const, src)
        assert m and int(m.group(1)) == getattr(_native, "SOLVE_" + const) == want, const
    assert M.DENOMINATOR == _native.SOLVE_DENOMINATOR
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        assert "qttt_solve" in open(os.path.join(ROOT, doc)).read(), doc


def test_header_is_plain_c99_and_included_by_qttt_h_last():
    src = open(os.path.join(ROOT, "include", "qttt.h")).read()
    assert src.index('#include "qttt_selfplay_stream.h"') < src.index('#include "qttt_solve.h"')
    prog = ('#include "qttt.h"\nint main(void){'
            'int (*s)(const void *, int64_t, int, float *, float *, uint8_t *, int64_t *, uint8_t *, void *) = qttt_solve;\n'
            'return s == 0 || QTTT_SOLVE_MIN_PLY != 4 || QTTT_ABI_VERSION != 6;}\n')
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-x", "c",
                          "-I" + os.path.join(ROOT, "include"), "-"], input=prog, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_the_kernel_file_comes_after_the_search_core_and_respells_no_rule():
    hip = open(os.path.join(ROOT, "qtttgym_amd", "csrc", "qttt_kernels.hip")).read()
    assert hip.index('#include "qttt_selfplay_stream_kernels.h"') < hip.index('#include "qttt_solve_kernels.h"') \
        < hip.index('#include "qttt_launch.h"')
    src = open(os.path.join(ROOT, "qtttgym_amd", "csrc", "qttt_solve_kernels.h")).read()
    for rule in ("expand_pair(", "update_winner_from_step(", "lite_update_winner(", "fill_legal_lut<", "leaf_turn_signed(",
                 "pair_action<"):
        assert rule in src, rule
    assert "step_core" not in src and "atomicAdd(&n_items" in src
    assert not re.search(r"atomic\w*\([^)]*float", src)               # no floating-point atomics


# ---------------------------------------------------------------- argument errors, in the documented order
def _solve(L, state=0x10000, n=1, min_ply=5, value=0x20000, q=0x30000, best=0x40001, nodes=0x50000, status=0x60001):
    return L.qttt_solve(state, n, min_ply, value, q, best, nodes, status, None)


def test_every_argument_error_in_its_documented_order():
    L = _native.lib()
    # sizes first, whatever the pointers are
    for kw in ({"n": -1}, {"min_ply": 3}, {"min_ply": 10}, {"min_ply": 0}, {"min_ply": -4}):
        assert _solve(L, **kw) == ERR_SIZE, kw
        assert _solve(L, state=None, value=0x20001, **kw) == ERR_SIZE, kw
    assert _solve(L, n=-1, min_ply=3) == ERR_SIZE
    # then the empty batch: nothing to do, no pointer looked at
    assert _solve(L, n=0, state=None) == 0 and _solve(L, n=0, state=0x10001, value=0x20001, nodes=0x50004) == 0
    for m in range(4, 10):
        assert _solve(L, n=0, min_ply=m) == 0
    # then the one required pointer, before any alignment
    assert _solve(L, state=None) == ERR_NULL and _solve(L, state=None, value=0x20001, q=0x30002, nodes=0x50004) == ERR_NULL
    # then alignment: state 16 bytes, value and q 4, nodes 8; best and status take any address
    for kw in ({"state": 0x10008}, {"state": 0x10001}, {"value": 0x20002}, {"q": 0x30001}, {"nodes": 0x50004}):
        assert _solve(L, **kw) == ERR_ACTION, kw
    # every output null passes every check and has nothing to compute
    assert _solve(L, value=None, q=None, best=None, nodes=None, status=None) == 0


def test_the_package_exports_the_result_and_checks_min_ply_before_it_asks_for_a_device():
    import qtttgym_amd
    from qtttgym_amd import SolveResult, VecEnv
    from qtttgym_amd.solve import check_min_ply, default_boards_per_launch
    assert "SolveResult" in qtttgym_amd.__all__ and callable(VecEnv.solve)
    for bad in (3, 10, 0, -1):
        with pytest.raises(ValueError):
            check_min_ply(bad)
    assert [check_min_ply(m) for m in range(4, 10)] == list(range(4, 10))
    assert default_boards_per_launch(4) < default_boards_per_launch(5)
    assert all(default_boards_per_launch(m) is None for m in range(6, 10))       # from six moves on: one launch


def test_regret_is_zero_for_an_optimal_move_inf_for_an_illegal_one_and_nan_for_a_skipped_board():
    from qtttgym_amd import SolveResult
    inf, nan = float("inf"), float("nan")
    q = torch.full((3, 36), -inf)
    q[0, 3], q[0, 7], q[1, 0] = 0.5, -0.25, 1.0
    q[2] = nan
    r = SolveResult(torch.tensor([0.5, 1.0, nan]), q, torch.tensor([3, 0, 255], dtype=torch.uint8),
                    torch.tensor([9, 5, 0]), torch.tensor([True, True, False]))
    assert r.regret([3, 0, 4]).tolist()[:2] == [0.0, 0.0] and torch.isnan(r.regret([3, 0, 4])[2])
    assert r.regret(torch.tensor([7, 5, 0])).tolist()[:2] == [0.75, inf]
    with pytest.raises(ValueError):
        r.regret([0, 36, 0])
    with pytest.raises(ValueError):
        r.regret([0, 1])


# ---------------------------------------------------------------- the model against the fixture
def test_the_fixture_holds_what_it_should(golden):
    played = golden["played"]
    assert [(int(k), int((played == k).sum())) for k in np.unique(played)] == [(4, 2), (5, 8), (6, 32), (7, 32), (8, 32)]
    ob = oracle.boards_from_arrays(*(golden[k] for k in ("board", "moves", "n_moves", "qmask", "n_q")))
    assert [M.played(ob.b[i].tobytes()) for i in range(ob.n)] == played.tolist()
    leaf = golden["best"] == 255
    for k in (6, 7, 8):                                              # leaf roots among the late boards
        assert leaf[played >= 6].any() and not leaf[played == k].all()
    assert (golden["nodes"][leaf] == 1).all() and np.isneginf(golden["q"][leaf]).all()
    assert golden["value"].dtype == np.float32 and golden["q"].dtype == np.float32 and golden["nodes"].dtype == np.int64


def test_the_model_equals_the_fixture_on_every_board_with_five_or_more_moves(golden, modelled):
    keep, got = modelled
    assert len(keep) == 104
    for k in ("value", "q"):                                         # bit for bit
        assert np.array_equal(got[k].view(np.uint32), golden[k][keep].view(np.uint32)), k
    assert np.array_equal(got["best"], golden["best"][keep]) and np.array_equal(got["nodes"], golden["nodes"][keep])


def test_every_value_times_the_denominator_is_an_integer_and_none_is_a_negative_zero(golden, modelled, solver):
    _, got = modelled
    every = np.array([v for v, _ in solver.memo.values()])           # every position any fixture board's tree holds
    assert len(every) > 10000
    for x in (every, got["value64"], got["q64"][np.isfinite(got["q64"])], golden["value"].astype(np.float64),
              golden["q"][np.isfinite(golden["q"])].astype(np.float64)):
        assert np.array_equal(x * M.DENOMINATOR, np.round(x * M.DENOMINATOR)) and (np.abs(x) <= 1).all()
        assert not np.signbit(x[x == 0]).any()
    assert len(np.unique(every)) > 8                                 # the values are not trivial


def test_the_definitions_invariants_hold_on_the_fixture(golden):
    value, q, best, nodes = (golden[k] for k in ("value", "q", "best", "nodes"))
    ob = oracle.boards_from_arrays(*(golden[k] for k in ("board", "moves", "n_moves", "qmask", "n_q")))
    _, terminal, legal, _ = oracle.node_info(ob)
    for i in range(ob.n):
        mask = np.array([(int(legal[i]) >> a) & 1 for a in range(36)], dtype=bool)
        if terminal[i] or not mask.any():
            assert best[i] == 255 and nodes[i] == 1 and np.isneginf(q[i]).all() and value[i] in (-1.0, 0.0, 1.0)
            continue
        assert np.isneginf(q[i][~mask]).all() and np.isfinite(q[i][mask]).all()
        assert value[i] == q[i][mask].max()                          # V = max over the legal actions
        assert best[i] == np.flatnonzero(q[i] == value[i])[0] and mask[best[i]]      # the lowest argmax
        assert nodes[i] > 1 + mask.sum()


# ---------------------------------------------------------------- hand-built positions
def _play(moves_bits):
    ob = oracle.OracleBoards(1)
    for t, (a, c, bit) in enumerate(moves_bits):
        ob.step(np.array([[a, c]], dtype=np.uint8), np.array([bit], dtype=np.uint8))
    return ob


def test_a_certain_line_is_worth_one_and_best_is_the_lowest_winning_pair(solver):
    # X holds 0 and 3 after two collapses (O holds 1 and 4), then X plays (6, 8) and O (2, 5).  X to move: (6, 8) again
    # closes a cycle of X's own two moves, so X lands on 6 whichever way the coin falls, and 0-3-6 is a line.
    for b0 in (0, 1):
        for b1 in (0, 1):
            ob = _play([(0, 1, 0), (0, 1, b0), (3, 4, 0), (3, 4, b1), (6, 8, 0), (2, 5, 0)])
            if not (ob.board[0][0] == 0 and ob.board[0][3] == 2):    # the collapse that gave X squares 0 and 3
                continue
            r = solver.solve(ob.b[0])
            a = move2ind(6, 8)
            assert M.played(ob.b[0].tobytes()) == 6 and not r["leaf"]
            assert r["value"] == 1.0 and r["q"][a] == 1.0
            assert r["best"] == a == int(np.flatnonzero(r["q"] == 1.0)[0])      # the only certain win
            assert (r["q"][np.isfinite(r["q"])] < 1.0).any()          # and not every move wins
            return
    raise AssertionError("no collapse gave X squares 0 and 3")


def test_a_full_board_is_a_leaf_with_one_node(solver):
    seen = 0
    ob = oracle.OracleBoards(64)
    for t in range(9):
        ob.step(ob.sample_actions(7, t), None, 7, t)
    winner, terminal, legal, _ = oracle.node_info(ob)
    for i in range(ob.n):
        if (ob.board[i] >= 0).all():                                 # nine classical squares
            r = solver.solve(ob.b[i])
            first_to_move = M.played(ob.b[i].tobytes()) % 2 == 0
            want = 0.0 if winner[i] < 0 else (1.0 if (winner[i] == 1) == first_to_move else -1.0)
            assert r["leaf"] and r["nodes"] == 1 and r["best"] == 255 and r["value"] == want
            assert np.isneginf(r["q"]).all() and legal[i] == 0
            seen += 1
    assert seen >= 8
