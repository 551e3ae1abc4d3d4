"""CPU tests of the deep solver fixture (tests/golden/solve_deep.npz, from make_golden_solve_deep.py's selection of the C
oracle's uniform play): the classes of positions it exists for are in it, re-derived from its arrays, so that shrinking
it fails here; the Python model of the definition (tests/solve_model.py) equals it bit for bit from six moves on and on
the five-move boards that carry sixteenths or eighths; every value times 16 is an integer and none is -0.0.  No GPU."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import oracle  # noqa: E402
import solve_model as M  # noqa: E402

ARRAYS = ("board", "moves", "n_moves", "qmask", "n_q")
# The model's five-move work: of the five-move boards it follows only those that carry a sixteenth or an eighth, and the
# positions the fixture records for them are at most this many in all (the Python model takes about 7 us a position;
# a board with a sixteenth has had no collapse in five moves and is among the largest, 1.2 M positions).  The
# generator keeps the eighths with the smallest trees and fills up with boards that have none.
FIVE_MOVE_NODES_CAP = 4500000


@pytest.fixture(scope="module")
def deep():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "solve_deep.npz")))


@pytest.fixture(scope="module")
def boards(deep):
    return oracle.boards_from_arrays(*(deep[k] for k in ARRAYS))


def denominators(x):
    """The denominator 1, 2, 4, 8 or 16 of every finite entry; 0 where the entry is not finite."""
    x = np.asarray(x, dtype=np.float64)
    fin = np.isfinite(x)
    y = np.where(fin, x, 0.0)
    den = np.zeros(x.shape, dtype=np.int64)
    for d in (16, 8, 4, 2, 1):
        den[fin & (y * d == np.round(y * d))] = d
    assert (den[fin] > 0).all()
    return den


def carries(deep):
    """The boards with a sixteenth or an eighth among their q."""
    den = denominators(deep["q"])
    return ((den == 16) | (den == 8)).any(1)


@pytest.fixture(scope="module")
def modelled(deep, boards):
    """The model's solution of every board with six or more moves and of the five-move boards that carry a sixteenth or
    an eighth, once: (indices, arrays, every value met in those trees).  One solver per group, so that the memo of the
    five-move trees is not kept."""
    keep = np.flatnonzero((deep["played"] >= 6) | ((deep["played"] == 5) & carries(deep)))
    assert deep["nodes"][keep][deep["played"][keep] == 5].sum() <= FIVE_MOVE_NODES_CAP
    parts, every = [], []
    for group in (keep[deep["played"][keep] == 5], keep[deep["played"][keep] >= 6]):
        solver = M.Solver()
        parts.append(M.solve_boards(oracle.OracleBoards.from_records(boards.b[group]), solver))
        every.append(np.array([v for v, _ in solver.memo.values()]))
    return keep, {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}, np.concatenate(every)


# ---------------------------------------------------------------- the fixture holds its classes
def test_the_fixture_holds_every_class_of_position_it_exists_for(deep, boards):
    played, value, q, best, nodes = (deep[k] for k in ("played", "value", "q", "best", "nodes"))
    assert [(int(k), int((played == k).sum())) for k in np.unique(played)] == [(4, 6), (5, 64), (6, 256), (7, 256), (8, 256)]
    assert [M.played(boards.b[i].tobytes()) for i in range(boards.n)] == played.tolist()
    assert value.dtype == np.float32 and q.dtype == np.float32 and nodes.dtype == np.int64 and best.dtype == np.uint8
    winner, terminal, legal, _ = oracle.node_info(boards)
    leaf = (terminal != 0) | (legal == 0)
    assert np.array_equal(leaf, best == 255) and (nodes[leaf] == 1).all() and np.isneginf(q[leaf]).all()
    den, vden = denominators(q), denominators(value)
    has16, has8 = (den == 16).any(1), (den == 8).any(1)
    table = {}
    for k in (4, 5, 6, 7, 8):
        at = played == k
        table[k] = {"boards": int(at.sum()), "nodes": (int(nodes[at].min()), int(np.median(nodes[at])), int(nodes[at].max())),
                    "q": {d: int((den[at] == d).sum()) for d in (1, 2, 4, 8, 16)},
                    "with16": int(has16[at].sum()), "with8": int(has8[at].sum()), "value16or8": int((vden[at] >= 8).sum()),
                    "leaves": {w: int((leaf & at & (winner == w)).sum()) for w in (1, 0, -1)}}
        print(k, table[k])
    # four moves: the largest tree of the candidates, sixteenths among q, a value that is itself an odd 1/16 or 1/8
    assert table[4]["nodes"][2] >= 29000000 and table[4]["with16"] >= 2 and table[4]["value16or8"] >= 1
    # five moves: the largest tree, sixteenths, at least eight boards with an eighth, leaf roots
    assert table[5]["nodes"][2] >= 1200000 and table[5]["with16"] >= 1 and table[5]["with8"] >= 8
    assert sum(table[5]["leaves"].values()) >= 1
    # six to eight: eighths (three collapses can still follow six moves, two follow seven), the largest six-move tree,
    # leaf roots of every winner, and boards that are no leaves
    assert table[6]["with8"] >= 8 and table[6]["nodes"][2] >= 50000
    assert table[7]["q"][4] >= 8 and table[8]["q"][2] >= 8
    for k in (6, 7, 8):
        assert table[k]["with16"] == 0 and 0 < sum(table[k]["leaves"].values()) < table[k]["boards"]
        assert table[k]["leaves"][1] and table[k]["leaves"][0]
    assert sum(table[k]["leaves"][-1] for k in (6, 7, 8)) >= 1
    # an odd 16 q: what the halving of a collapse must not truncate
    assert ((q[np.isfinite(q)].astype(np.float64) * 16).astype(np.int64) & 1).sum() >= 4


# ---------------------------------------------------------------- the model against the fixture
def test_the_model_equals_the_fixture_from_six_moves_on_and_on_the_five_move_boards_with_sixteenths_or_eighths(deep, modelled):
    keep, got, _ = modelled
    den = denominators(deep["q"])
    left_out = np.setdiff1d(np.arange(len(deep["played"])), keep)
    assert (deep["played"][left_out] <= 5).all() and not carries(deep)[left_out[deep["played"][left_out] == 5]].any()
    five = keep[deep["played"][keep] == 5]
    assert len(five) >= 9 and (den[five] == 16).any(1).sum() >= 1 and (den[five] == 8).any(1).sum() >= 8
    assert (deep["played"][keep] >= 6).sum() == 768
    for k in ("value", "q"):                                         # bit for bit
        assert np.array_equal(got[k].view(np.uint32), deep[k][keep].view(np.uint32)), k
    assert np.array_equal(got["best"], deep["best"][keep]) and np.array_equal(got["nodes"], deep["nodes"][keep])


def test_every_value_times_the_denominator_is_an_integer_and_none_is_a_negative_zero(deep, modelled):
    _, got, every = modelled                                         # every: each position any modelled board's tree holds
    assert len(every) > 1000000
    for x in (every, got["value64"], got["q64"][np.isfinite(got["q64"])], deep["value"].astype(np.float64),
              deep["q"][np.isfinite(deep["q"])].astype(np.float64)):
        assert np.array_equal(x * M.DENOMINATOR, np.round(x * M.DENOMINATOR)) and (np.abs(x) <= 1).all()
        assert not np.signbit(x[x == 0]).any()
    seen = set((deep["q"][np.isfinite(deep["q"])].astype(np.float64) * 16).astype(np.int64).tolist())
    assert set(range(-16, 17, 2)) <= seen                            # every multiple of 1/8 is some action's value,
    assert any(k % 2 and k > 0 for k in seen) and any(k % 2 and k < 0 for k in seen)   # and odd sixteenths of both signs
