#!/usr/bin/env python3
"""Generates tests/golden/symmetry_traces.npz from the UNMODIFIED reference's Board / QEvalClassic, loaded through
ref_shim.py.  Build container only; the .npz is data (inputs + expected outputs).

512 random games, each played twice: as it is (side a), and under a random symmetry k (side b) — every move (lo, hi)
as (sigma(lo), sigma(hi)) and the square forced on random.choice (qeval.py:35) as sigma of the original game's.  After
every ply both boards' attributes are recorded: board, moves, qstructs (masks in LIST ORDER) and their number.

The group is restated here from its definition (include/qttt_symmetry.h) so that the recorder needs nothing but the
reference.  The seed is chosen so that at least 20 recorded positions have a mirrored qstructs list whose order is NOT
the permuted order of the original's (update_qstructs keeps a union at the place of the set holding the move's lower
square); the recorder asserts it.
"""
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from ref_shim import load_reference  # noqa: E402

GAMES, SEED, MIN_ORDER_CASES = 512, 20261018, 20


def sigma(k):
    out = []
    for v in range(9):
        r, c = divmod(v, 3)
        if k & 4:
            c = 2 - c
        for _ in range(k & 3):
            r, c = c, 2 - r
        out.append(3 * r + c)
    return out


class Landing:
    """random.choice stand-in: the closing move lands on the square it is told to."""

    def __init__(self):
        self.square = None

    def choice(self, seq):
        assert self.square in seq, (self.square, seq)
        return self.square


def attrs(b):
    mv = [[255, 255] for _ in range(9)]
    for i, m in enumerate(b.moves):
        mv[i] = [m[0], m[1]]
    qm = [0] * 4
    for i, s in enumerate(b.qstructs):
        qm[i] = sum(1 << x for x in s)
    return list(b.board), mv, len(b.moves), qm, len(b.qstructs)


def main():
    qtttgym, _ = load_reference()
    land = Landing()
    qtttgym.qeval.random = land
    rng = random.Random(SEED)
    keys = ("board", "moves", "n_moves", "qmask", "n_q")
    dtypes = {"board": np.int8, "moves": np.uint8, "n_moves": np.uint8, "qmask": np.uint16, "n_q": np.uint8}
    pad = dict(zip(keys, attrs(qtttgym.Board(qtttgym.QEvalClassic()))))
    rec = {side + "_" + k: [] for side in "ab" for k in keys}
    ks, n_plies, move, landing = [], [], [], []
    positions = order_cases = 0
    for _ in range(GAMES):
        k = rng.randrange(8)
        s = sigma(k)
        a, b = qtttgym.Board(qtttgym.QEvalClassic()), qtttgym.Board(qtttgym.QEvalClassic())
        rows = {name: [] for name in rec}
        mv, ld = [], []
        while len(a.moves) < 9 and max(a.check_win()) <= 0:
            free = [v for v in range(9) if a.board[v] == -1]
            lo, hi = sorted(rng.sample(free, 2))
            L = rng.choice((lo, hi))
            land.square = L
            a.make_move((lo, hi))
            land.square = s[L]
            b.make_move((s[lo], s[hi]))
            mv.append([lo, hi])
            ld.append(L)
            for side, brd in (("a", a), ("b", b)):
                for name, val in zip(keys, attrs(brd)):
                    rows[side + "_" + name].append(val)
            positions += 1
            order_cases += [sum(1 << s[x] for x in c) for c in a.qstructs] != [sum(1 << x for x in c) for c in b.qstructs]
        assert max(b.check_win()) == max(a.check_win()) and len(a.moves) == len(b.moves)
        ks.append(k)
        n_plies.append(len(mv))
        fill = 9 - len(mv)
        move.append(mv + [[255, 255]] * fill)
        landing.append(ld + [255] * fill)
        for name in rec:
            rec[name].append(rows[name] + [pad[name[2:]]] * fill)
    assert order_cases >= MIN_ORDER_CASES, order_cases
    out = {"k": np.array(ks, dtype=np.uint8), "n_plies": np.array(n_plies, dtype=np.uint8),
           "move": np.array(move, dtype=np.uint8), "landing": np.array(landing, dtype=np.uint8)}
    for name, val in rec.items():
        out[name] = np.array(val, dtype=dtypes[name[2:]])
    path = os.path.join(HERE, "symmetry_traces.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d games, %d positions, %d with a qstructs order that is not the permuted one, %d B"
          % (path, GAMES, positions, order_cases, os.path.getsize(path)))


if __name__ == "__main__":
    main()
