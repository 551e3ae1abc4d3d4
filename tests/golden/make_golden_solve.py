#!/usr/bin/env python3
"""Generates tests/golden/solve_positions.npz: late positions from the C oracle's uniform play with their exact
expectimax solution (include/qttt_solve.h) — value, q, best, nodes — computed by a small C recursion compiled here
against oracle/qttt_oracle.c.  Nothing but this repository's oracle is involved.

    python tests/golden/make_golden_solve.py

Recorded: 2 boards with four moves played (the two with the fewest nodes of CANDIDATES_4), 8 with five, and 32 each
with six, seven and eight, leaf roots among them, in the reference-shaped arrays VecEnv.import_boards takes."""
import ctypes
import multiprocessing
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import oracle  # noqa: E402

SEED = 20261020
CANDIDATES_4 = 24
COUNTS = {4: 2, 5: 8, 6: 32, 7: 32, 8: 32}

DRIVER = r"""
#include <math.h>
#include "qttt_oracle.h"

/* moves played: len(moves) without the autofill move (lo == hi) */
static int played(const qo_board *b) {
    int n = b->n_moves;
    return (n && b->moves[n - 1][0] == b->moves[n - 1][1]) ? n - 1 : n;
}
static double leaf_value(const qo_board *b, int winner) {
    if (winner < 0) return 0.0;
    return ((winner == 1) == (played(b) % 2 == 0)) ? 1.0 : -1.0;
}
static double value_of(const qo_board *b, int64_t *nodes);
/* Q(a); returns 0 where the expansion has no child */
static int q_of(const qo_board *b, int a, double *q, int64_t *nodes) {
    qo_board child[2];
    int w[2], t[2];
    uint64_t lm[2];
    int k = qo_expand(b, a, child, w, t, lm);
    if (k == 0) return 0;
    double sum = 0.0;
    for (int c = 0; c < k; ++c) sum += value_of(&child[c], nodes);
    *q = k == 1 ? 0.0 - sum : 0.0 - sum / 2.0;
    return 1;
}
static double value_of(const qo_board *b, int64_t *nodes) {
    int winner, terminal;
    qo_update_winner(b, &winner, &terminal);
    uint64_t legal = qo_legal_mask(b);
    *nodes += 1;
    if (terminal || legal == 0) return leaf_value(b, winner);
    double best = -INFINITY, q;
    for (int a = 0; a < 36; ++a)
        if ((legal >> a & 1) && q_of(b, a, &q, nodes) && q > best) best = q;
    return best;
}
int solve_board(const qo_board *b, double *value, double *q36, int *best, int64_t *nodes) {
    int winner, terminal;
    qo_update_winner(b, &winner, &terminal);
    uint64_t legal = qo_legal_mask(b);
    *nodes = 1;
    *best = 255;
    for (int a = 0; a < 36; ++a) q36[a] = -INFINITY;
    if (terminal || legal == 0) { *value = leaf_value(b, winner); return 1; }
    *value = -INFINITY;
    for (int a = 0; a < 36; ++a)
        if ((legal >> a & 1) && q_of(b, a, &q36[a], nodes) && q36[a] > *value) { *value = q36[a]; *best = a; }
    return 0;
}
"""

_driver = None


def driver():
    global _driver
    if _driver is None:
        d = tempfile.mkdtemp(prefix="qttt_solve_driver_")
        src, so = os.path.join(d, "solve_driver.c"), os.path.join(d, "solve_driver.so")
        with open(src, "w") as f:
            f.write(DRIVER)
        odir = os.path.join(ROOT, "oracle")
        subprocess.check_call([os.environ.get("CC", "gcc"), "-O2", "-std=c99", "-shared", "-fPIC", "-I" + odir, "-o", so, src,
                               os.path.join(odir, "qttt_oracle.c"), "-lm"])
        _driver = ctypes.CDLL(so)
    return _driver


def solve(rec_bytes):
    buf = ctypes.create_string_buffer(rec_bytes, 48)
    value, q, best, nodes = ctypes.c_double(), (ctypes.c_double * 36)(), ctypes.c_int(), ctypes.c_int64()
    driver().solve_board(buf, ctypes.byref(value), q, ctypes.byref(best), ctypes.byref(nodes))
    return value.value, list(q), best.value, nodes.value


def played(ob):
    n = ob.b["n_moves"].astype(np.int64)
    last = ob.b["moves"][np.arange(ob.n), np.maximum(n - 1, 0)]
    return n - ((n > 0) & (last[:, 0] == last[:, 1]))


def positions(k, want, seed):
    """The first `want` games of the oracle's uniform play (qo_sample_action, hashed collapse bits) that reach k moves
    played, at that point — finished or not."""
    n = 8 * want + 64
    ob = oracle.OracleBoards(n)
    alive = np.ones(n, dtype=bool)
    for t in range(k):
        alive &= ob.terminated() == 0                       # a game that ended earlier never has k moves
        ob.step(ob.sample_actions(seed, t), None, seed, t)
    keep = np.flatnonzero(alive & (played(ob) == k))[:want]
    assert len(keep) == want, (k, len(keep))
    return oracle.OracleBoards.from_records(ob.b[keep])


def main():
    parts = []
    driver()                                                # compiled once, before the workers fork
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        for k, want in COUNTS.items():
            ob = positions(k, CANDIDATES_4 if k == 4 else want, SEED + k)
            res = pool.map(solve, [ob.b[i].tobytes() for i in range(ob.n)])
            if k == 4:
                order = sorted(range(ob.n), key=lambda i: res[i][3])[:want]
                ob, res = oracle.OracleBoards.from_records(ob.b[order]), [res[i] for i in order]
            parts.append((k, ob, res))
            print("%d moves played: %d boards, nodes %d .. %d, leaves %d" % (
                k, ob.n, min(r[3] for r in res), max(r[3] for r in res), sum(r[2] == 255 for r in res)))
    cat = lambda f: np.concatenate([f(k, ob, res) for k, ob, res in parts])  # noqa: E731
    v64 = cat(lambda k, ob, res: np.array([r[0] for r in res], dtype=np.float64))
    q64 = cat(lambda k, ob, res: np.array([r[1] for r in res], dtype=np.float64))
    assert np.array_equal(v64 * 16, np.round(v64 * 16))
    out = {"played": cat(lambda k, ob, res: np.full(ob.n, k, dtype=np.uint8)),
           "moves": cat(lambda k, ob, res: ob.moves), "n_moves": cat(lambda k, ob, res: ob.n_moves),
           "board": cat(lambda k, ob, res: ob.board), "qmask": cat(lambda k, ob, res: ob.qmask),
           "n_q": cat(lambda k, ob, res: ob.n_q),
           "value": v64.astype(np.float32), "q": q64.astype(np.float32),
           "best": cat(lambda k, ob, res: np.array([r[2] for r in res], dtype=np.uint8)),
           "nodes": cat(lambda k, ob, res: np.array([r[3] for r in res], dtype=np.int64))}
    leaves = out["best"] == 255
    assert leaves[out["played"] >= 6].any() and not leaves[out["played"] >= 6].all()
    path = os.path.join(HERE, "solve_positions.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d boards, %d bytes" % (path, len(out["best"]), os.path.getsize(path)))


if __name__ == "__main__":
    main()
