#!/usr/bin/env python3
"""Generates tests/golden/solve_deep.npz: positions SELECTED from the C oracle's uniform play for what the exact solver
(include/qttt_solve.h) can get wrong unnoticed — values with denominator 16 and 8, the largest trees, leaf roots of
every winner — with their exact solution by make_golden_solve.py's C recursion (imported, not copied).  Nothing but
this repository's oracle is involved.  The arrays are those of solve_positions.npz.

    python tests/golden/make_golden_solve_deep.py

Per number of moves played the candidates are the first CANDIDATES[k] games of one stream of uniform play; the boards
kept are, in this order and without repeats, the classes below, then the stream's first boards up to COUNTS[k]:
  four:   the largest tree; SIXTEENTHS_4 boards with a sixteenth among their q (the smallest trees that have one, and the
          largest); one board whose value itself is an odd multiple of 1/16 or 1/8, if there is one;
  five:   the largest tree; every board with a sixteenth; EIGHTHS_5 boards with an eighth (the smallest trees); leaf roots;
          the boards that fill up have no eighth, so that tests/test_solve_deep_cpu.py can follow every board that has one;
  six to eight: every board with an eighth; leaf roots of every winner the candidates hold; at six the largest tree."""
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import oracle  # noqa: E402
from make_golden_solve import driver, positions, solve  # noqa: E402

SEED = 20261105
CANDIDATES = {4: 96, 5: 1280, 6: 2000, 7: 2000, 8: 2000}
COUNTS = {4: 6, 5: 64, 6: 256, 7: 256, 8: 256}
SIXTEENTHS_4 = 3
EIGHTHS_5 = 12
LEAVES_PER_WINNER = 4
MIN_LARGEST = {4: 29000000, 5: 1200000}
MAX_BYTES = 160000                                          # below tests/golden/step_traces.npz
WINNERS = ((1, "first"), (0, "second"), (-1, "none"))


def denominators(q):
    """The denominator 1, 2, 4, 8 or 16 of every finite entry of q (f64, any shape); 0 where q is not finite."""
    q = np.asarray(q, dtype=np.float64)
    den = np.zeros(q.shape, dtype=np.int64)
    fin = np.isfinite(q)
    for d in (16, 8, 4, 2, 1):
        den[fin & (np.where(fin, q, 0.0) * d == np.round(np.where(fin, q, 0.0) * d))] = d
    assert (den[fin] > 0).all()
    return den


def coverage(played, value, q, best, nodes, winner):
    """Per number of moves played: boards, nodes min / median / max, the count of finite q by denominator, the boards
    that have a q of denominator 16 / 8, the boards whose value has one, and the leaf roots by winner."""
    out = {}
    den, vden = denominators(q), denominators(value)
    for k in np.unique(played):
        at = played == k
        leaf = at & (best == 255)
        out[int(k)] = {
            "boards": int(at.sum()),
            "nodes": (int(nodes[at].min()), int(np.median(nodes[at])), int(nodes[at].max())),
            "q_by_denominator": {d: int((den[at] == d).sum()) for d in (1, 2, 4, 8, 16)},
            "boards_with_16": int((den[at] == 16).any(1).sum()), "boards_with_8": int((den[at] == 8).any(1).sum()),
            "value_16_or_8": int((vden[at] >= 8).sum()),
            "leaves": {name: int((leaf & (winner == w)).sum()) for w, name in WINNERS}}
    return out


def print_coverage(title, cov):
    print(title)
    print("  moves boards      nodes min / median / max           q by denominator 1 / 2 / 4 / 8 / 16   boards with 16th 8th"
          "  value 16th|8th  leaves first / second / none")
    for k, c in cov.items():
        print("  %5d %6d  %9d / %9d / %9d   %6d / %6d / %6d / %5d / %4d   %15d %4d  %13d  %6d / %6d / %4d" % (
            (k, c["boards"]) + c["nodes"] + tuple(c["q_by_denominator"][d] for d in (1, 2, 4, 8, 16))
            + (c["boards_with_16"], c["boards_with_8"], c["value_16_or_8"]) + tuple(c["leaves"][n] for _, n in WINNERS)))


def candidates(k, pool):
    """(boards, value f64[n], q f64[n, 36], best, nodes, winner) of the CANDIDATES[k] boards with k moves played."""
    ob = positions(k, CANDIDATES[k], SEED + k)
    res = pool.map(solve, [ob.b[i].tobytes() for i in range(ob.n)], chunksize=1 if k == 4 else 16)
    winner = oracle.node_info(ob)[0].astype(np.int64)
    return (ob, np.array([r[0] for r in res]), np.array([r[1] for r in res]).reshape(ob.n, 36),
            np.array([r[2] for r in res], dtype=np.uint8), np.array([r[3] for r in res], dtype=np.int64), winner)


def select(k, value, q, best, nodes, winner):
    """The indices of the candidates kept, classes first (see the module's docstring)."""
    den, vden = denominators(q), denominators(value)
    has16, has8 = (den == 16).any(1), (den == 8).any(1)
    by_size = np.argsort(nodes, kind="stable")
    keep = []

    def take(idx):
        keep.extend(int(i) for i in idx if int(i) not in keep)

    if k <= 6:
        take([np.argmax(nodes)])
    if k == 4:
        small16 = [i for i in by_size if has16[i]]
        take(small16[:SIXTEENTHS_4 - 1] + small16[-1:])
        take([i for i in by_size if vden[i] >= 8][:1])
    elif k == 5:
        take(np.flatnonzero(has16))
        take([i for i in by_size if has8[i]][:EIGHTHS_5])
    else:
        take(np.flatnonzero(has8))
    if k >= 5:
        for w, _ in WINNERS:
            take(np.flatnonzero((best == 255) & (winner == w))[:LEAVES_PER_WINNER])
    assert len(keep) <= COUNTS[k], (k, len(keep))
    if k == 4:
        take(by_size)                                       # the smallest trees fill up
    else:                                                   # five moves: no further eighths, which the CPU model has to follow
        take(i for i in range(len(nodes)) if k > 5 or not has8[i])
    return np.array(keep[:COUNTS[k]])


def check_classes(k, cand, kept):
    """The classes the fixture exists for, asserted before anything is written."""
    c, f = cand[k], kept[k]
    assert f["nodes"][2] == c["nodes"][2] and (k not in MIN_LARGEST or f["nodes"][2] >= MIN_LARGEST[k]), (k, f["nodes"])
    if k == 4:
        assert f["boards_with_16"] >= 2 and f["q_by_denominator"][16] >= 2
        if c["value_16_or_8"] == 0:
            print("  four moves: no candidate's value is an odd multiple of 1/16 or 1/8")
        else:
            assert f["value_16_or_8"] >= 1
    if k == 5:
        assert f["boards_with_16"] == c["boards_with_16"] >= 1 and f["boards_with_8"] >= 8
        assert sum(f["leaves"].values()) >= 1
    if k >= 6:
        assert f["boards_with_8"] == c["boards_with_8"] and f["boards_with_16"] == c["boards_with_16"] == 0
        for _, name in WINNERS:
            assert (f["leaves"][name] > 0) == (c["leaves"][name] > 0), (k, name)
        assert sum(f["leaves"].values()) < f["boards"]


def main():
    driver()                                                # compiled once, before the workers fork
    parts, cand_cov, kept_cov = [], {}, {}
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        for k in COUNTS:
            ob, value, q, best, nodes, winner = candidates(k, pool)
            idx = select(k, value, q, best, nodes, winner)
            played = np.full(ob.n, k)
            cand_cov.update(coverage(played, value, q, best, nodes, winner))
            kept_cov.update(coverage(played[idx], value[idx], q[idx], best[idx], nodes[idx], winner[idx]))
            parts.append((k, oracle.OracleBoards.from_records(ob.b[idx]), value[idx], q[idx], best[idx], nodes[idx], winner[idx]))
    print_coverage("candidates (seed %d)" % SEED, cand_cov)
    print_coverage("kept", kept_cov)
    for k in COUNTS:
        check_classes(k, cand_cov, kept_cov)
    every = [w for k in (6, 7, 8) for w, n in kept_cov[k]["leaves"].items() if n]
    assert set(every) == {"first", "second", "none"}, every   # over six to eight moves every winner has a leaf root
    cat = lambda f: np.concatenate([f(p) for p in parts])  # noqa: E731
    v64, q64 = cat(lambda p: p[2]), cat(lambda p: p[3])
    assert np.array_equal(v64 * 16, np.round(v64 * 16))
    out = {"played": cat(lambda p: np.full(p[1].n, p[0], dtype=np.uint8)),
           "moves": cat(lambda p: p[1].moves), "n_moves": cat(lambda p: p[1].n_moves),
           "board": cat(lambda p: p[1].board), "qmask": cat(lambda p: p[1].qmask), "n_q": cat(lambda p: p[1].n_q),
           "value": v64.astype(np.float32), "q": q64.astype(np.float32),
           "best": cat(lambda p: p[4]), "nodes": cat(lambda p: p[5])}
    path = os.path.join(HERE, "solve_deep.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote %s: %d boards, %d bytes" % (path, len(out["best"]), size))
    assert size < MAX_BYTES, size


if __name__ == "__main__":
    main()
